"""Dilated grouped conv (the polyphase form of csrc/pv_gconv.hip and csrc/pv_gconv_wide.hip) on the MI355X against
F.conv3d(dilation=, groups=) in float64, by the method, the buffers and the bound of tests/test_gpu_gconv_kernels.py:
|got - want| <= 2^-8 |want| + K 2^-23 S, K = taps * gw, S = the same conv of |x| and |w| times |scale|.  A phase is the outputs
h = i dh + rh, w = j dw + rw, tiled on its own: 11 x 11 under dilation 2 has phases of 6 and 5 rows / columns, H = 3 under
dil_h = 4 leaves phase 3 empty, W = 37 under dil_w = 2 is wider than one 16-column tile.  B = 2."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import CANARY, _routed_kernel, call, rel_err
from test_gpu_gconv_kernels import _buffer, _desc

pytestmark = pytest.mark.gpu
NONE, RELU, SWISH = L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH
#        groups kernel     stride     padding    dilation   T  H   W   act    affine
CASES = [(5, (1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2), 2, 11, 11, RELU, True),     # "same"; phases of 6 and 5; gw 16: ragged slab
         (2, (3, 3, 3), (2, 1, 1), (1, 0, 0), (1, 2, 2), 5, 11, 11, NONE, False),    # 27 taps, T stride 2, no spatial padding
         (2, (1, 3, 3), (1, 1, 1), (0, 4, 1), (1, 4, 1), 1, 3, 9, NONE, True),       # Ho = 3 < dil_h: phase 3 has no outputs
         (2, (1, 3, 3), (1, 1, 1), (0, 2, 1), (1, 2, 1), 1, 9, 17, SWISH, False),    # H dilated only
         (2, (1, 3, 3), (1, 2, 1), (0, 1, 3), (1, 1, 3), 1, 9, 17, RELU, True),      # W dilated only, stride 2 in the undilated H
         (2, (1, 3, 3), (1, 1, 1), (0, 1, 2), (1, 1, 2), 1, 9, 37, NONE, False)]     # phases of 19 and 18 columns: two tiles each


def _dilated(x, w, y, gw, C_, k, s, p, dil, act, sc=None, sh=None):
    To, Ho, Wo = [(i + 2 * pp - ((kk - 1) * dd + 1)) // ss + 1 for i, kk, ss, pp, dd in zip((x["T"], x["H"], x["W"]), k, s, p, dil)]
    return _desc(x, w, y, gw, C_, k, s, p, act, sc, sh, To=To, Ho=Ho, Wo=Wo, dil_t=dil[0], dil_h=dil[1], dil_w=dil[2])


@pytest.mark.parametrize("G,k,s,p,dil,T,H,W,act,affine", CASES)
@pytest.mark.parametrize("gw", [16, 32, 64, 128])
def test_dilated_grouped_conv_matches_float64(gw, G, k, s, p, dil, T, H, W, act, affine):
    C_ = gw * (G if gw < 64 else 2)
    g = torch.Generator().manual_seed(gw * 1000 + C_ + W)
    B, K = 2, k[0] * k[1] * k[2] * gw
    x = torch.randn(B, C_, T, H, W, generator=g).bfloat16()
    w = (torch.randn(C_, gw, *k, generator=g) * K ** -0.5).bfloat16()
    scale, shift = (torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.5) if affine else (torch.ones(C_), torch.zeros(C_))
    conv = lambda a, b: F.conv3d(a.double(), b.double(), stride=s, padding=p, dilation=dil, groups=C_ // gw)
    acc = conv(x, w) * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
    S = conv(x.abs(), w.abs()) * scale.double().view(1, -1, 1, 1, 1)
    want = torch.relu(acc) if act == RELU else acc * torch.sigmoid(acc) if act == SWISH else acc
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * S

    xb, yb = _buffer(B, T, H, W, C_, float("nan")), _buffer(B, *want.shape[2:], C_, CANARY)
    xb["view"].copy_(x.permute(0, 2, 3, 4, 1))
    wd = w.permute(0, 2, 3, 4, 1).contiguous().cuda()                    # [cout][taps][gw]
    d = _dilated(xb, wd, yb, gw, C_, k, s, p, dil, act, *((scale.cuda(), shift.cuda()) if affine else ()))
    assert L.lib().pv_conv3d_grouped_supported(C.byref(d)) == 1
    call("pv_conv3d", d)
    err = (yb["view"].permute(0, 4, 1, 2, 3).double().cpu() - want).abs()
    print("max err %.3e, worst err / bound %.3f" % (err.max(), (err / bound.clamp_min(1e-30)).max()))
    assert bool((err <= bound).all()), "worst element %s" % (torch.unravel_index((err - bound).argmax(), err.shape),)
    rest = yb["buf"].clone()             # padding rows, the batch gap and the channels beyond C are as they went in
    yb["rows"](rest)[..., 8: 8 + C_] = CANARY
    assert bool((rest == CANARY).all())
    assert ("gconv_wide_kernel" if gw >= 64 else "gconv_plane_kernel") in _routed_kernel(L.OP_CONV3D, d)


@pytest.mark.parametrize("s,p,dil,out", [((1, 1, 1), (2, 1, 1), (2, 1, 1), (5, 9, 9)), ((1, 2, 1), (0, 2, 1), (1, 2, 1), (3, 5, 9))],
                         ids=["dil_t", "strided_dilated_h"])
def test_out_of_scope_dilations_are_unsupported(s, p, dil, out):
    xb, yb, w = _buffer(1, 5, 9, 9, 32, 0.0), _buffer(1, *out, 32, CANARY), torch.zeros(32, 27, 16, dtype=torch.bfloat16, device="cuda")
    d = _dilated(xb, w, yb, 16, 32, (3, 3, 3), s, p, dil, NONE)
    assert (d.To, d.Ho, d.Wo) == out             # a valid conv: what is refused is the route, not the geometry
    assert L.lib().pv_conv3d_grouped_supported(C.byref(d)) == 0 and L.lib().pv_conv3d(C.byref(d), None) == L.PV_ERR_UNSUPPORTED
    assert bool((yb["buf"] == CANARY).all())


def test_resnext_detection_backbone_matches_the_oracle():
    """A ResNeXt-style create_resnet_with_roi_head at toy size (res4: 8 groups of 16, stride 2; res5: 16 groups of 16, stride 1,
    conv_b dilated (1, 2, 2)) in bf16 against the fp32 oracle on the bf16-rounded weights and input, under the bound of
    tests/test_gpu_models.py (1e-2 of the output's abs-max)."""
    from oracle import functional as OF
    from oracle.weights import detection_fill, quantize_like_kernels, seeded_input
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    torch.manual_seed(0)
    m = detection_fill(create_resnet_with_roi_head(model_num_class=9, stem_dim_out=32, stage_conv_b_num_groups=(1, 1, 8, 16)), 6).eval()
    x = seeded_input((2, 3, 4, 64, 96), 6)
    boxes = torch.tensor([[0, 4.0, 6.0, 40.0, 30.0], [1, 0.0, 0.0, 95.0, 63.0], [1, 30.0, 20.0, 70.5, 50.2]])
    want = OF.resnet_detection_forward(quantize_like_kernels(m.state_dict()), x.bfloat16().float(), boxes)
    assert 0.0 < want.min().item() and want.max().item() < 1.0      # not saturated
    transmute_model(m, "mi355x")
    dm = convert_to_deployable_form(m, (x.cuda().bfloat16(), boxes), dtype=torch.bfloat16)
    got = dm(x.cuda().bfloat16(), boxes)
    assert got.shape == want.shape and rel_err(got.float(), want) <= 1e-2
