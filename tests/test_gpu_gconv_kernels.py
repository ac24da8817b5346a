"""Grouped conv kernel (csrc/pv_gconv.hip, pv_conv3d_desc.groups) on the MI355X against F.conv3d(groups=G) in float64.

Reference: the conv of the bf16-rounded input and weights, then scale / shift / activation, all in float64.  Bound per
element: |got - want| <= 2^-8 |want| + K 2^-23 S, K = taps * gw, S = the same conv of |x| and |w| times |scale| -- one bf16
rounding of the result plus an fp32 accumulation of K products in any order.  Weights have std K^-1/2, so a dropped or
misplaced tap or a cross-wired group moves an element by about |want| / sqrt(taps).

Shapes: the kernel's tiles are 8 x 16 output voxels (8 x 8 on planes of at most 8 columns, 4 x 16 with 32-channel slabs where
a W-strided halo does not fit otherwise); 9 x 17 outputs make both edges ragged and put a halo across a tile seam.  T = 6 / 7
is longer than the ring of kt + 1 planes; 80 / 96 channels leave a ragged last slab."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import CANARY, _routed_kernel, call, rel_err

pytestmark = pytest.mark.gpu
NONE, RELU, SWISH = L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH

#        gw  C   kernel     stride     padding    T  H   W   act    affine
CASES = [
    (16, 80, (3, 3, 3), (1, 1, 1), (1, 1, 1), 6, 9, 17, RELU, True),     # slabs of 4 + 1 groups
    (32, 96, (3, 3, 3), (1, 1, 1), (1, 1, 1), 6, 9, 17, SWISH, True),
    (16, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1, 17, 33, NONE, False),   # one group, one frame, odd planes under stride 2
    (16, 32, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1, 17, 33, NONE, False),   # the same on the grouped kernel: two groups, one slab
    (32, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1, 17, 33, RELU, True),
    (16, 80, (3, 1, 1), (2, 1, 1), (1, 0, 0), 7, 9, 17, NONE, True),
    (32, 96, (3, 1, 1), (2, 1, 1), (1, 0, 0), 7, 9, 17, RELU, False),
    (16, 80, (3, 3, 3), (1, 2, 2), (1, 1, 1), 6, 17, 33, SWISH, True),   # 32-channel slabs (2 + 2 + 1 groups), 4 x 16 tiles
    (32, 64, (3, 3, 3), (2, 1, 1), (0, 0, 0), 7, 11, 9, NONE, True),     # no padding; 9 x 7 outputs on 8 x 8 tiles
]


def _desc(x, w, y, gw, C_, k, s, p, act, scale=None, shift=None, **kw):
    B, Ti, Hi, Wi = x["B"], x["T"], x["H"], x["W"]
    To, Ho, Wo = [(i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip((Ti, Hi, Wi), k, s, p)]
    d = L.Conv3dDesc(x=x["ptr"], w=w.data_ptr(), y=y["ptr"], x_bs=x["bs"], y_bs=y["bs"], ldx=x["ld"], ldy=y["ld"],
                     B=B, Ti=Ti, Hi=Hi, Wi=Wi, cin=C_, To=To, Ho=Ho, Wo=Wo, cout=C_, kt=k[0], kh=k[1], kw=k[2],
                     st=s[0], sh=s[1], sw=s[2], pt=p[0], ph=p[1], pw=p[2], act=act, dtype=L.PV_BF16, groups=C_ // gw)
    kw.update(scale=scale.data_ptr() if scale is not None else None, shift=shift.data_ptr() if shift is not None else None)
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _buffer(B, T, H, W, C_, fill):
    """Channel slice [8, 8 + C) of rows of C + 24 elements, a gap of 64 elements behind every batch item."""
    ld, bs = C_ + 24, T * H * W * (C_ + 24) + 64
    buf = torch.full((B * bs,), fill, dtype=torch.bfloat16, device="cuda")
    rows = lambda t: torch.as_strided(t, (B, T, H, W, ld), (bs, H * W * ld, W * ld, ld, 1))
    return dict(buf=buf, rows=rows, view=rows(buf)[..., 8: 8 + C_], ptr=buf.data_ptr() + 16, bs=bs, ld=ld, B=B, T=T, H=H, W=W)


@pytest.mark.parametrize("gw,C_,k,s,p,T,H,W,act,affine", CASES)
def test_grouped_conv_matches_float64(gw, C_, k, s, p, T, H, W, act, affine):
    g = torch.Generator().manual_seed(gw * 1000 + C_ + T)
    B, taps = 2, k[0] * k[1] * k[2]
    K = taps * gw
    x = torch.randn(B, C_, T, H, W, generator=g).bfloat16()
    w = (torch.randn(C_, gw, *k, generator=g) * K ** -0.5).bfloat16()
    scale = torch.rand(C_, generator=g) + 0.5 if affine else None
    shift = torch.randn(C_, generator=g) * 0.5 if affine else None
    conv = lambda a, b: F.conv3d(a.double(), b.double(), stride=s, padding=p, groups=C_ // gw)
    acc, S = conv(x, w), conv(x.abs(), w.abs())
    if affine:
        acc = acc * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1)
        S = S * scale.double().view(1, -1, 1, 1, 1)
    want = torch.relu(acc) if act == RELU else acc * torch.sigmoid(acc) if act == SWISH else acc
    bound = 2.0 ** -8 * want.abs() + K * 2.0 ** -23 * S

    xb = _buffer(B, T, H, W, C_, float("nan"))
    xb["view"].copy_(x.permute(0, 2, 3, 4, 1))
    yb = _buffer(B, *want.shape[2:], C_, CANARY)
    wd = w.permute(0, 2, 3, 4, 1).contiguous().cuda()                    # [cout][taps][gw]
    sc, sh = (scale.cuda(), shift.cuda()) if affine else (None, None)
    d = _desc(xb, wd, yb, gw, C_, k, s, p, act, sc, sh)
    # C of exactly one group is groups = 1, which the ABI defines as dense: same weights, the dense kernels
    assert L.lib().pv_conv3d_grouped_supported(C.byref(d)) == (1 if C_ > gw else 0)
    call("pv_conv3d", d)
    got = yb["view"].permute(0, 4, 1, 2, 3).double().cpu()
    err = (got - want).abs()
    print("max err %.3e, worst err / bound %.3f" % (err.max(), (err / bound.clamp_min(1e-30)).max()))
    assert bool((err <= bound).all()), "worst element %s" % (torch.unravel_index((err - bound).argmax(), err.shape),)
    # everything outside the slice is as it went in (C is a multiple of 16: no padding channels inside round_up(C, 8))
    rest = yb["buf"].clone()
    yb["rows"](rest)[..., 8: 8 + C_] = CANARY
    assert bool((rest == CANARY).all())


def test_route_is_the_grouped_kernel():
    xb, yb = _buffer(1, 2, 9, 17, 64, 0.0), _buffer(1, 2, 9, 17, 64, CANARY)
    w = torch.zeros(64, 9, 16, dtype=torch.bfloat16, device="cuda")
    d = _desc(xb, w, yb, 16, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), RELU)
    assert "gconv_plane_kernel" in _routed_kernel(L.OP_CONV3D, d)


@pytest.mark.parametrize("gw,kw", [(24, {}), (16, dict(dtype=L.PV_F32)), (16, dict(residual=True))],
                         ids=["gw24", "fp32", "residual"])
def test_out_of_range_descriptors_are_unsupported(gw, kw):
    C_ = 2 * gw
    xb, yb = _buffer(1, 1, 4, 4, C_, 0.0), _buffer(1, 1, 4, 4, C_, CANARY)
    w = torch.zeros(C_, 9, gw, dtype=torch.float32, device="cuda")
    if kw.get("residual"):
        kw = dict(residual=yb["ptr"], ldr=yb["ld"], r_bs=yb["bs"])
    d = _desc(xb, w, yb, gw, C_, (1, 3, 3), (1, 1, 1), (0, 1, 1), NONE, **kw)
    assert L.lib().pv_conv3d_grouped_supported(C.byref(d)) == 0
    assert L.lib().pv_conv3d(C.byref(d), None) == L.PV_ERR_UNSUPPORTED
    assert bool((yb["buf"] == CANARY).all())


def test_resnext_matches_the_host_mirror():
    """32 groups, inner widths 128 / 256 / 512 / 1024 (4, 8, 16, 32 channels per group), bf16, as tests/test_gpu_models.py."""
    from oracle.weights import deterministic_fill, quantize_like_kernels, seeded_input
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet
    cfg = dict(model_depth=50, model_num_class=9, stem_dim_out=128, stage_conv_b_num_groups=(32, 32, 32, 32),
               head_pool_kernel_size=(4, 2, 2))
    torch.manual_seed(0)
    m = deterministic_fill(create_resnet(**cfg), 6).eval()
    ref = create_resnet(**cfg).eval()
    ref.load_state_dict(quantize_like_kernels(m.state_dict()))
    x = seeded_input((1, 3, 4, 64, 64), 6)
    with torch.no_grad():
        want = ref(x.bfloat16().float())
    transmute_model(m, "mi355x")
    dm = convert_to_deployable_form(m, x.cuda().bfloat16(), dtype=torch.bfloat16)
    got = dm(x.cuda().bfloat16())
    assert got.shape == want.shape and rel_err(got.float(), want) <= 1e-2
    assert getattr(dm, "_pv_inputs", None) is not None     # nothing declined: one launch plan
