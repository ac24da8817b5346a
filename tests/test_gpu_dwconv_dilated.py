"""Dilated depthwise / channel-wise grouped conv (pv_dwconv3d_desc.dil_t / dil_h / dil_w) on the MI355X against
F.conv3d(dilation=, groups=) in float64 on the same bf16-rounded inputs, with the buffers, checks and tolerances of gpu_util (y: fp32
1e-3, bf16 1e-2 of the abs-max; the psum mean 1e-3).  B = 2 with a batch gap, C = 53 (56 grouped), rows of round_up(C, 8) + 8.
dw3_plane_kernel (bf16 3x3x3 stride 1 "same"): a phase (ho = i dil_h + rh, wo = j dil_w + rw) is tiled 4 x 8 on its own extent.
dwconv_kernel: everything else dilated -- dil_t, kt != 3, a strided dilated dimension, other padding, gw 2 / 4 / 8, fp32."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import _routed_kernel, call, rel_err

pytestmark = pytest.mark.gpu
NONE, RELU, SWISH = L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH
B, K3, S1 = 2, (3, 3, 3), (1, 1, 1)
_cdiv = lambda a, b: -(-a // b)


def _make(dtype, T, H, W, k, s, pad, dil, act, gw=0, seed=1001):
    """-> (inputs on the CPU, geometry fields of the descriptor, pre-activation reference (B, rows, C), Expect for y)"""
    Cc, g = (56, gw) if gw else (53, 1)
    cp = U.round_up8(Cc)
    out = [(n + 2 * p - ((kk - 1) * d + 1)) // ss + 1 for n, kk, ss, p, d in zip((T, H, W), k, s, pad, dil)]
    ldx, ldy, Rx, Ry = cp + 8, cp + 8, T * H * W, out[0] * out[1] * out[2]
    f = dict(B=B, Ti=T, Hi=H, Wi=W, C=Cc, To=out[0], Ho=out[1], Wo=out[2], kt=k[0], kh=k[1], kw=k[2], st=s[0], sh=s[1], sw=s[2],
             pt=pad[0], ph=pad[1], pw=pad[2], dil_t=dil[0], dil_h=dil[1], dil_w=dil[2], act=act, gw=gw, ldx=ldx, ldy=ldy,
             x_bs=Rx * ldx + 16, y_bs=Ry * ldy + 32, dtype=L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    wref = U.randn((Cc, g) + tuple(k), seed + 1, (g * k[0] * k[1] * k[2]) ** -0.5 * 1.7)
    i = dict(x=U.rows_buf(U.randn((B, Rx, Cc), seed), ldx, dtype, bs=f["x_bs"]), y0=U.canary_buf(B, f["y_bs"], dtype),
             w=U.pack_dw_weights(wref, cp), scale=U.randn((Cc,), seed + 2, 0.2, 1.0), shift=U.randn((Cc,), seed + 3, 0.5, 0.25))
    xd = U.rows_of(i["x"], Rx, ldx, Cc).double().reshape(B, T, H, W, Cc).permute(0, 4, 1, 2, 3)
    pre = F.conv3d(xd, wref.double(), None, stride=s, padding=pad, dilation=dil, groups=Cc // g).permute(0, 2, 3, 4, 1)
    pre = (pre * i["scale"].double() + i["shift"].double()).reshape(B, Ry, Cc)
    return i, f, pre, U.Expect(U.ref_act(pre, act), i["y0"], ldy, tol=U.TOL[dtype])


def _desc(t, f, psum=None, **more):
    d = L.DwConv3dDesc(**dict(f, **more))
    d.x, d.w, d.y, d.scale, d.shift = (t[k].data_ptr() for k in ("x", "w", "y0", "scale", "shift"))
    d.psum = psum.data_ptr() if psum is not None else None
    return d


def _run(made, want_psum, blocks, symbol):
    i, f, pre, expect = made
    t = {k: v.cuda() for k, v in i.items()}
    assert L.lib().pv_dwconv3d_psum_blocks(C.byref(_desc(t, f))) == blocks
    assert L.lib().pv_dwconv3d_pw_supported(C.byref(_desc(t, f))) == 0
    assert _routed_kernel(L.OP_DWCONV3D, _desc(t, f)) == symbol
    t = {k: v.cuda() for k, v in i.items()}          # the routing launch wrote y: check a fresh buffer
    psum = torch.full((B * blocks + 1, U.round_up8(f["C"])), float("nan"), device="cuda") if want_psum else None
    call("pv_dwconv3d", _desc(t, f, psum))
    print("y error %.3e of the abs-max" % expect.check(t["y0"], symbol))
    if want_psum:
        print("psum mean error %.3e" % U.check_psum(psum, pre, dict(B=B, C=f["C"]), blocks, U.PSUM_TOL, symbol))


@pytest.mark.parametrize("T,H,W,dil,act,psum", [
    (3, 11, 11, (1, 2, 2), RELU, True),        # phases of 6 and 5 rows / columns
    (1, 3, 9, (1, 4, 1), NONE, False),         # H only; Ho = 3 < dil_h: phase 3 has no outputs and no workgroups
    (1, 5, 37, (1, 1, 2), SWISH, True),        # W only; 19 and 18 columns: three 8-column tiles per phase
    (3, 6, 10, (1, 3, 2), SWISH, False),       # unequal dilations
    (2, 9, 9, (1, 2, 1), NONE, True),          # even T: the other exit of the two-plane walk
], ids=["11x11_d22", "h3_d41", "w37_d12", "6x10_d32", "9x9_d21"])
def test_plane_kernel_polyphase(T, H, W, dil, act, psum):
    blocks = sum(_cdiv(_cdiv(H - r, dil[1]), 4) for r in range(min(dil[1], H))) * \
        sum(_cdiv(_cdiv(W - r, dil[2]), 8) for r in range(min(dil[2], W)))
    _run(_make(torch.bfloat16, T, H, W, K3, S1, dil, dil, act), psum, blocks, "dw3_plane_kernel")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("T,H,W,k,s,pad,dil,act,psum,gw", [
    (5, 4, 5, (3, 1, 1), S1, (2, 0, 0), (2, 1, 1), RELU, True, 0),             # dil_t
    (2, 7, 9, (1, 3, 3), S1, (0, 2, 2), (1, 2, 2), SWISH, True, 0),            # kt != 3 keeps bf16 off the plane kernel
    (3, 9, 10, K3, (1, 2, 2), (1, 2, 2), (1, 2, 2), NONE, False, 0),           # a strided dilated dimension
    (3, 9, 10, K3, S1, (1, 1, 3), (1, 2, 2), NONE, False, 0),                  # not the "same" padding
    (2, 5, 6, K3, S1, (1, 2, 2), (1, 2, 2), RELU, True, 2),
    (2, 5, 6, K3, S1, (1, 2, 2), (1, 2, 2), SWISH, False, 4),
    (2, 5, 6, K3, S1, (1, 2, 2), (1, 2, 2), NONE, True, 8),
], ids=["dil_t", "k133", "strided", "pad", "gw2", "gw4", "gw8"])
def test_generic_kernel_dilated(T, H, W, k, s, pad, dil, act, psum, gw, dtype):
    made = _make(dtype, T, H, W, k, s, pad, dil, act, gw=gw)
    f = made[1]
    blocks = _cdiv(f["To"] * f["Ho"] * f["Wo"], 256 // (U.round_up8(f["C"]) // 8))     # one output per thread
    _run(made, psum, blocks, "dwconv_kernel")


@pytest.mark.parametrize("change,status", [(dict(n_prefix=1), L.PV_ERR_UNSUPPORTED), (dict(pw_w=1, pw_cin=24), L.PV_ERR_UNSUPPORTED),
                                           (dict(dil_w=-1), L.PV_ERR_INVALID)], ids=["n_prefix", "pw_w", "negative"])
def test_dilated_refusals_launch_nothing(change, status):
    i, f, _, _ = _make(torch.bfloat16, 1, 5, 9, K3, S1, (1, 2, 2), (1, 2, 2), NONE)
    t = {k: v.cuda() for k, v in i.items()}
    d = _desc(t, f, **{k: (t["w"].data_ptr() if k == "pw_w" else v) for k, v in change.items()})
    assert L.lib().pv_dwconv3d_pw_supported(C.byref(d)) == 0
    assert L.lib().pv_dwconv3d(C.byref(d), U.stream()) == status
    torch.cuda.synchronize()
    assert torch.equal(t["y0"].cpu(), i["y0"])


def test_depthwise_detection_backbone_matches_the_oracle():
    """create_resnet_with_roi_head at toy size, depthwise (3,3,3) conv_b in every stage, res5 dilated (1, 2, 2), in bf16 against the
    fp32 oracle on the bf16-rounded weights and input, under the bound of tests/test_gpu_models.py (1e-2 of the abs-max)."""
    from oracle import functional as OF
    from oracle.weights import detection_fill, quantize_like_kernels, seeded_input
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    torch.manual_seed(0)
    m = detection_fill(create_resnet_with_roi_head(model_num_class=9, stem_dim_out=32, stage_conv_b_kernel_size=(K3,) * 4,
                                                   stage_conv_b_num_groups=(32, 64, 128, 256)), 6).eval()
    conv_b = m.model.blocks[4].res_blocks[0].branch2.conv_b
    assert conv_b.groups == conv_b.in_channels == 256 and conv_b.dilation == (1, 2, 2)
    x = seeded_input((2, 3, 4, 64, 96), 6)
    boxes = torch.tensor([[0, 4.0, 6.0, 40.0, 30.0], [1, 0.0, 0.0, 95.0, 63.0], [1, 30.0, 20.0, 70.5, 50.2]])
    want = OF.resnet_detection_forward(quantize_like_kernels(m.state_dict()), x.bfloat16().float(), boxes)
    assert 0.0 < want.min().item() and want.max().item() < 1.0      # not saturated
    transmute_model(m, "mi355x")
    dm = convert_to_deployable_form(m, (x.cuda().bfloat16(), boxes), dtype=torch.bfloat16)
    got = dm(x.cuda().bfloat16(), boxes)
    assert got.shape == want.shape and rel_err(got.float(), want) <= 1e-2
