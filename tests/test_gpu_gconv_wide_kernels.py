"""Wide grouped conv kernel (csrc/pv_gconv_wide.hip: 64 / 128 channels per group) on the MI355X against
F.conv3d(groups=G) in float64, by the method and the bound of tests/test_gpu_gconv_kernels.py:
|got - want| <= 2^-8 |want| + K 2^-23 S, K = taps * gw, S = the same conv of |x| and |w| times |scale|.

Tiles are 8 x 16 output voxels, 4 x 16 / 8 x 8 / 4 x 8 where the ring of kt + 1 halo planes does not fit otherwise (8 x 8 first on
planes of at most 8 columns); gw = 128 with kernel (3,3,3) under a spatial stride of 2 fits only 4 x 8 with a ring of kt planes."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
from gpu_util import CANARY, _routed_kernel, call
from test_gpu_gconv_kernels import _buffer, _desc

pytestmark = pytest.mark.gpu
NONE, RELU, SWISH = L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH

#        gw   C    kernel     stride     padding    T  H   W   act    affine
CASES = [
    (64, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), 6, 9, 17, RELU, True),     # two groups; ragged tiles; ring wrap; 27 taps streamed
    (64, 192, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1, 17, 33, NONE, False),   # one frame; odd planes under stride 2; 4 x 16 tiles
    (64, 128, (3, 1, 1), (2, 1, 1), (1, 0, 0), 7, 9, 17, SWISH, True),    # temporal stride 2; the frame before the clip is zero
    (128, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), 2, 9, 17, RELU, False),   # four row tiles per group, four voxel tiles per wave
    (128, 256, (3, 3, 3), (1, 2, 2), (1, 1, 1), 6, 17, 33, SWISH, True),  # 4 x 8 tiles, ring of kt planes; stride-2 halo
    (128, 384, (3, 3, 3), (2, 1, 1), (0, 0, 0), 7, 11, 9, NONE, True),    # no padding; 9 x 7 outputs on 8 x 8 tiles; three groups
]


@pytest.mark.parametrize("gw,C_,k,s,p,T,H,W,act,affine", CASES)
def test_wide_grouped_conv_matches_float64(gw, C_, k, s, p, T, H, W, act, affine):
    g = torch.Generator().manual_seed(gw * 1000 + C_ + T)
    B, K = 2, k[0] * k[1] * k[2] * gw
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
    assert L.lib().pv_conv3d_grouped_supported(C.byref(d)) == 1
    call("pv_conv3d", d)
    got = yb["view"].permute(0, 4, 1, 2, 3).double().cpu()
    err = (got - want).abs()
    print("max err %.3e, worst err / bound %.3f" % (err.max(), (err / bound.clamp_min(1e-30)).max()))
    assert bool((err <= bound).all()), "worst element %s" % (torch.unravel_index((err - bound).argmax(), err.shape),)
    rest = yb["buf"].clone()                                             # everything outside the slice is as it went in
    yb["rows"](rest)[..., 8: 8 + C_] = CANARY
    assert bool((rest == CANARY).all())


@pytest.mark.parametrize("gw,kernel", [(64, "gconv_wide_kernel"), (16, "gconv_plane_kernel")])
def test_route_by_group_width(gw, kernel):
    C_ = 2 * gw
    xb, yb = _buffer(1, 2, 9, 17, C_, 0.0), _buffer(1, 2, 9, 17, C_, CANARY)
    w = torch.zeros(C_, 9, gw, dtype=torch.bfloat16, device="cuda")
    d = _desc(xb, w, yb, gw, C_, (1, 3, 3), (1, 1, 1), (0, 1, 1), RELU)
    assert kernel in _routed_kernel(L.OP_CONV3D, d)
