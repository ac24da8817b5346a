"""Shared by tests/test_transforms_spatial.py and tests/test_gpu_resample.py: the seeded inputs of
tests/golden/make_spatial_golden.py, the pinned bilinear formula of include/pv_mi355x.h restated in torch, and the derived
tolerance."""
import math
import os
import sys

import torch

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLD_DIR not in sys.path:
    sys.path.insert(0, GOLD_DIR)
from make_spatial_golden import BOX_CASES, CASES, MEAN, STD, boxes, clip, normalised  # noqa: E402,F401


def golden():
    return torch.load(os.path.join(GOLD_DIR, "spatial_transforms.pt"), weights_only=False)


def affine(mean=MEAN, std=STD, k=255.0):
    """(ch_scale, ch_shift) of Div255 + Normalize, as DevicePacker builds them."""
    m, s = torch.tensor(mean, dtype=torch.float64), torch.tensor(std, dtype=torch.float64)
    return (1.0 / (k * s)).float(), (-m / s).float()


def ulp32(v):
    """Spacing of fp32 numbers just below 2^ceil(log2 v): one rounding of a source coordinate < v."""
    return 2.0 ** (math.floor(math.log2(v)) - 23)


def bound(ref, hs, ws, max_scale, bf16=False):
    """Elementwise tolerance.  A source coordinate below 2^k carries at most one ulp of error per operation, which moves
    an interpolation weight by as much; a tap difference is at most 255 (times the affine scale).  Plus four roundings of
    the blend itself, and one more to bf16 where the destination is bf16."""
    ref = ref.float()
    tol = 2 * ulp32(max(hs, ws)) * 255.0 * max_scale + 4 * 2.0 ** -23 * torch.clamp(ref.abs(), min=1.0)
    return tol + 2.0 ** -8 * ref.abs() if bf16 else tol


def _axis(n_in, n_out, off, n):
    """i0, i1, l0, l1 of the pinned formula for destination indices off .. off+n-1, every operation in fp32."""
    s = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    d = torch.arange(off, off + n, dtype=torch.float32)
    r = torch.clamp(s * (d + 0.5) - 0.5, min=0.0)
    i0 = r.to(torch.int64)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = r - i0.to(torch.float32)
    return i0, i1, 1.0 - l1, l1


def pinned_resample(x, hn, wn, y_off, x_off, ho, wo, scale=None, shift=None):
    """The header's formula on a (..., C, T, Hs, Ws) tensor of raw values: interpolate the taps in fp32, then the affine map."""
    x = x.float()
    hs, ws = x.shape[-2:]
    i0y, i1y, l0y, l1y = _axis(hs, hn, y_off, ho)
    i0x, i1x, l0x, l1x = _axis(ws, wn, x_off, wo)
    top, bot = x[..., i0y, :], x[..., i1y, :]
    l0y, l1y = l0y.view(-1, 1), l1y.view(-1, 1)
    v = l0y * (l0x * top[..., i0x] + l1x * top[..., i1x]) + l1y * (l0x * bot[..., i0x] + l1x * bot[..., i1x])
    if scale is not None:
        shape = [1] * v.dim()
        shape[-4] = -1
        v = v * scale.view(shape) + shift.view(shape)
    return v


def check(got, ref, hs, ws, max_scale, bf16=False, what=""):
    """Assert |got - ref| <= bound everywhere (no element excluded); print and return the worst deviation."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    tol = bound(ref, hs, ws, max_scale, bf16)
    worst = err.max().item()
    print("%s: worst |d| %.3e, bound at that scale %.3e, |ref| max %.3f" % (what, worst, tol.min().item(), ref.abs().max().item()))
    assert bool((err <= tol).all()), "%s: %d elements over the bound, worst %.3e" % (what, int((err > tol).sum()), worst)
    return worst
