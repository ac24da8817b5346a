"""Shared by tests/test_area_views.py and tests/test_gpu_area_views.py: the integer windows of include/pv_mi355x.h ("box-filtered
downscale") restated in torch, the float64 reference built on them, and the derived tolerance."""
import torch

from pytorchvideo_amd import transforms as TR

# Hs x Ws -> short side, crop (None: no crop, the window is the whole scaled frame or the named one), what it exercises
GEOMETRIES = {
    "45x70_to_16": (45, 70, 16, 16),          # windows of 2-3, neighbours overlapping; three 16 x 16 views
    "64x96_to_16": (64, 96, 16, 16),          # integer ratio 4, no overlap
    "135x240_to_16": (135, 240, 16, 16),      # ratio 8.4375, windows of 9 x 10 = up to 100 taps
    "20x30_to_32": (20, 30, 32, 32),          # upscaling, windows of 1-2, repeated rows
    "33x57_to_33": (33, 57, 33, 33),          # identity
    "37x61_to_12": (37, 61, 12, 12),          # odd width, unaligned rows
    "96x1500_to_32": (96, 1500, 32, None),    # no crop: several strips, at least two column tiles
}


def windows(n_in, n_out, off, n):
    """(start, end) of the header's formula for destination indices off .. off + n - 1 of the scaled axis, int64 [n] each."""
    d = torch.arange(off, off + n, dtype=torch.int64)
    start = (d * n_in) // n_out
    end = ((d + 1) * n_in + n_out - 1) // n_out
    assert bool((end > start).all()) and int(start.min()) >= 0 and int(end.max()) <= n_in
    return start, end


def _membership(n_in, start, end):
    """float64 [n, n_in]: 1 where source index k lies in [start, end) of output i."""
    k = torch.arange(n_in, dtype=torch.int64)[None]
    return ((k >= start[:, None]) & (k < end[:, None])).double()


def reference(x, hn, wn, y_off, x_off, ho, wo, scale=None, shift=None):
    """The box mean of the raw taps `x` (..., C, T, Hs, Ws) over the header's windows, in float64, then the affine map:
    (..., C, T, ho, wo) float64, and the largest tap count of a window.  Sums of integers below 2^53 are exact in float64."""
    x = x.double()
    hs, ws = x.shape[-2:]
    sy, ey = windows(hs, hn, y_off, ho)
    sx, ex = windows(ws, wn, x_off, wo)
    total = _membership(hs, sy, ey) @ x @ _membership(ws, sx, ex).T
    count = ((ey - sy)[:, None] * (ex - sx)[None]).double()
    v = total / count
    if scale is not None:
        shape = [1] * v.dim()
        shape[-4] = -1
        v = v * scale.double().view(shape) + shift.double().view(shape)
    return v, int(count.max())


def tolerance(ref, n, max_scale, exact_sums, bf16=False):
    """Elementwise bound on |got - ref|, derived, not tuned.  With n the largest window count of the case: the recursive fp32
    sum of n values <= 255 is off by at most (n - 1) 2^-24 of its magnitude, which survives the division as an error of the
    mean; the division, the fma of the affine map and the three fmas of a YUV tap add one rounding each, of values <= 255
    (times the affine scale): (n + 4) 2^-24 255 max|ch_scale|.  uint8 RGB / planar sums are exact integers (`exact_sums`):
    that term is dropped.  Plus four roundings at the magnitude of the result, and one more to bf16 for a bf16 destination."""
    ref = ref.double()
    tol = 4 * 2.0 ** -23 * torch.clamp(ref.abs(), min=1.0)
    if not exact_sums:
        tol = tol + (n + 4) * 2.0 ** -24 * 255.0 * max_scale
    return tol + 2.0 ** -8 * ref.abs() if bf16 else tol


def check(got, ref, n, max_scale, exact_sums, bf16=False, what=""):
    """Assert |got - ref| <= tolerance everywhere (no element excluded); print and return the worst deviation."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    err = (got - ref).abs()
    tol = tolerance(ref, n, max_scale, exact_sums, bf16)
    worst = err.max().item()
    print("%s: worst |d| %.3e, smallest bound %.3e, n %d, |ref| max %.3f" % (what, worst, tol.min().item(), n, ref.abs().max().item()))
    assert bool((err <= tol).all()), "%s: %d elements over the bound, worst %.3e" % (what, int((err > tol).sum()), worst)
    return worst


def view_geometry(hs, ws, short, crop, views=(0, 1, 2)):
    """(Hn, Wn, (Ho, Wo), [(y_off, x_off) per view]) of a GEOMETRIES entry: short_side_scale + uniform_crop, or no crop."""
    hn, wn = TR.scaled_size(hs, ws, short)
    if crop is None:
        return hn, wn, (hn, wn), [(0, 0)]
    return hn, wn, (crop, crop), [TR.crop_offsets(hn, wn, crop, v) for v in views]
