"""Shared by tests/test_yuv_ingest.py and tests/test_gpu_yuv_ingest.py: seeded Y / U / V planes and their packings as
decoder surfaces -- NV12 / NV21 / I420 / YV12, with a coded height above the display height, a row pitch above the width
and a base at any byte address -- built independently of `transforms.yuv_geometry` (which the tests check against them)."""
import torch


def planes(n, hs, ws, seed):
    """uint8 Y [n, hs, ws], U and V [n, hs/2, ws/2]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, hs, ws), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (n, hs // 2, ws // 2), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (n, hs // 2, ws // 2), generator=g, dtype=torch.uint8))


class Packed:
    """A flat uint8 buffer holding the frames, and the [n, Hc*3/2, W] view of it the library is given."""

    def __init__(self, buf, shape, strides, offset):
        self.buf, self.shape, self.strides, self.offset = buf, shape, strides, offset

    def frames(self, device=None):
        buf = self.buf if device is None else self.buf.to(device)
        return torch.as_strided(buf, self.shape, self.strides, self.offset)


def pack(y, u, v, layout, coded_height=None, pitch=None, base=0, garbage=None):
    """The planes as `layout` frames.  Everything that is not a sample of the display frame -- the pitch padding, the luma
    rows between the display and the coded height, the chroma of those rows, the bytes in front of `base` -- is zero, or
    random bytes seeded by `garbage`."""
    n, hs, ws = y.shape
    hc = coded_height or hs
    p = pitch or ws
    rows = hc * 3 // 2
    frame = rows * p
    size = base + n * frame + 16
    if garbage is None:
        buf = torch.zeros(size, dtype=torch.uint8)
    else:
        buf = torch.randint(0, 256, (size,), generator=torch.Generator().manual_seed(garbage), dtype=torch.uint8)
    torch.as_strided(buf, (n, hs, ws), (frame, p, 1), base).copy_(y)
    first = base + hc * p
    if layout in ("NV12", "NV21"):
        a, b = (u, v) if layout == "NV12" else (v, u)
        torch.as_strided(buf, a.shape, (frame, p, 2), first).copy_(a)
        torch.as_strided(buf, b.shape, (frame, p, 2), first + 1).copy_(b)
    else:
        assert p % 2 == 0, "planar chroma rows have half the luma pitch"
        a, b = (u, v) if layout == "I420" else (v, u)
        torch.as_strided(buf, a.shape, (frame, p // 2, 1), first).copy_(a)
        torch.as_strided(buf, b.shape, (frame, p // 2, 1), first + (hc // 2) * (p // 2)).copy_(b)
    return Packed(buf, (n, rows, ws), (frame, p, 1), base)


def rgb_of_planes(y, u, v, matrix):
    """clamp(M . (Y, U, V, 1), 0, 255) with chroma replicated over 2 x 2, straight from the planes: fp64 [n, 3, hs, ws]."""
    up = [c.double().repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v)]
    m = matrix.double()
    out = [m[c, 0] * y.double() + m[c, 1] * up[0] + m[c, 2] * up[1] + m[c, 3] for c in range(3)]
    return torch.clamp(torch.stack(out, dim=1), 0.0, 255.0)
