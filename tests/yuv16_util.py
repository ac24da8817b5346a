"""Shared by tests/test_yuv16_ingest.py and tests/test_gpu_yuv16_ingest.py: seeded Y / U / V planes of 16-bit codes and their
packings as decoder surfaces -- P010 / P012 / P016 (NV12's arrangement) and I010 / I012 / I016 (I420's, yuv420p10le) -- with
a coded height above the display height, a row pitch above the width and a base any number of samples into the buffer.
Built independently of `transforms.yuv_geometry` (which the tests check against them), as tests/yuv_util.py is.

Codes are held as int64 here (0 .. 65535) and stored through their int16 bit pattern: this torch build has few CPU operators
for uint16, and the surfaces are handed out as uint16 or int16 views of the same bytes."""
import torch

INTERLEAVED = ("P010", "P012", "P016")
PLANAR = ("I010", "I012", "I016")


def planes(n, hs, ws, seed, lo=0, hi=1024, shift=0):
    """int64 codes in [lo, hi) << shift: Y [n, hs, ws], U and V [n, hs/2, ws/2]."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(lo, hi, s, generator=g, dtype=torch.int64) << shift
                 for s in ((n, hs, ws), (n, hs // 2, ws // 2), (n, hs // 2, ws // 2)))


def _bits(codes):
    """Codes 0 .. 65535 as the int16 with the same 16 bits."""
    assert int(codes.min()) >= 0 and int(codes.max()) <= 65535
    return torch.where(codes >= 32768, codes - 65536, codes).to(torch.int16)


class Packed:
    """A flat int16 buffer holding the frames, and the [n, Hc*3/2, W] view of it the library is given, as uint16 or int16."""

    def __init__(self, buf, shape, strides, offset):
        self.buf, self.shape, self.strides, self.offset = buf, shape, strides, offset

    def frames(self, device=None, dtype=torch.uint16):
        buf = self.buf if device is None else self.buf.to(device)
        return torch.as_strided(buf.view(dtype), self.shape, self.strides, self.offset)


def pack(y, u, v, layout, coded_height=None, pitch=None, base=0, garbage=None):
    """The planes as `layout` frames; `pitch` and `base` count SAMPLES.  Everything that is not a sample of the display frame
    -- the pitch padding, the luma rows between the display and the coded height, the chroma of those rows, the samples in
    front of `base` -- is zero, or random 16-bit patterns seeded by `garbage`."""
    n, hs, ws = y.shape
    hc = coded_height or hs
    p = pitch or ws
    rows = hc * 3 // 2
    frame = rows * p
    size = base + n * frame + 8
    if garbage is None:
        buf = torch.zeros(size, dtype=torch.int16)
    else:
        buf = _bits(torch.randint(0, 65536, (size,), generator=torch.Generator().manual_seed(garbage), dtype=torch.int64))
    torch.as_strided(buf, (n, hs, ws), (frame, p, 1), base).copy_(_bits(y))
    first = base + hc * p
    if layout in INTERLEAVED:
        torch.as_strided(buf, u.shape, (frame, p, 2), first).copy_(_bits(u))
        torch.as_strided(buf, v.shape, (frame, p, 2), first + 1).copy_(_bits(v))
    else:
        assert layout in PLANAR and p % 2 == 0, "planar chroma rows have half the luma pitch"
        torch.as_strided(buf, u.shape, (frame, p // 2, 1), first).copy_(_bits(u))
        torch.as_strided(buf, v.shape, (frame, p // 2, 1), first + (hc // 2) * (p // 2)).copy_(_bits(v))
    return Packed(buf, (n, rows, ws), (frame, p, 1), base)


def rgb_of_planes(y, u, v, matrix):
    """clamp(M . (Y, U, V, 1), 0, 255) with chroma replicated over 2 x 2, straight from the codes: fp64 [n, 3, hs, ws]."""
    up = [c.double().repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v)]
    m = matrix.double()
    out = [m[c, 0] * y.double() + m[c, 1] * up[0] + m[c, 2] * up[1] + m[c, 3] for c in range(3)]
    return torch.clamp(torch.stack(out, dim=1), 0.0, 255.0)


def magnitudes_below_1024(matrix, top=65535.0):
    """The tap bound of tests/test_gpu_yuv_ingest.py needs every product and every partial sum of a tap's three multiply-adds
    below 1024 in magnitude for any code in [0, top]: the largest each can get, per row of the matrix."""
    m = matrix.float().double()
    worst = 0.0
    for c in range(3):
        lo = hi = float(m[c, 3])
        worst = max(worst, abs(lo))
        for k in (0, 1, 2):                                  # the header's order: Y, then U, then V
            prod = float(m[c, k]) * top
            worst = max(worst, abs(prod))
            lo, hi = lo + min(prod, 0.0), hi + max(prod, 0.0)
            worst = max(worst, abs(lo), abs(hi))
    return worst < 1024.0
