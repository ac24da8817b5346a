"""Helpers of the packed YUV 4:2:2 tests (tests/test_yuyv_views.py, tests/test_gpu_yuyv_views.py): macropixel frames built
from planes as strided views into a larger random buffer -- one sample into the buffer (an odd address for 8-bit samples, an
address that is 2 mod 4 for 16-bit samples), a pitch that exceeds the row and is no multiple of 16 bytes -- in the form
tests/yuv4_util.py's launcher takes, so that ONE launcher serves the new launches (PV_SRC_YUYV422, c_step 4) and their
reference, the PV_SRC_YUV422 launch on the de-interleaved planes (include/pv_mi355x.h, "packed YUV 4:2:2")."""
import torch

import yuv4_util as Y4

PACKED = (0, 1, "packed")                                        # the `sub` of a Packed surface: 4:2:2's shifts, one plane
Y4.CODE[PACKED] = 13                                             # PV_SRC_YUYV422, for Y4.launch
# sample order -> the samples of (U, V) inside a macropixel; VYUY has no layout string
ORDERS = {"YUY2": (1, 3), "YVYU": (3, 1), "UYVY": (0, 2), "VYUY": (2, 0)}
# layout string -> (order, sample bytes, bit depth, MSB-aligned)
LAYOUT = {"YUY2": ("YUY2", 1, 8, False), "YVYU": ("YVYU", 1, 8, False), "UYVY": ("UYVY", 1, 8, False),
          "Y210": ("YUY2", 2, 10, True), "Y212": ("YUY2", 2, 12, True), "Y216": ("YUY2", 2, 16, True)}


def planes(n, h, w, seed, sb=1, bits=8, msb=False):
    """Unrelated random Y [n,h,w] and U, V [n,h,w/2] planes (Y4.planes of 4:2:2)."""
    return Y4.planes(n, h, w, Y4.SUB422, seed, sb, bits, msb)


def _pitch(w, sb):
    """A row pitch in elements, above the 2 w samples of a row, whose bytes are no multiple of 16."""
    p = 2 * w + 3
    while (p * sb) % 16 == 0:
        p += 1
    return p


class Packed:
    """Packed 4:2:2 frames built from planes: rows of w / 2 macropixels with U and V at samples `order` and luma at the other
    two, inside a random buffer.  `view` is the [n, h, w, 2] tensor a user would hand over; `geom` the record fields in BYTES,
    with the members Y4.launch reads (sub, c_step, sb, buf)."""

    def __init__(self, y, u, v, order="YUY2", sb=1, seed=0, device="cpu"):
        n, h, w = y.shape
        us, vs = ORDERS[order]
        p = _pitch(w, sb)
        frame, start = h * p + 5, 1                              # elements: frames a few samples apart, one sample into the buffer
        size = start + n * frame + 64
        g = torch.Generator().manual_seed(seed)
        buf8 = torch.randint(0, 256, (size * sb,), dtype=torch.uint8, generator=g)
        buf = buf8 if sb == 1 else buf8.view(torch.int16)

        def put(plane, step, at):
            val = plane if sb == 1 else torch.where(plane >= 32768, plane - 65536, plane)
            buf.as_strided(tuple(plane.shape), (frame, p, step), start + at).copy_(val.to(buf.dtype))

        y0 = 0 if us & 1 else 1                                  # luma: the two samples chroma leaves
        put(y, 2, y0)
        put(u, 4, us)
        put(v, 4, vs)
        self.buf = buf.to(device)
        self.view = self.buf.as_strided((n, h, w, 2), (frame, p, 2, 1), start)
        self.sub, self.c_step, self.sb, self.order = PACKED, 4, sb, order
        self.geom = dict(N=n, Hs=h, Ws=w, Hc=h, frame_stride=frame * sb, y_pitch=p * sb, c_pitch=0, c_step=4,
                         u_offset=us * sb, v_offset=vs * sb)
        addr = self.view.data_ptr()
        assert addr % (2 * sb) == sb and (p * sb) % 16 and p > 2 * w


def packed_of(layout, y, u, v, seed=0, device="cpu"):
    order, sb, _, _ = LAYOUT[layout]
    return Packed(y, u, v, order, sb, seed, device)


def planar_of(y, u, v, sb=1, seed=0, device="cpu"):
    """The de-interleaved planes as a PV_SRC_YUV422, c_step 1 surface: the reference of every packed launch."""
    return Y4.Surface(y, u, v, Y4.SUB422, 1, False, sb, seed, device)
