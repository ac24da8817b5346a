"""Helpers of the YUV 4:2:2 / 4:4:4 tests (tests/test_yuv4_views.py, tests/test_gpu_yuv4_views.py): YUV frames of any
subsampling built from planes as strided views into a larger random buffer -- an odd base address for 8-bit samples, an even
one for 16-bit samples, a pitch that is no multiple of 16, a coded height above the display height --, and one raw launcher
for the four entry points that honour the layouts (include/pv_mi355x.h, "YUV 4:2:2 and 4:4:4"), which serves the new launches
and their reference, the unchanged PV_SRC_YUV420 launch, alike."""
import ctypes as C

import torch

import packed_util as PU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

FORMS, FORM_IDS = PU.FORMS, PU.FORM_IDS
SUB420, SUB422, SUB444 = (1, 1), (0, 1), (0, 0)
CODE = {SUB420: 2, SUB422: 10, SUB444: 11}                       # PV_SRC_YUV420 / PV_SRC_YUV422 / PV_SRC_YUV444


def planes(n, h, w, sub, seed, sb=1, bits=8, msb=False):
    """Unrelated random Y [n,h,w] and U, V [n, ceil(h / 2^csy), ceil(w / 2^csx)] planes as int64 codes: 8-bit, or `bits`-bit
    values -- in the HIGH bits of a 16-bit code with `msb` -- for two-byte samples."""
    g = torch.Generator().manual_seed(seed)
    top = 256 if sb == 1 else 1 << bits
    hc, wc = (h + sub[0]) >> sub[0], (w + sub[1]) >> sub[1]
    out = [torch.randint(0, top, s, generator=g, dtype=torch.int64) for s in ((n, h, w), (n, hc, wc), (n, hc, wc))]
    return [p << (16 - bits) for p in out] if (sb == 2 and msb) else out


def replicated(y, u, v, sub_from, sub_to):
    """The planes of the frames whose chroma `sub_to` holds replicated: every chroma sample of `sub_from` over the luma pixels
    it covers, cut to the luma size."""
    ry, rx = 1 << (sub_from[0] - sub_to[0]), 1 << (sub_from[1] - sub_to[1])
    hc, wc = (y.shape[1] + sub_to[0]) >> sub_to[0], (y.shape[2] + sub_to[1]) >> sub_to[1]
    return [y] + [c.repeat_interleave(ry, 1).repeat_interleave(rx, 2)[:, :hc, :wc].contiguous() for c in (u, v)]


def _pitch(w, sb, halved):
    """A row pitch in elements, at least w + 3, even, whose bytes -- and, `halved`, the bytes of half of it -- are no multiple
    of 16."""
    p = w + 3 + (w + 3) % 2
    while (p * sb) % 16 == 0 or (halved and ((p // 2) * sb) % 16 == 0):
        p += 2
    return p


class Surface:
    """YUV frames built from planes in the arrangement `yuv_geometry` reads -- Hc luma rows of pitch P, then the chroma:
    interleaved rows of pitch P (4:4:4: 2 P), or two planes of pitch P >> csx -- inside a random buffer.  `view` is the
    [n, rows, w] tensor a user would hand over (NV24: [n, 3 Hc, w], which no string names); `geom` the record fields in BYTES
    plus sub, c_step, sb."""

    def __init__(self, y, u, v, sub, c_step=1, v_first=False, sb=1, seed=0, device="cpu", extra_rows=None):
        n, h, w = y.shape
        csy, csx = sub
        hc = h + (extra_rows if extra_rows is not None else (2 if csy else 3))   # the coded height
        inter = c_step == 2
        p = _pitch(w, sb, (not inter) and csx == 1)
        c_pitch = (p * (2 if csx == 0 else 1)) if inter else (p >> csx)
        hcc = hc >> csy
        rows_elems = hc * p + hcc * c_pitch * (1 if inter else 2)
        assert rows_elems % p == 0
        rows = rows_elems // p
        frame, start = rows_elems + 6, 1                         # elements: frames a few samples apart, one sample into the buffer
        size = start + n * frame + 64
        g = torch.Generator().manual_seed(seed)
        buf8 = torch.randint(0, 256, (size * sb,), dtype=torch.uint8, generator=g)
        buf = buf8 if sb == 1 else buf8.view(torch.int16)
        first = hc * p
        if inter:
            a, b = (first + 1, first) if v_first else (first, first + 1)
        else:
            second = first + hcc * c_pitch
            a, b = (second, first) if v_first else (first, second)

        def put(plane, pitch, step, at):
            val = plane if sb == 1 else torch.where(plane >= 32768, plane - 65536, plane)
            buf.as_strided(tuple(plane.shape), (frame, pitch, step), start + at).copy_(val.to(buf.dtype))

        put(y, p, 1, 0)
        put(u, c_pitch, c_step, a)
        put(v, c_pitch, c_step, b)
        self.buf = buf.to(device)
        self.view = self.buf.as_strided((n, rows, w), (frame, p, 1), start)
        self.sub, self.c_step, self.sb, self.hc = sub, c_step, sb, hc
        self.geom = dict(N=n, Hs=h, Ws=w, Hc=hc, frame_stride=frame * sb, y_pitch=p * sb, c_pitch=c_pitch * sb, c_step=c_step,
                         u_offset=a * sb, v_offset=b * sb)
        addr = self.view.data_ptr()
        assert addr % 2 == (1 if sb == 1 else 0) and (p * sb) % 16 and hc > h


# layout string -> (sub, c_step, V first, sample bytes, bit depth, MSB-aligned)
LAYOUT = {"I420": (SUB420, 1, False, 1, 8, False), "NV12": (SUB420, 2, False, 1, 8, False),
          "I010": (SUB420, 1, False, 2, 10, False), "P010": (SUB420, 2, False, 2, 10, True),
          "I422": (SUB422, 1, False, 1, 8, False), "YV16": (SUB422, 1, True, 1, 8, False),
          "NV16": (SUB422, 2, False, 1, 8, False), "NV61": (SUB422, 2, True, 1, 8, False),
          "P210": (SUB422, 2, False, 2, 10, True), "P212": (SUB422, 2, False, 2, 12, True), "P216": (SUB422, 2, False, 2, 16, True),
          "I210": (SUB422, 1, False, 2, 10, False), "I212": (SUB422, 1, False, 2, 12, False), "I216": (SUB422, 1, False, 2, 16, False),
          "I444": (SUB444, 1, False, 1, 8, False), "YV24": (SUB444, 1, True, 1, 8, False),
          "I410": (SUB444, 1, False, 2, 10, False), "I412": (SUB444, 1, False, 2, 12, False), "I416": (SUB444, 1, False, 2, 16, False)}


def surface_of(layout, y, u, v, seed=0, device="cpu"):
    sub, c_step, v_first, sb, _, _ = LAYOUT[layout]
    return Surface(y, u, v, sub, c_step, v_first, sb, seed, device)


def _f32(a, b):
    return C.c_float(a / b).value


def launch(surfaces, table, triples, form, dtype, matrix, short=None, crop=None, idxs=(1,), frames=False, orients=None,
           regions=None, window=None, area=False, extra=1, affine=True):
    """One launch of pv_batch_views / pv_frame_views (`frames`) / pv_region_views (`regions`) / pv_area_views (`area`) over
    `surfaces` (device `Surface`s of one subsampling, chroma arrangement and sample width), as packed_util.launch launches
    packed frames.  `matrix`: 3 x 4.  Returns (dst, cl) with `extra` unwritten items behind the launch's."""
    from gpu_util import call
    s0 = surfaces[0]
    assert all((s.sub, s.c_step, s.sb) == (s0.sub, s0.c_step, s0.sb) and s.buf.is_cuda for s in surfaces)
    orients = orients or [0] * len(surfaces)
    ho, wo = window if window is not None else (crop, crop)
    sources = (L.ViewSource * len(surfaces))()
    keep, ptrs = [], []
    for rec, s, orient in zip(sources, surfaces, orients):
        g = s.geom
        n, hs, ws = g["N"], g["Hs"], g["Ws"]
        hd, wd = (ws, hs) if orient & 1 else (hs, ws)
        if regions is not None:
            hn, wn, offs = ho, wo, [(0, 0)]
        elif window is not None:
            hn, wn = TR.scaled_size(hd, wd, short)
            assert (hn, wn) == (ho, wo)
            offs = [(0, 0)] * len(idxs)
        else:
            hn, wn = TR.scaled_size(hd, wd, short)
            offs = [TR.crop_offsets(hn, wn, crop, i) for i in idxs]
        rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn, rec.orient = n, hs, ws, hn, wn, orient
        rec.sy, rec.sx = _f32(hd, hn), _f32(wd, wn)
        for k, (y, x) in enumerate(offs):
            rec.y_off[k], rec.x_off[k] = y, x
        for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch"):
            setattr(rec, k, g[k])
        if frames:
            rec.src = 8 * len(ptrs)                              # the slice's offset; the table's address is added below
            ptrs.extend(s.view.data_ptr() + i * g["frame_stride"] for i in range(n))
        else:
            rec.src = s.view.data_ptr()
    outer = f = None
    if area:
        outer = L.AreaViewsDesc()
        outer.filter = L.PV_FILTER_AREA
        f = outer.frames
    elif regions is not None:
        outer = L.RegionViewsDesc()
        f = outer.frames
    elif frames:
        outer = f = L.FrameViewsDesc()
    d = L.BatchViewsDesc() if f is None else f.batch
    if frames:
        table_host = torch.tensor(ptrs, dtype=torch.int64)
        table_dev = table_host.cuda()
        keep += [table_host, table_dev]
        for rec in sources:
            rec.src = table_dev.data_ptr() + (rec.src or 0)
        f.frame_ptrs, f.frame_ptrs_dev, f.n_frame_ptrs = table_host.data_ptr(), table_dev.data_ptr(), len(ptrs)
    items = (L.ViewItem * len(triples))()
    for i, (s, r, vw) in enumerate(triples):
        items[i].source, items[i].row, items[i].view = s, r, vw
    tab = table.to(torch.int32).contiguous().cuda()
    scale, shift = PU.affine("cuda")
    m = torch.as_tensor(matrix).float().reshape(12).cuda()
    keep += [PU._upload(sources), PU._upload(items), tab, scale, shift, m]
    d.sources, d.sources_dev = C.addressof(sources), keep[-6].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[-5].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], tab.shape[1], 3, tab.shape[1]
    d.src_dtype, d.src_layout = (L.PV_U16 if s0.sb == 2 else L.PV_U8), CODE[s0.sub]
    d.c_step, d.yuv2rgb = s0.c_step, m.data_ptr()
    d.Ho, d.Wo, d.n_views = ho, wo, (1 if regions is not None else len(idxs))
    if affine:
        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    if regions is not None:
        rec_host = TR.region_records(torch.as_tensor(regions), (ho, wo))
        rec_dev = rec_host.cuda()
        keep += [rec_host, rec_dev]
        outer.regions, outer.regions_dev = rec_host.data_ptr(), rec_dev.data_ptr()
    dst, cl = PU.destination(form, dtype, len(triples) + extra, tab.shape[1], ho, wo)
    d.dst, d.dst_dtype = dst.data_ptr(), (L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], tab.shape[1] * ho * wo * cl[1]
    entry = "pv_area_views" if area else "pv_region_views" if regions is not None else "pv_frame_views" if frames else "pv_batch_views"
    call(entry, d if outer is None else outer)
    torch.cuda.synchronize()
    return dst, cl
