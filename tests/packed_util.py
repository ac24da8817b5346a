"""Helpers of the packed-pixel tests (tests/test_packed_views.py, tests/test_gpu_packed_views.py): packed frames as strided
views into a larger random buffer, and one raw launcher for the four entry points that honour the packed layouts
(include/pv_mi355x.h, "packed pixels") -- whole videos or frame lists, any destination form, oriented records, rectangles, the
box filter -- which serves the packed launch and its reference, the `PV_SRC_NTHWC` launch of the dense R, G, B copy, alike."""
import ctypes as C

import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

LAYOUTS = TR.PACKED_LAYOUTS
# the five destination forms of the ingest (RS_DISPATCH, pytorchvideo_amd/csrc/pv_rs.h)
FORMS = [("planar", torch.bfloat16), ("planar", torch.float32), ("c4", torch.bfloat16), ("cl8_ld16", torch.bfloat16),
         ("cl8", torch.float32)]
FORM_IDS = ["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS]
MEAN, STD = (0.45, 0.40, 0.35), (0.225, 0.25, 0.275)             # per channel, all different: a swapped channel shows


def layout_bytes(layout):
    return 3 if layout == "BGR" else 4


def strides_of(layout, n, h, w):
    """(start, pitch, frame stride, buffer bytes) of the tests' packed surface: it starts one pixel into the buffer -- BGR two
    more bytes, so that `addr & 15` of the first frame is odd (5) --, its rows have a pitch of W * PB + 12 (PB == 4) or
    W * 3 + 7 (BGR: odd, so the rows alternate between odd and even addresses), and its frames lie a few bytes apart."""
    pb = layout_bytes(layout)
    pitch = w * pb + (12 if pb == 4 else 7)
    frame = h * pitch + (20 if pb == 4 else 5)
    start = pb + (0 if pb == 4 else 2)
    return start, pitch, frame, start + n * frame + 64


def surface(layout, n, h, w, seed, device="cpu"):
    """(buffer, view): a random uint8 buffer and the [n, h, w, PB] view of `strides_of` into it.  Every byte is random: the
    alpha channel, the row padding and the gaps between frames too."""
    pb = layout_bytes(layout)
    start, pitch, frame, size = strides_of(layout, n, h, w)
    buf = torch.randint(0, 256, (size,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(device)
    return buf, view_of(buf, layout, n, h, w)


def view_of(buf, layout, n, h, w):
    start, pitch, frame, _ = strides_of(layout, n, h, w)
    return buf.as_strided((n, h, w, layout_bytes(layout)), (frame, pitch, layout_bytes(layout), 1), start)


def scrambled(buf, layout, n, h, w, seed):
    """A buffer with the same R, G and B bytes in the surface's pixels and OTHER values everywhere else: alpha, row padding,
    the bytes around and between the frames."""
    other = (buf + torch.randint(1, 256, buf.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(buf.device))
    rgb = list(TR._PACKED_RGB[layout])
    view_of(other, layout, n, h, w)[..., rgb] = view_of(buf, layout, n, h, w)[..., rgb]
    return other


def affine(device):
    mean, std = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    return (1.0 / (255.0 * std)).float().to(device), (-mean / std).float().to(device)


def _f32(a, b):
    return C.c_float(a / b).value


def _upload(ctypes_array):
    return torch.frombuffer(ctypes_array, dtype=torch.uint8).cuda()


def bits(x):
    """The raw bits: NaN sentinels compare equal to themselves."""
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def destination(form, dtype, n, t, ho, wo):
    """A NaN-filled destination of n items, and (c_p, ld) for the channels-last forms."""
    if form == "planar":
        return torch.full((n, 3, t, ho, wo), float("nan"), dtype=dtype, device="cuda"), None
    c_p, ld = {"c4": (4, 4), "cl8": (8, 8), "cl8_ld16": (8, 16)}[form]
    return torch.full((n, t, ho, wo, ld), float("nan"), dtype=dtype, device="cuda"), (c_p, ld)


def footprint(dst, cl, n_written):
    """(inside, outside): the elements the launch of `n_written` items must have written, and all the others."""
    inside = torch.zeros(dst.shape, dtype=torch.bool, device=dst.device)
    if cl is None:
        inside[:n_written] = True
    else:
        inside[:n_written, ..., :cl[0]] = True
    return inside, ~inside


def launch(layout, videos, table, triples, form, dtype, short=None, crop=None, idxs=(1,), frames=False, orients=None,
           regions=None, window=None, area=False, extra=1):
    """One launch of pv_batch_views / pv_frame_views (`frames`) / pv_region_views (`regions`) / pv_area_views (`area`).
    `layout`: "NTHWC" (dense [N,H,W,3] device tensors) or a packed layout (device views [N,H,W,PB] with any legal strides,
    which become y_pitch / frame_stride).  `table`: int32 [rows, T]; `triples`: the items (source, row, view).  `crop`: the side
    of the square crop of `short`-side-scaled frames, views `idxs`; `window` = (Ho, Wo): no crop, the whole scaled frame (or,
    with `regions` -- int [rows, T, 4] -- the size every rectangle is resized to).  Returns (dst, cl) with `extra` unwritten
    items behind the launch's."""
    from gpu_util import call
    packed = layout != "NTHWC"
    pb = layout_bytes(layout) if packed else 3
    orients = orients or [0] * len(videos)
    ho, wo = window if window is not None else (crop, crop)
    sources = (L.ViewSource * len(videos))()
    keep, ptrs = [], []
    for rec, v, orient in zip(sources, videos, orients):
        n, hs, ws, c = v.shape
        assert c == pb and v.is_cuda and v.dtype == torch.uint8 and (packed or v.is_contiguous())
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
        if packed:
            # whole videos: the bytes between frames; frame lists: the extent of one frame
            rec.y_pitch, rec.frame_stride = v.stride(1), (v.stride(0) if not frames else (hs - 1) * v.stride(1) + ws * pb)
        if frames:
            rec.src = 8 * len(ptrs)                              # the slice's offset; the table's address is added below
            ptrs.extend(v[i].data_ptr() for i in range(n))
        else:
            rec.src = v.data_ptr()
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
    scale, shift = affine("cuda")
    keep += [_upload(sources), _upload(items), tab, scale, shift]
    d.sources, d.sources_dev = C.addressof(sources), keep[-5].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[-4].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], tab.shape[1], 3, tab.shape[1]
    d.src_dtype, d.src_layout = L.PV_U8, (getattr(L, "SRC_" + layout) if packed else L.SRC_NTHWC)
    d.Ho, d.Wo, d.n_views = ho, wo, (1 if regions is not None else len(idxs))
    d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    if regions is not None:
        rec_host = TR.region_records(torch.as_tensor(regions), (ho, wo))
        rec_dev = rec_host.cuda()
        keep += [rec_host, rec_dev]
        outer.regions, outer.regions_dev = rec_host.data_ptr(), rec_dev.data_ptr()
    dst, cl = destination(form, dtype, len(triples) + extra, tab.shape[1], ho, wo)
    d.dst, d.dst_dtype = dst.data_ptr(), (L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], tab.shape[1] * ho * wo * cl[1]
    entry = "pv_area_views" if area else "pv_region_views" if regions is not None else "pv_frame_views" if frames else "pv_batch_views"
    call(entry, d if outer is None else outer)
    return dst, cl


def dense_rgb(view, layout):
    """The reference's source: the dense [N,H,W,3] R, G, B copy of packed frames."""
    return TR.packed_to_rgb(view, layout).contiguous()
