"""`pv_yuv16_views` and the `PV_U16` sources of `pv_batch_views` / `pv_frame_views` on the MI355X: the ingest reading 10- to
16-bit YUV 4:2:0 (P010 / P012 / P016, I010 / I012 / I016) itself, and the `src_layout="P010"` ... paths of
`device_scale_crop`, `DevicePacker`, `FrameList` and the predictors.

Two references.  Bit for bit: scaling a code by 256 and a coefficient by 2^-8 is exact in fp32, so a P016 / I016 surface
holding `sample << 8` with the MSB-aligned matrix must give the very bits `pv_yuv_views` gives for the NV12 / I420 surface.
Within a bound: `transforms.yuv420_to_rgb` -- the host mirror, conversion in fp64 with the fp32 matrix the device holds --
followed by `spatial_util.pinned_resample`, held to the bound of tests/test_gpu_yuv_ingest.py,
`spatial_util.bound(...) + 4 * 2^-14 * max_scale`.  That derivation needs every product and partial sum of a tap's three
multiply-adds below 1024 in magnitude; `yuv16_util.magnitudes_below_1024` asserts it for every matrix used here.

The helpers are those of tests/test_gpu_yuv_ingest.py, test_gpu_batch_views.py and test_gpu_frame_views.py."""
from fractions import Fraction

import pytest
import torch

import spatial_util as SU
import test_gpu_batch_views as BV
import test_gpu_yuv_ingest as G8
import yuv16_util as Y16
import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import StreamPredictor, VideoBatchPredictor, VideoPredictor

pytestmark = pytest.mark.gpu
SENTINEL, MAX_SCALE, FORMS, TABLE, KW = G8.SENTINEL, G8.MAX_SCALE, G8.FORMS, G8.TABLE, G8.KW
IDS = ["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS]
TWO_FORMS = (("planar", torch.float32), ("c4", torch.bfloat16))
M601 = TR.yuv_matrix("bt601", False)
M601_MSB = TR.yuv_matrix("bt601", False, 16, True)             # == the 8-bit matrix, Y / U / V columns times 2^-8
M2020_10 = TR.yuv_matrix("bt2020", False, 10)                   # I010: LSB-aligned 10-bit codes
M709F_P010 = TR.yuv_matrix("bt709", True, 10, True)             # P010: 10-bit codes << 6, full range
M709_P016 = TR.yuv_matrix("bt709", False, 16, True)             # P016: all 16 bits are the sample


def test_the_matrices_keep_every_product_and_partial_sum_below_1024():
    assert Y16.magnitudes_below_1024(M2020_10, 1023.0)
    for m in (M709F_P010, M709_P016, M601_MSB):
        assert Y16.magnitudes_below_1024(m, 65535.0)
    assert not Y16.magnitudes_below_1024(M2020_10, 65535.0)      # the check does fire


# ----------------------------------------------------------------------------- kernel
def _run(frames, layout, table, size, crop, idxs, form, dtype, matrix, item0=0, n_items=0, extra=1, affine=True, **geom_kw):
    """pv_yuv16_views (pv_yuv_views for an 8-bit layout) on device frames: (sentinel-filled destination of `extra` more items
    than the window, items written)."""
    from gpu_util import call
    geom = TR.yuv_geometry(frames, layout, **geom_kw)
    tab = table.to(torch.int32).contiguous().cuda()
    m = matrix.float().reshape(12).cuda()
    d = TR._yuv_desc(frames, geom, tab, m, size, crop, idxs)
    d.item0, d.n_items = item0, n_items
    keep = [x.cuda() for x in SU.affine()] if affine else []
    if affine:
        d.ch_scale, d.ch_shift = keep[0].data_ptr(), keep[1].data_ptr()
    n = n_items if n_items else table.shape[0] * len(idxs)
    t = table.shape[1]
    dst, cl = G8._destination(form, dtype, n + extra, t, crop)
    d.dst, d.dst_dtype = dst.data_ptr(), (L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], t * crop * crop * cl[1]
    call("pv_yuv16_views" if layout in TR.YUV16_LAYOUTS else "pv_yuv_views", d)
    return dst, n


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# 1. the tie to the pinned 8-bit kernel ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tied10():
    """10 frames of 98 x 132: the 8-bit planes on the device as NV12 / I420, and the same samples << 8 as P016 / I016."""
    y, u, v = YU.planes(10, 98, 132, 1200)
    wide = [c.to(torch.int64) << 8 for c in (y, u, v)]
    return {"NV12": YU.pack(y, u, v, "NV12").frames("cuda"), "I420": YU.pack(y, u, v, "I420").frames("cuda"),
            "P016": Y16.pack(*wide, "P016").frames("cuda"), "I016": Y16.pack(*wide, "I016").frames("cuda", torch.int16)}


@pytest.mark.parametrize("form,dtype", FORMS, ids=IDS)
@pytest.mark.parametrize("wide,narrow", [("P016", "NV12"), ("I016", "I420")])
def test_yuv16_views_on_shifted_samples_writes_the_bits_of_yuv_views(tied10, wide, narrow, form, dtype):
    got, n = _run(tied10[wide], wide, TABLE, 64, 56, (0, 1, 2), form, dtype, M601_MSB, extra=2)
    want, _ = _run(tied10[narrow], narrow, TABLE, 64, 56, (0, 1, 2), form, dtype, M601, extra=2)
    assert n == 6 and torch.equal(_bits(got), _bits(want))
    assert torch.all(got[n:] == SENTINEL) and not torch.any(torch.all(got[:n].flatten(1) == SENTINEL, dim=1))


# 2. real high-depth content against the mirror ----------------------------------------------------------------------
def _reference(frames_cpu, layout, matrix, table, size, crop, idxs, affine=True, **geom_kw):
    rgb = TR.yuv420_to_rgb(frames_cpu, layout, matrix.float().double(), **geom_kw)
    return G8._resampled(rgb, table, size, crop, idxs, affine)


CONTENT = {"I010_bt2020_limited": ("I010", M2020_10, dict(lo=0, hi=1024, shift=0)),
           "P010_bt709_full": ("P010", M709F_P010, dict(lo=0, hi=1024, shift=6)),
           "P016_full_codes": ("P016", M709_P016, dict(lo=0, hi=65536, shift=0))}


@pytest.fixture(scope="module")
def content10():
    cache = {}

    def case(name):
        if name not in cache:
            layout, m, kw = CONTENT[name]
            y, u, v = Y16.planes(10, 98, 132, 2200, **kw)
            if name == "P016_full_codes":
                assert 0.45 < float((y >= 32768).double().mean()) < 0.55
            packed = Y16.pack(y, u, v, layout)
            cache[name] = (packed.frames("cuda"), layout, m, _reference(packed.frames(), layout, m, TABLE, 64, 56, (0, 1, 2)))
        return cache[name]
    return case


@pytest.mark.parametrize("name,form,dtype", [("P016_full_codes", f, t) for f, t in FORMS]
                         + [(n, f, t) for n in ("I010_bt2020_limited", "P010_bt709_full") for f, t in (FORMS[4], FORMS[0])])
def test_yuv16_views_high_depth_content_against_the_mirror(content10, name, form, dtype):
    frames, layout, m, want = content10(name)
    dst, n = _run(frames, layout, TABLE, 64, 56, (0, 1, 2), form, dtype, m, extra=2)
    assert n == 6
    G8._check(G8._planar_of(dst, form, n), want, 98, 132, MAX_SCALE, dtype == torch.bfloat16, "%s %s %s" % (name, form, dtype))


# 3. alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,pitch", [("P010", 25), ("I010", 26)], ids=["P010_pitch25", "I010_pitch26"])
def test_yuv16_views_two_byte_alignment_pitch_coded_height_and_upscaling(layout, pitch):
    """30 x 22 frames with a row pitch of W + 3 samples (I010: W + 4), coded height 32, the base one sample into the buffer,
    scaled up to 41 and cropped to 37 (dense staging): rows are only 2-byte aligned.  Whatever lies in the padding, in the
    undisplayed rows and in their chroma must not matter."""
    y, u, v = Y16.planes(4, 30, 22, 2201, shift=6 if layout == "P010" else 0)
    m = M709F_P010 if layout == "P010" else M2020_10
    table = torch.tensor([[0, 1, 2, 3], [3, 3, 0, 2]], dtype=torch.int32)
    outs = []
    for garbage in (31, 32):
        packed = Y16.pack(y, u, v, layout, coded_height=32, pitch=pitch, base=1, garbage=garbage)
        frames = packed.frames("cuda")
        assert frames.data_ptr() % 4 == 2 and frames.stride() == (48 * pitch, pitch, 1)
        for form, dtype in TWO_FORMS:
            dst, n = _run(frames, layout, table, 41, 37, (0, 1, 2), form, dtype, m, height=30, coded_height=32)
            outs.append(dst)
            if garbage == 31:
                want = _reference(packed.frames(), layout, m, table, 41, 37, (0, 1, 2), height=30, coded_height=32)
                G8._check(G8._planar_of(dst, form, n), want, 30, 22, MAX_SCALE, dtype == torch.bfloat16, "%s pitch %d %s" % (layout, pitch, form))
    assert torch.equal(outs[0], outs[2]) and torch.equal(_bits(outs[1]), _bits(outs[3]))


# 4. sparse staging --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["P010", "I010"])
def test_yuv16_views_sparse_staging(layout):
    """256 x 340 -> 64 / 56: every output row stages its own two luma rows and their chroma rows."""
    y, u, v = Y16.planes(3, 256, 340, 2202, shift=6 if layout == "P010" else 0)
    m = M709F_P010 if layout == "P010" else M2020_10
    table = torch.tensor([[2, 0], [1, 1]], dtype=torch.int32)
    packed = Y16.pack(y, u, v, layout)
    want = _reference(packed.frames(), layout, m, table, 64, 56, (0, 1, 2))
    for form, dtype in (("planar", torch.bfloat16), ("cl8", torch.float32)):
        dst, n = _run(packed.frames("cuda"), layout, table, 64, 56, (0, 1, 2), form, dtype, m)
        G8._check(G8._planar_of(dst, form, n), want, 256, 340, MAX_SCALE, dtype == torch.bfloat16, "%s sparse %s" % (layout, form))


# 5. short strips ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws,per_row,rows", [(1200, 9664, 3), (4000, 32064, 1)], ids=["1200_R3", "4000_R1"])
def test_yuv16_views_short_strips_of_wide_frames(ws, per_row, rows):
    """A 16 x ws P010 frame -> 8 x ws/2, the whole scaled frame as one rectangular window, through the C ABI.  The byte span
    of the window makes the two staged source rows of an output row `per_row` LDS bytes, so a workgroup of the 32 KiB budget
    holds `rows` output rows (8 rows: strips of 3 + 3 + 2, or eight of 1) -- still under the 64 KiB limit."""
    from gpu_util import call
    pitch = -(-(2 * ws + 15) // 16) * 16
    assert 2 * 2 * pitch == per_row and (32 * 1024) // per_row == rows
    y, u, v = Y16.planes(2, 16, ws, 2203, shift=6)
    packed = Y16.pack(y, u, v, "P010")
    frames = packed.frames("cuda")
    geom = TR.yuv_geometry(frames, "P010")
    table = torch.tensor([[1, 0]], dtype=torch.int32)
    tab, m = table.cuda(), M709F_P010.float().reshape(12).cuda()
    scale, shift = [x.cuda() for x in SU.affine()]
    d = L.YuvViewsDesc()
    d.src, d.t_index, d.yuv2rgb, d.ch_scale, d.ch_shift = frames.data_ptr(), tab.data_ptr(), m.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.n_clips, d.T, d.N, d.t_stride, d.Hs, d.Ws = 1, 2, 2, 2, 16, ws
    for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch", "c_step"):
        setattr(d, k, geom[k])
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = 8, ws // 2, 8, ws // 2, 1
    dst = torch.full((2, 3, 2, 8, ws // 2), SENTINEL, dtype=torch.float32, device="cuda")
    d.dst, d.dst_layout, d.dst_dtype = dst.data_ptr(), L.DST_NCTHW, L.PV_F32
    call("pv_yuv16_views", d)
    assert torch.all(dst[1:] == SENTINEL)
    rgb = TR.yuv420_to_rgb(packed.frames(), "P010", M709F_P010.float().double())
    clips = rgb[table.long()].permute(0, 2, 1, 3, 4)
    want = SU.pinned_resample(clips, 8, ws // 2, 0, 0, 8, ws // 2, *SU.affine())
    G8._check(dst[:1], want, 16, ws, MAX_SCALE, False, "P010 16 x %d" % ws)


# 6. item windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dtype", TWO_FORMS, ids=["planar_f32", "c4_bf16"])
def test_yuv16_views_item_ranges(form, dtype):
    """2 clips x 3 views: every window writes only its range and equals the whole launch, bit for bit."""
    frames = Y16.pack(*Y16.planes(6, 50, 68, 2204, shift=6), "P010").frames("cuda")
    table = torch.tensor([[0, 2, 4], [5, 3, 1]], dtype=torch.int32)
    args = (frames, "P010", table, 32, 28, (0, 1, 2), form, dtype, M709F_P010)
    whole, n = _run(*args, 0, 6)
    assert n == 6 and torch.all(whole[6:] == SENTINEL) and not torch.any(torch.all(whole[:6].flatten(1) == SENTINEL, dim=1))
    implied, _ = _run(*args, 0, 0)                               # n_items == 0: all
    assert torch.equal(_bits(implied), _bits(whole))
    for item0, cnt in ((1, 4), (5, 1)):
        part, n = _run(*args, item0, cnt, extra=2)
        assert n == cnt and torch.all(part[cnt:] == SENTINEL)
        assert torch.equal(_bits(part[:cnt]), _bits(whole[item0:item0 + cnt])), (item0, cnt)


# 7. the entry points tie to one another -----------------------------------------------------------------------------
def _alone(frames, layout, table, size, crop, idxs, form, dtype, matrix, **geom_kw):
    dst, n = _run(frames, layout, table, size, crop, idxs, form, dtype, matrix, extra=0, **geom_kw)
    return dst


def _records(sources, srcs, geoms, size, crop, idxs):
    for rec, src, g in zip(sources, srcs, geoms):
        BV._geometry(rec, src, g["N"], g["Hs"], g["Ws"], size, crop, idxs)
        for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch"):
            setattr(rec, k, g[k])


def _u16_desc(d, tab, t, crop, n_views, c_step, matrix):
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], tab.shape[1], 3, t
    d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U16, L.SRC_YUV420, c_step, matrix.data_ptr()
    d.Ho, d.Wo, d.n_views = crop, crop, n_views


@pytest.mark.parametrize("layout", ["P010", "I010"])
def test_batch_and_frame_views_u16_tie_to_yuv16_views(layout):
    """A pitched video with a coded height (its base one sample into the buffer) and a tight one of another size, items
    scrambled: `pv_batch_views` with PV_U16 equals `pv_yuv16_views` on each video alone, and `pv_frame_views` over the same
    frames as separately allocated surfaces, in pool order, equals `pv_batch_views` -- bit for bit."""
    from gpu_util import call
    shift = 6 if layout == "P010" else 0
    m = M709F_P010 if layout == "P010" else M2020_10
    packed = [Y16.pack(*Y16.planes(10, 98, 132, 2210, shift=shift), layout, coded_height=112, pitch=160, base=1, garbage=5),
              Y16.pack(*Y16.planes(7, 66, 50, 2211, shift=shift), layout)]
    kws = [dict(coded_height=112, height=98), {}]
    videos = [p.frames("cuda") for p in packed]
    geoms = [TR.yuv_geometry(v, layout, **kw) for v, kw in zip(videos, kws)]
    tables = [torch.tensor([[0, 2, 2, 9], [7, 9, 4, 5], [3, 2, 1, 0]], dtype=torch.int32),
              torch.tensor([[6, 0, 3, 3], [1, 2, 4, 6]], dtype=torch.int32)]
    matrix = m.float().reshape(12).cuda()
    every = [(s, r, v) for s in range(2) for r in range(tables[s].shape[0]) for v in range(3)]
    order = torch.randperm(len(every), generator=torch.Generator().manual_seed(5)).tolist()
    triples = [every[i] for i in order] + [every[order[0]]]
    tab, row0 = BV._concat_tables(tables, 4)
    items = BV._items([(s, row0[s] + r, v) for s, r, v in triples])
    # the same frames as surfaces of their own: int16 allocations, every surface 1 or 3 samples in, allocated out of order
    lists = []
    for j, p in enumerate(packed):
        cpu = p.frames(dtype=torch.int16)
        n, rows, w = cpu.shape
        pitch = cpu.stride(1)
        own = [None] * n
        for i in torch.randperm(n, generator=torch.Generator().manual_seed(2220 + j)).tolist():
            buf = torch.full((rows * pitch + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
            off = (1, 3)[i % 2]
            # a surface is its rows * pitch samples: the half-pitch chroma rows of the planar form lie partly behind column W
            buf[off:off + rows * pitch].copy_(torch.as_strided(cpu, (rows * pitch,), (1,), cpu[i].storage_offset()))
            own[i] = torch.as_strided(buf, (rows, w), (pitch, 1), off)
        lists.append(own)
    assert all(f.data_ptr() % 4 == 2 for own in lists for f in own)
    ptrs = torch.tensor([f.data_ptr() for own in lists for f in own], dtype=torch.int64)
    ptrs_dev = ptrs.cuda()
    for form, dtype in FORMS:
        sources = (L.ViewSource * 2)()
        _records(sources, [v.data_ptr() for v in videos], geoms, 64, 56, (0, 1, 2))
        d = L.BatchViewsDesc()
        _u16_desc(d, tab, 4, 56, 3, geoms[0]["c_step"], matrix)
        got = BV._launch_batch(d, sources, items, form, dtype, 3, 4, 56)
        alone = [_alone(v, layout, t, 64, 56, (0, 1, 2), form, dtype, m, **kw) for v, t, kw in zip(videos, tables, kws)]
        for i, (s, r, v) in enumerate(triples):
            assert BV._same_bits(got[i], alone[s][r * 3 + v]), (layout, form, dtype, i, s, r, v)
        assert torch.all(got[len(triples):] == SENTINEL) and not torch.all(got[:len(triples)] == SENTINEL)
        # pv_frame_views on the surfaces
        fsources = (L.ViewSource * 2)()
        _records(fsources, [ptrs_dev.data_ptr(), ptrs_dev.data_ptr() + 8 * len(lists[0])], geoms, 64, 56, (0, 1, 2))
        f = L.FrameViewsDesc()
        _u16_desc(f.batch, tab, 4, 56, 3, geoms[0]["c_step"], matrix)
        keep = [BV._upload(fsources), BV._upload(items)] + [x.cuda() for x in SU.affine()]
        b = f.batch
        b.sources, b.sources_dev = BV.C.addressof(fsources), keep[0].data_ptr()
        b.items, b.items_dev = BV.C.addressof(items), keep[1].data_ptr()
        b.n_sources, b.n_items = 2, len(items)
        b.ch_scale, b.ch_shift = keep[2].data_ptr(), keep[3].data_ptr()
        dst, cl = BV._destination(form, dtype, len(items) + 2, 3, 4, 56)
        BV._set_destination(b, dst, cl, dtype, 4, 56)
        f.frame_ptrs, f.frame_ptrs_dev, f.n_frame_ptrs = ptrs.data_ptr(), ptrs_dev.data_ptr(), ptrs.numel()
        call("pv_frame_views", f)
        assert BV._same_bits(dst, got), (layout, form, dtype)


# 8. predictors ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def x3d6():
    return G8._x3d(6)


def _p010_video(n, hs, ws, seed, dtype=torch.uint16, **kw):
    return Y16.pack(*Y16.planes(n, hs, ws, seed, shift=6), "P010", **kw).frames("cuda", dtype)


YUV = ("bt2020", False)


def _composed(dep, video, table, batch, short_side, crop, views, **geom):
    """The composed path: P010 clips materialised by index_select through an int16 view (uint16 has no index_select),
    `device_scale_crop(..., src_layout="P010")`, the views fed to the deploy form `batch` items at a time (the last batch
    padded with items that are never folded), `VideoEnsembler`.  (video scores, clip scores)."""
    n_clips, t = table.shape
    n_views = len(views)
    v16 = video.view(torch.int16)
    clips = v16.index_select(0, table.reshape(-1).long().to(video.device)).view(n_clips, t, *video.shape[1:])
    x = TR.device_scale_crop(clips, short_side, crop, views, num_frames=t, dtype=torch.bfloat16, src_layout="P010", yuv=YUV, **KW, **geom)
    total = n_clips * n_views
    ve = ce = None
    for i0 in range(0, total, batch):
        k = min(batch, total - i0)
        xb = torch.cat([x[i0:i0 + k], torch.full((batch - k,) + tuple(x.shape[1:]), 2.0, dtype=x.dtype, device=x.device)])
        logits = dep(xb)[:k].clone()
        if ve is None:
            ve, ce = VideoEnsembler(1, logits.shape[1], "sum"), VideoEnsembler(n_clips, logits.shape[1], "sum")
        ve.update(logits, [0] * k)
        ce.update(logits, [(i0 + i) // n_views for i in range(k)])
    return ve.result()[0].clone(), ce.result().clone()


def test_predictors_on_p010_videos(x3d6):
    """x3d_xs, batch 6 = 2 clips x 3 views.  A 40-frame 64 x 86 P010 surface (pitched, coded height 72, the base one sample
    in) at 10 fps, 5 clips of 8 frames subsampled to 4: `VideoPredictor` equals the composed path; the same video as a
    `FrameList` of its surfaces equals the one-tensor result; `VideoBatchPredictor` on it and a tight video of another size
    equals the two `VideoPredictor` results."""
    geom = dict(coded_height=72, height=64)
    video = _p010_video(40, 64, 86, 2230, coded_height=72, pitch=96, base=1, garbage=9)
    assert not video.is_contiguous() and video.dtype == torch.uint16
    sampler = D.ConstantClipsPerVideoSampler(Fraction(8, 10), 5)
    pred = VideoPredictor(x3d6, sampler, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, **KW, **geom)
    table, _ = D.clip_frame_table(sampler, 40, 10, pred.packer.clip_frames)
    scores, clip_scores = pred(video, 10, return_clip_scores=True)
    scores, clip_scores = scores.clone(), clip_scores.clone()
    want, want_clips = _composed(x3d6, video, table, 6, 176, 160, (0, 1, 2), **geom)
    assert torch.equal(scores, want), "video scores differ by %.3e" % (scores - want).abs().max().item()
    assert torch.equal(clip_scores, want_clips) and not torch.equal(clip_scores[0], clip_scores[-1])
    # the surfaces as a FrameList (views of the pitched buffer: nothing is stacked), uint16 and int16
    for dtype in (torch.uint16, torch.int16):
        frames = TR.FrameList(list(video.view(dtype).unbind(0)), src_layout="P010")
        assert torch.equal(pred(frames, 10), scores), dtype
    # many videos per forward
    other = _p010_video(17, 70, 60, 2231, dtype=torch.int16)
    single = VideoPredictor(x3d6, sampler, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, **KW)
    want_other = single(other, 10).clone()
    both = VideoBatchPredictor(x3d6, sampler, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, **KW)
    got = both([video.view(torch.int16), other], 10, height=[64, None], coded_height=[72, None])
    assert torch.equal(got[0], scores) and torch.equal(got[1], want_other) and not torch.equal(got[0], got[1])
    # a batch of materialised clips through DevicePacker.__call__
    clips = torch.as_strided(video, (2, 4) + tuple(video.shape[1:]), (4 * video.stride(0),) + tuple(video.stride()),
                             video.storage_offset() + 8 * video.stride(0))
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, **KW, **geom)
    logits = packer(clips).clone()
    views = TR.device_scale_crop(clips, 176, 160, (0, 1, 2), src_layout="P010", yuv=YUV, **KW, **geom)
    assert torch.equal(logits, x3d6(views).clone())


def test_stream_predictor_on_p010_surfaces(x3d6):
    """One push of 23 P010 surfaces (each an allocation of its own) scores the 6 windows `VideoPredictor` scores offline."""
    dur, stride, fps = Fraction(8, 10), Fraction(3, 10), 10
    video = _p010_video(23, 64, 86, 2232)
    surfaces = [f.clone() for f in video.view(torch.int16).unbind(0)]
    pred = VideoPredictor(x3d6, D.UniformClipSampler(dur, stride), short_side=176, crop_size=160, spatial_idx=(0, 1, 2),
                          src_layout="P010", yuv=YUV, **KW)
    clip_scores = pred(video, fps, return_clip_scores=True)[1].clone()
    assert tuple(clip_scores.shape) == (6, 400)
    sp = StreamPredictor(x3d6, dur, stride, fps, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="P010", yuv=YUV, **KW)
    out = sp.push(surfaces)
    assert [k for k, _, _ in out] == list(range(6))
    for k, _, s in out:
        assert torch.equal(s, clip_scores[k]), k
    assert not torch.equal(out[0][2], out[5][2])


# 9. clamp -----------------------------------------------------------------------------------------------------------
def test_yuv16_views_clamps_every_tap_before_the_blend():
    """A frame of (Y, U, V) corners at 0 and 1023, far out of gamut, equals the CLAMPED mirror -- and neither a clamp behind
    the blend nor no clamp at all would."""
    g = torch.Generator().manual_seed(2240)
    y, u, v = [torch.randint(0, 2, s, generator=g, dtype=torch.int64) * 1023 for s in ((2, 32, 44), (2, 16, 22), (2, 16, 22))]
    table = torch.tensor([[0, 1]], dtype=torch.int32)
    m10 = TR.yuv_matrix("bt601", False, 10)
    assert Y16.magnitudes_below_1024(m10, 1023.0)
    packed = Y16.pack(y, u, v, "I010")
    want = _reference(packed.frames(), "I010", m10, table, 41, 37, (1,), affine=False)
    dst, n = _run(packed.frames("cuda"), "I010", table, 41, 37, (1,), "planar", torch.float32, m10, affine=False)
    G8._check(dst[:n], want, 32, 44, 1.0, False, "I010 corners")
    assert want.min().item() >= 0.0 and want.max().item() <= 255.0
    m = m10.float().double()
    up = [c.double().repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v)]
    raw = torch.stack([m[c, 0] * y.double() + m[c, 1] * up[0] + m[c, 2] * up[1] + m[c, 3] for c in range(3)], dim=1).float()
    assert raw.min().item() < -100 and raw.max().item() > 400
    unclamped = G8._resampled(raw, table, 41, 37, (1,), affine=False)
    tol = SU.bound(want, 32, 44, 1.0) + G8.TAP
    assert bool(((unclamped - want).abs() > 100 * tol).any())
    assert bool(((torch.clamp(unclamped, 0, 255) - want).abs() > 100 * tol).any())
