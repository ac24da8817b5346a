"""Many videos per forward on the MI355X: `pv_batch_views` (one source per destination item, include/pv_mi355x.h),
`DevicePacker.video_batch` / `fill_batch` and `inference.VideoBatchPredictor`.

Reference, bit for bit (`torch.equal` on the raw bits, no tolerance): the one-source entry points the existing suite already
holds against the reference's fixtures -- `pv_video_views` / `pv_yuv_views` on every video alone
(tests/test_gpu_video_views.py, tests/test_gpu_yuv_ingest.py) -- and, for whole models, the SAME deploy form driven by
`fill_video` + `launch` on the concatenation of same-size videos.  The per-item kernels run the same instruction sequence on
the same taps, and neither the rows per workgroup nor the LDS pitch enters a value, so any difference is a bug.  No test feeds
the device a table that leaves its video."""
import ctypes as C
import os
from fractions import Fraction

import pytest
import torch

import spatial_util as SU
import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import VideoBatchPredictor

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 7.0
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)


# ----------------------------------------------------------------------------- kernel
def _source(video_u8, layout, dtype):
    """A uint8 [3, N, Hs, Ws] CPU video on the device in one of the source forms."""
    if layout == "NTHWC":
        return video_u8.permute(1, 2, 3, 0).contiguous().cuda()
    return (video_u8.float() if dtype == torch.float32 else video_u8).cuda()


def _destination(form, dtype, n, c, t, crop):
    if form == "planar":
        return torch.full((n, c, t, crop, crop), SENTINEL, dtype=dtype, device="cuda"), None
    c_p, ld = {"c4": (4, 4), "cl8": (8, 8), "cl8_ld16": (8, 16), "cl16": (16, 16)}[form]
    return torch.full((n, t, crop, crop, ld), SENTINEL, dtype=dtype, device="cuda"), (c_p, ld)


def _set_destination(d, dst, cl, dtype, t, crop):
    d.dst, d.dst_dtype = dst.data_ptr(), (L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], t * crop * crop * cl[1]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _f32(a, b):
    return C.c_float(a / b).value


def _geometry(rec, src_ptr, n, hs, ws, size, crop, idxs):
    hn, wn = TR.scaled_size(hs, ws, size)
    assert crop <= hn and crop <= wn                             # every crop fits (checked on the CPU)
    rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn = src_ptr, n, hs, ws, hn, wn
    rec.sy, rec.sx = _f32(hs, hn), _f32(ws, wn)
    for k, v in enumerate(idxs):
        rec.y_off[k], rec.x_off[k] = TR.crop_offsets(hn, wn, crop, v)
    return hn, wn


def _upload(ctypes_array):
    return torch.frombuffer(ctypes_array, dtype=torch.uint8).cuda()


def _launch_batch(d, sources, items, form, dtype, c, t, crop, extra=2):
    """pv_batch_views into a sentinel-filled destination of `extra` more items than the launch writes."""
    from gpu_util import call
    keep = [_upload(sources), _upload(items)] + [x.cuda() for x in SU.affine()]
    d.sources, d.sources_dev = C.addressof(sources), keep[0].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[1].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.ch_scale, d.ch_shift = keep[2].data_ptr(), keep[3].data_ptr()
    dst, cl = _destination(form, dtype, len(items) + extra, c, t, crop)
    _set_destination(d, dst, cl, dtype, t, crop)
    call("pv_batch_views", d)
    return dst


def _items(triples):
    items = (L.ViewItem * len(triples))()
    for i, (s, r, v) in enumerate(triples):
        items[i].source, items[i].row, items[i].view = s, r, v
    return items


def _concat_tables(tables, stride):
    """The tables of all videos one after another, on the device, with a row stride of its own; the first row of each."""
    rows = sum(t.shape[0] for t in tables)
    tab = torch.zeros((rows, stride), dtype=torch.int32)
    row0, r = [], 0
    for t in tables:
        row0.append(r)
        tab[r:r + t.shape[0], :t.shape[1]] = t
        r += t.shape[0]
    return tab.cuda(), row0


def _alone_rgb(src, layout, table, size, crop, idxs, form, dtype):
    """pv_video_views on ONE video: all n_clips * n_views items."""
    from gpu_util import call
    n_clips, t = table.shape
    c, n, hs, ws = TR._video_geometry(src, layout)
    hn, wn = TR.scaled_size(hs, ws, size)
    tab = table.contiguous().cuda()
    keep = [x.cuda() for x in SU.affine()]
    d = L.VideoViewsDesc()
    d.src, d.t_index = src.data_ptr(), tab.data_ptr()
    d.n_clips, d.C, d.T, d.N, d.t_stride, d.Hs, d.Ws = n_clips, c, t, n, t, hs, ws
    d.src_dtype = L.PV_U8 if src.dtype == torch.uint8 else L.PV_F32
    d.src_layout = L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = hn, wn, crop, crop, len(idxs)
    for k, v in enumerate(idxs):
        d.y_off[k], d.x_off[k] = TR.crop_offsets(hn, wn, crop, v)
    d.ch_scale, d.ch_shift = keep[0].data_ptr(), keep[1].data_ptr()
    dst, cl = _destination(form, dtype, n_clips * len(idxs), c, t, crop)
    _set_destination(d, dst, cl, dtype, t, crop)
    call("pv_video_views", d)
    return dst


def _batch_rgb(srcs, layout, tables, stride, size, crop, idxs, triples, form, dtype):
    """pv_batch_views on the videos `srcs` for the items `triples` = (video, clip of that video, view)."""
    sources = (L.ViewSource * len(srcs))()
    for rec, src in zip(sources, srcs):
        c, n, hs, ws = TR._video_geometry(src, layout)
        _geometry(rec, src.data_ptr(), n, hs, ws, size, crop, idxs)
    tab, row0 = _concat_tables(tables, stride)
    d = L.BatchViewsDesc()
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], stride, 3, tables[0].shape[1]
    d.src_dtype = L.PV_U8 if srcs[0].dtype == torch.uint8 else L.PV_F32
    d.src_layout = L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC
    d.Ho, d.Wo, d.n_views = crop, crop, len(idxs)
    items = _items([(s, row0[s] + r, v) for s, r, v in triples])
    return _launch_batch(d, sources, items, form, dtype, 3, tables[0].shape[1], crop)


FORMS = [("c4", torch.bfloat16), ("cl8", torch.bfloat16), ("cl8", torch.float32), ("cl8_ld16", torch.bfloat16), ("cl16", torch.float32),
         ("planar", torch.bfloat16), ("planar", torch.float32)]
SOURCES = [("NCTHW", torch.uint8), ("NCTHW", torch.float32), ("NTHWC", torch.uint8)]
# landscape, portrait, and a small one that is upscaled; short side 64, crop 56
SIZES = [(12, 97, 131), (9, 131, 97), (5, 40, 53)]
# rows overlap, repeat frames and run backwards; the first and the last frame of every video
TABLES = [torch.tensor([[0, 2, 4], [3, 4, 5], [5, 5, 11], [11, 10, 0], [7, 7, 7]], dtype=torch.int32),
          torch.tensor([[8, 4, 0], [1, 1, 2]], dtype=torch.int32),
          torch.tensor([[4, 0, 4], [2, 3, 3], [0, 1, 2]], dtype=torch.int32)]


def _scrambled(tables, n_views):
    """Every (video, clip, view) once, in an order that jumps between the sources, and one item a second time."""
    every = [(s, r, v) for s, t in enumerate(tables) for r in range(t.shape[0]) for v in range(n_views)]
    order = torch.randperm(len(every), generator=torch.Generator().manual_seed(77 + n_views)).tolist()
    out = [every[i] for i in order]
    return out + [out[3]]


@pytest.fixture(scope="module")
def small_videos():
    return [SU.clip((3, n, h, w), 930 + i) for i, (n, h, w) in enumerate(SIZES)]


@pytest.mark.parametrize("form,dtype", FORMS, ids=["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS])
@pytest.mark.parametrize("layout,src_dtype", SOURCES, ids=["planar_u8", "planar_f32", "interleaved_u8"])
def test_batch_views_writes_the_bits_of_video_views_on_every_video_alone(small_videos, layout, src_dtype, form, dtype):
    """Three sources of different sizes in one launch, the items scrambled across them and one repeated; every destination
    form x source form; 3 views and 1 view; the items behind the launch keep the sentinel."""
    srcs = [_source(v, layout, src_dtype) for v in small_videos]
    for idxs in ((0, 1, 2), (2,)):
        triples = _scrambled(TABLES, len(idxs))
        assert len({s for s, _, _ in triples[:4]}) > 1           # the launch does jump between sources
        got = _batch_rgb(srcs, layout, TABLES, 5, 64, 56, idxs, triples, form, dtype)
        alone = [_alone_rgb(src, layout, tab, 64, 56, idxs, form, dtype) for src, tab in zip(srcs, TABLES)]
        what = "%s %s -> %s %s views %s" % (layout, src_dtype, form, dtype, idxs)
        for i, (s, r, v) in enumerate(triples):
            assert _same_bits(got[i], alone[s][r * len(idxs) + v]), "%s: item %d = video %d clip %d view %d" % (what, i, s, r, v)
        assert not torch.all(got[:len(triples)] == SENTINEL), what
        assert torch.all(got[len(triples):] == SENTINEL), "items behind the launch were written: " + what


def test_batch_views_at_full_geometry_mixes_sparse_and_dense_strips():
    """One launch holds a 720p video (source rows staged in pairs) and a 128 x 171 one (upscaled: the strip's rows staged as
    one run, no source row 16-byte aligned); short side to 256, 224 crops, 3 views, the items interleaved."""
    videos = [SU.clip((3, 6, 720, 1280), 940), SU.clip((3, 9, 128, 171), 941)]
    tables = [torch.tensor([[0, 1, 2, 3], [5, 5, 0, 4]], dtype=torch.int32),
              torch.tensor([[2, 3, 4, 5], [8, 8, 0, 7]], dtype=torch.int32)]
    triples = [(i % 2, r, v) for i, (r, v) in enumerate((r, v) for r in range(2) for v in range(3) for _ in range(2))]
    assert sorted(triples) == sorted((s, r, v) for s in range(2) for r in range(2) for v in range(3))
    for layout, src_dtype in SOURCES:
        srcs = [_source(v, layout, src_dtype) for v in videos]
        for form, dtype in (("c4", torch.bfloat16), ("planar", torch.bfloat16), ("cl8", torch.float32)):
            got = _batch_rgb(srcs, layout, tables, 4, 256, 224, (0, 1, 2), triples, form, dtype)
            alone = [_alone_rgb(src, layout, tab, 256, 224, (0, 1, 2), form, dtype) for src, tab in zip(srcs, tables)]
            for i, (s, r, v) in enumerate(triples):
                assert _same_bits(got[i], alone[s][r * 3 + v]), (layout, src_dtype, form, dtype, i, s, r, v)
            assert torch.all(got[len(triples):] == SENTINEL)


# ----------------------------------------------------------------------------- kernel, YUV
M601 = TR.yuv_matrix("bt601", False)


def _alone_yuv(frames, layout, table, size, crop, idxs, form, dtype, matrix, **geom_kw):
    """pv_yuv_views on ONE video: all n_clips * n_views items."""
    from gpu_util import call
    geom = TR.yuv_geometry(frames, layout, **geom_kw)
    tab = table.contiguous().cuda()
    d = TR._yuv_desc(frames, geom, tab, matrix, size, crop, idxs)
    keep = [x.cuda() for x in SU.affine()]
    d.ch_scale, d.ch_shift = keep[0].data_ptr(), keep[1].data_ptr()
    dst, cl = _destination(form, dtype, table.shape[0] * len(idxs), 3, table.shape[1], crop)
    _set_destination(d, dst, cl, dtype, table.shape[1], crop)
    call("pv_yuv_views", d)
    return dst


def _batch_yuv(frames, layouts, tables, size, crop, idxs, triples, form, dtype, matrix, geom_kws):
    sources = (L.ViewSource * len(frames))()
    steps = set()
    for rec, f, layout, kw in zip(sources, frames, layouts, geom_kws):
        g = TR.yuv_geometry(f, layout, **kw)
        _geometry(rec, f.data_ptr(), g["N"], g["Hs"], g["Ws"], size, crop, idxs)
        for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch"):
            setattr(rec, k, g[k])
        steps.add(g["c_step"])
    assert len(steps) == 1                                       # one launch has one chroma form
    tab, row0 = _concat_tables(tables, tables[0].shape[1])
    d = L.BatchViewsDesc()
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], tab.shape[1], 3, tables[0].shape[1]
    d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U8, L.SRC_YUV420, steps.pop(), matrix.data_ptr()
    d.Ho, d.Wo, d.n_views = crop, crop, len(idxs)
    items = _items([(s, row0[s] + r, v) for s, r, v in triples])
    return _launch_batch(d, sources, items, form, dtype, 3, tables[0].shape[1], crop)


@pytest.mark.parametrize("pair", [("NV12", "NV21"), ("I420", "YV12")], ids=["nv12_nv21", "i420_yv12"])
def test_batch_views_yuv_mixes_the_two_chroma_orders_of_one_form(pair):
    """NV12 as a decoder writes it -- pitched, a coded height above the display height, an odd base address -- beside a
    tight NV21 video of another size in ONE launch (c_step 2); I420 (pitched, coded) beside YV12 in another (c_step 1).  The
    order of U and V is the record's.  Every item equals pv_yuv_views on its video alone."""
    ya, yb = YU.planes(10, 98, 132, 1210), YU.planes(7, 66, 50, 1211)
    first = YU.pack(*ya, pair[0], coded_height=112, pitch=160, base=3 if pair[0] == "NV12" else 2, garbage=5).frames("cuda")
    second = YU.pack(*yb, pair[1]).frames("cuda")
    frames, kws = [first, second], [dict(coded_height=112, height=98), {}]
    tables = [torch.tensor([[0, 2, 2, 9], [7, 9, 4, 5], [3, 2, 1, 0]], dtype=torch.int32),
              torch.tensor([[6, 0, 3, 3], [1, 2, 4, 6]], dtype=torch.int32)]
    matrix = M601.float().reshape(12).cuda()
    every = [(s, r, v) for s in range(2) for r in range(tables[s].shape[0]) for v in range(3)]
    order = torch.randperm(len(every), generator=torch.Generator().manual_seed(5)).tolist()
    triples = [every[i] for i in order] + [every[order[0]]]
    for form, dtype in (("c4", torch.bfloat16), ("cl8_ld16", torch.bfloat16), ("cl8", torch.float32), ("planar", torch.bfloat16),
                        ("planar", torch.float32)):
        got = _batch_yuv(frames, pair, tables, 64, 56, (0, 1, 2), triples, form, dtype, matrix, kws)
        alone = [_alone_yuv(f, layout, tab, 64, 56, (0, 1, 2), form, dtype, matrix, **kw)
                 for f, layout, tab, kw in zip(frames, pair, tables, kws)]
        for i, (s, r, v) in enumerate(triples):
            assert _same_bits(got[i], alone[s][r * 3 + v]), (pair, form, dtype, i, s, r, v)
        assert torch.all(got[len(triples):] == SENTINEL) and not torch.all(got[:len(triples)] == SENTINEL)


# ----------------------------------------------------------------------------- packer
def _deploy(m, x, dtype=torch.bfloat16, **kw):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    transmute_model(m, "mi355x")
    xd = [t.cuda().to(dtype) for t in x] if isinstance(x, list) else x.cuda().to(dtype)
    return convert_to_deployable_form(m, xd, dtype=dtype, **kw)


def _x3d(batch, dtype=torch.bfloat16, **kw):
    """x3d_xs (4 x 160 x 160, 400 classes) converted for `batch` items."""
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    m = trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()
    return _deploy(m, seeded_input((batch, 3, 4, 160, 160), 6), dtype, **kw)


def _nthwc_video(n, hs, ws, seed):
    return SU.clip((3, n, hs, ws), seed).permute(1, 2, 3, 0).contiguous().cuda()


def _input_items(packer):
    """[B, elements] view of the buffer the forward reads for pathway 0: the packer's own NCDHW clip, or the arena buffer;
    the sub-plans of a split-batch form one after another."""
    if packer.subs is not None:
        return torch.cat([_input_items(s) for s in packer.subs])
    if packer._planar:
        return packer._planar[0].view(packer._planar[0].shape[0], -1)
    ref, sess = packer.refs[0], packer.sess
    return sess.arena_t[ref.off: ref.off + ref.B * ref.bs * ref.itemsize].view(ref.B, -1)


@pytest.fixture(scope="module")
def x3d6():
    return _x3d(6)


@pytest.fixture(scope="module")
def x3d6_split():
    dep = _x3d(6, streams=2)
    assert list(dep._splits) == [3, 3]
    return dep


@pytest.mark.parametrize("kind", ["bf16_planar_stem", "fp32_arena", "streams2"])
def test_fill_batch_writes_the_items_fill_video_writes_for_every_video(kind, x3d6, x3d6_split):
    """x3d_xs at batch 6; three videos of different sizes with 1, 1 and 3 clips x 3 views = 15 items.  Chunks that start
    inside the first video and span all three, that start and end inside the third, and a short last chunk with a zero tail."""
    dep = {"bf16_planar_stem": lambda: x3d6, "fp32_arena": lambda: _x3d(6, dtype=torch.float32), "streams2": lambda: x3d6_split}[kind]()
    packer = TR.DevicePacker(dep, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
    videos = [_nthwc_video(9, 180, 240, 950), _nthwc_video(6, 250, 190, 951), _nthwc_video(12, 120, 161, 952)]
    tables = [torch.tensor([[0, 2, 5, 8]]), torch.tensor([[5, 3, 1, 0]]), torch.tensor([[0, 1, 2, 3], [4, 6, 8, 11], [11, 11, 7, 2]])]
    # what fill_video writes, video by video (cloned: the buffers are reused)
    want = []
    for video, table in zip(videos, tables):
        one = packer.video_tables(table, video.shape[0])
        total = table.shape[0] * 3
        for i0 in range(0, total, 6):
            n = min(6, total - i0)
            packer.fill_video(video, one, i0, n)
            want.extend(_input_items(packer)[:n].clone())
    assert len(want) == 15 and (kind != "bf16_planar_stem" or bool(packer._planar))
    batch = packer.video_batch(videos, tables)
    assert batch.total == 15 and batch.video_of.tolist() == [0] * 3 + [1] * 3 + [2] * 9
    assert batch.clip_of.tolist() == [r for r in range(5) for _ in range(3)] and batch.video_of.is_cuda
    for i0, n in ((1, 6), (7, 6), (0, 6), (12, 3), (14, 1), (6, 6)):
        packer.fill_batch(batch, i0, n)
        got = _input_items(packer)
        for k in range(n):
            assert torch.equal(got[k], want[i0 + k]), "%s: item %d of chunk [%d, +%d)" % (kind, k, i0, n)
        assert not bool((got[n:] != 0).any()), "%s: the tail of chunk [%d, +%d) must be zero" % (kind, i0, n)
    for i0, n in ((0, 7), (15, 1), (10, 6), (-1, 2), (0, 0)):    # chunks that leave the sequence or the deploy batch
        with pytest.raises(RuntimeError):
            packer.fill_batch(batch, i0, n)


# ----------------------------------------------------------------------------- scores
def _check_scores(dep, sampler, videos, fps, short_side, crop, views, frame_ratios=None, method="sum"):
    """Same-size videos make an exact oracle: their concatenation is ONE video whose frame table is the videos' tables with
    frame offsets, so `fill_video` + `launch` on it, chunk by chunk, feeds the forward the same items at the same batch
    positions; folded by `VideoEnsembler` with the same video_of it must give the same scores, bit for bit."""
    pred = VideoBatchPredictor(dep, sampler, short_side=short_side, crop_size=crop, spatial_idx=views, frame_ratios=frame_ratios,
                               method=method, **KW)
    p = pred.packer
    scores, clip_scores = pred(videos, fps, return_clip_scores=True)
    scores, clip_scores = scores.clone(), [c.clone() for c in clip_scores]
    tables = [D.clip_frame_table(sampler, v.shape[0], fps, p.clip_frames)[0] for v in videos]
    clips = [t.shape[0] for t in tables]
    n_views, total = len(views), sum(clips) * len(views)
    assert pred.video_ensembler.counts.tolist() == [c * n_views for c in clips]          # the views per video, exactly
    assert pred.clip_ensembler.counts.tolist() == [n_views] * sum(clips)
    assert pred.forwards == -(-total // p.batch)
    assert scores.dtype == torch.float32 and scores.shape[0] == len(videos) and [c.shape[0] for c in clip_scores] == clips
    # the oracle
    whole = torch.cat(videos)
    first = [0]
    for v in videos[:-1]:
        first.append(first[-1] + v.shape[0])
    table = torch.cat([t + f for t, f in zip(tables, first)])
    video_of = torch.tensor([j for j, c in enumerate(clips) for _ in range(c * n_views)], dtype=torch.int32, device="cuda")
    one = p.video_tables(table, whole.shape[0])
    ve = VideoEnsembler(len(videos), scores.shape[1], method)
    ce = VideoEnsembler(sum(clips), scores.shape[1], method)
    for i0 in range(0, total, p.batch):
        n = min(p.batch, total - i0)
        p.fill_video(whole, one, i0, n)
        logits = p.launch()[:n]
        ve.update(logits, video_of[i0:i0 + n])
        ce.update(logits, torch.arange(i0, i0 + n, dtype=torch.int32, device="cuda") // n_views)
    want, want_clips = ve.result(), ce.result()
    assert torch.equal(scores, want), "video scores differ by %.3e" % (scores - want).abs().max().item()
    assert torch.equal(torch.cat(clip_scores), want_clips)
    assert torch.equal(pred(videos, fps), scores)                # without the clip scores: the same video scores
    assert not torch.equal(scores[0], scores[1])                 # the videos are different frames
    return pred, total


@pytest.mark.parametrize("streams", [1, 2])
def test_batch_predictor_x3d_equals_the_concatenated_video(streams, x3d6, x3d6_split):
    """x3d_xs at batch 6, three 180 x 240 videos of 24, 5 and 17 frames at 10 fps, clips of 8 frames subsampled to 4."""
    dep = x3d6_split if streams == 2 else x3d6
    videos = [_nthwc_video(n, 180, 240, 960 + n) for n in (24, 5, 17)]
    clip = Fraction(8, 10)
    _, total = _check_scores(dep, D.UniformClipSampler(clip), videos, 10, 176, 160, (0, 1, 2))
    assert total == 18                                           # 3 + 1 + 2 clips x 3 views: three full forwards, where
    #                                                              one video per call takes 2 + 1 + 1 = 4
    _, total = _check_scores(dep, D.ConstantClipsPerVideoSampler(clip, 5), videos, 10, 176, 160, (0, 2), method="max")
    assert total == 30
    _, total = _check_scores(dep, D.UniformClipSampler(clip, Fraction(3, 10), True), videos, 10, 176, 160, (0, 1, 2))
    assert total == 36                                           # overlapping clips, the last one of a video back-padded
    _, total = _check_scores(dep, D.ConstantClipsPerVideoSampler(clip, 3), videos, 10, 176, 160, (0, 1, 2))
    assert total == 27                                           # four full forwards and a short last chunk of 3


def test_batch_predictor_slowfast_and_mvit():
    """slowfast_r50_small (4 + 16 frames at 96 x 96, frame_ratios (4, 1), batch 4): both pathways read column subsets of
    the one concatenated table; mvit_b_small (4 x 64 x 64, batch 6)."""
    from oracle.weights import deterministic_fill, seeded_input
    from pytorchvideo_amd.models import create_multiscale_vision_transformers, create_slowfast
    g = torch.load(os.path.join(GOLD, "slowfast_r50_small.pt"), weights_only=False)
    m = deterministic_fill(create_slowfast(**g["cfg"]), g["seed"]).eval()
    fast = seeded_input((4, 3, 16, 96, 96), 7)
    dep = _deploy(m, [TR.uniform_temporal_subsample(fast, 4, 2), fast])
    videos = [_nthwc_video(n, 131, 113, 970 + n) for n in (40, 9, 25)]
    pred, total = _check_scores(dep, D.ConstantClipsPerVideoSampler(Fraction(24, 20), 3, 2), videos, 20, 100, 96, (0, 2),
                                frame_ratios=(4, 1))
    assert total == 18 and pred.packer.clip_frames == 16         # 4 full forwards and a short one
    g = torch.load(os.path.join(GOLD, "mvit_b_small.pt"), weights_only=False)
    m = deterministic_fill(create_multiscale_vision_transformers(**g["cfg"]), g["seed"]).eval()
    dep = _deploy(m, seeded_input((6, 3, 4, 64, 64), 8))
    videos = [_nthwc_video(n, 75, 101, 980 + n) for n in (20, 4, 11)]
    _check_scores(dep, D.UniformClipSampler(Fraction(6, 10)), videos, 10, 70, 64, (0, 1, 2))


# ----------------------------------------------------------------------------- refusals
def test_batch_predictor_refuses_what_it_cannot_score(x3d6):
    """Errors before any launch: a detection model; a CPU tensor, a video whose crop does not fit and a table entry outside
    ITS video (while inside a longer neighbour) leave the input buffers as they were."""
    from oracle.weights import detection_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    g = torch.load(os.path.join(GOLD, "resnet_det_r50_small.pt"), weights_only=False)
    m = detection_fill(create_resnet_with_roi_head(**g["cfg"]), g["seed"]).eval()
    transmute_model(m, "mi355x")
    x = SU.normalised(SU.clip((3, 4, 64, 64), 916))[None].repeat(2, 1, 1, 1, 1)
    dm = convert_to_deployable_form(m, (x.cuda().bfloat16(), g["boxes"]), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="detection"):
        VideoBatchPredictor(dm, D.UniformClipSampler(1), short_side=72, crop_size=64, **KW)
    pred = VideoBatchPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, **KW)
    good = [_nthwc_video(12, 180, 240, 990), _nthwc_video(8, 200, 180, 991)]
    pred(good, 10)
    before, forwards = _input_items(pred.packer).clone(), pred.forwards
    with pytest.raises(RuntimeError, match="is on cpu"):
        pred([good[0], good[1].cpu()], 10)
    # the short side is scaled to 150, below the 160 crop of the deploy form: no frame is large enough
    small = VideoBatchPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), short_side=150, crop_size=160, **KW)
    with pytest.raises(RuntimeError, match="crop does not fit"):
        small(good, 10)
    with pytest.raises(ValueError, match="leave the video"):
        pred.packer.video_batch(good, [torch.tensor([[0, 3, 7, 11]]), torch.tensor([[0, 3, 7, 11]])])   # frame 11 of 8
    assert pred.packer.video_batch(good, [torch.tensor([[0, 3, 7, 11]]), torch.tensor([[0, 3, 5, 7]])]).total == 6
    with pytest.raises(ValueError):
        pred(good, [10])                                         # one fps for two videos
    assert torch.equal(_input_items(pred.packer), before) and pred.forwards == forwards
