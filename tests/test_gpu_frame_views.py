"""Frame-list sources on the MI355X: `pv_frame_views` (every frame individually addressed, include/pv_mi355x.h),
`transforms.FrameList` through `DevicePacker.video_batch` / `fill_batch` and the three predictors, and
`inference.StreamPredictor`.

Reference, bit for bit (`torch.equal` on the raw bits, no tolerance): the entry points that take one allocation per video --
`pv_batch_views` on the frames stacked into one tensor, and the predictors on that tensor.  The kernels wrap the same
staged-strip bodies and hand them the same values but the frame's address, so any difference is a bug.  For whole models the
oracle is "the same items at the same batch positions" (tests/test_gpu_batch_views.py, `_check_scores`).

Every frame is an allocation of its own; the lists run against the allocation order, name a frame twice, and uint8 frames are
views at byte offsets 1 and 7 inside larger buffers.  The helpers and the geometry are those of tests/test_gpu_batch_views.py
and tests/test_gpu_keyframe_detection.py."""
from fractions import Fraction

import pytest
import torch

import spatial_util as SU
import test_gpu_batch_views as BV
import test_gpu_keyframe_detection as KD
import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import KeyframeDetector, StreamPredictor, VideoBatchPredictor, VideoPredictor

pytestmark = pytest.mark.gpu
KW = BV.KW


# ----------------------------------------------------------------------------- frames
def _own_frames(frames, seed):
    """Every tensor of `frames` (CPU or device, any strides) copied into a device allocation of its own, with its shape and
    strides, as a view at byte offset 1 or 7 (uint8; fp32: 4 or 12) inside a larger buffer filled with other bytes.  The
    buffers are allocated in a shuffled order, so the list order is not the allocation order."""
    frames = list(frames)
    order = torch.randperm(len(frames), generator=torch.Generator().manual_seed(seed)).tolist()
    out = [None] * len(frames)
    for i in order:
        f = frames[i]
        item = f.element_size()
        extent = 1 + sum((n - 1) * s for n, s in zip(f.shape, f.stride()))           # elements from the first to the last
        buf = torch.full(((extent + 4) * item + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        off = (1, 7)[i % 2] if item == 1 else (4, 12)[i % 2]
        own = torch.as_strided(buf[off:off + extent * item].view(f.dtype), tuple(f.shape), f.stride())
        own.copy_(f)
        assert own.data_ptr() == buf.data_ptr() + off
        out[i] = own
    return out


def _own_surfaces(video, seed):
    """The pitched YUV surfaces of `video` (CPU, [N, Hc*3/2, W] with a row pitch P >= W) as device allocations of their own
    at odd addresses, in a shuffled allocation order.  A surface is its Hc*3/2 * P bytes, not the W columns of its rows: the
    half-pitch chroma rows of the planar forms lie partly behind column W."""
    n, rows, w = video.shape
    pitch = video.stride(1)
    out = [None] * n
    for i in torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist():
        buf = torch.full((rows * pitch + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        off = (1, 7)[i % 2]
        buf[off:off + rows * pitch].copy_(torch.as_strided(video[i], (rows * pitch,), (1,)))
        out[i] = torch.as_strided(buf, (rows, w), (pitch, 1), off)
    return out


def _rgb_lists(small_videos, layout, src_dtype):
    """Per-frame lists of the three small videos in one source form; video 0 names frame 1 a second time at position 5 and
    video 1 runs backwards through its allocations."""
    lists = []
    for j, v in enumerate(small_videos):                         # uint8 [3, N, H, W] on the CPU
        v = v.float() if src_dtype == torch.float32 else v
        per_frame = v.permute(1, 2, 3, 0).contiguous().unbind(0) if layout == "NTHWC" else v.unbind(1)
        own = _own_frames([f.contiguous() for f in per_frame], 1300 + j)
        if j == 0:
            own[5] = own[1]
        if j == 1:
            own = own[::-1]
        lists.append(own)
    return lists


def _stacked(frames, layout):
    return torch.stack(frames, dim=1 if layout == "NCTHW" else 0).contiguous()


def _launch_frames(lists, fill_record, fill_desc, tables, stride, idxs, triples, form, dtype, crop):
    """pv_frame_views on the per-frame `lists` for the items `triples` = (video, clip of that video, view), into a
    sentinel-filled destination of two more items than the launch writes."""
    from gpu_util import call
    sources = (L.ViewSource * len(lists))()
    ptrs = torch.tensor([f.data_ptr() for own in lists for f in own], dtype=torch.int64)
    ptrs_dev = ptrs.cuda()
    first = 0
    for rec, own in zip(sources, lists):
        fill_record(rec, own, ptrs_dev.data_ptr() + 8 * first)
        first += len(own)
    tab, row0 = BV._concat_tables(tables, stride)
    items = BV._items([(s, row0[s] + r, v) for s, r, v in triples])
    f = L.FrameViewsDesc()
    d = f.batch
    t = tables[0].shape[1]
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], stride, 3, t
    d.Ho, d.Wo, d.n_views = crop, crop, len(idxs)
    fill_desc(d)
    keep = [BV._upload(sources), BV._upload(items)] + [x.cuda() for x in SU.affine()]
    d.sources, d.sources_dev = BV.C.addressof(sources), keep[0].data_ptr()
    d.items, d.items_dev = BV.C.addressof(items), keep[1].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.ch_scale, d.ch_shift = keep[2].data_ptr(), keep[3].data_ptr()
    dst, cl = BV._destination(form, dtype, len(items) + 2, 3, t, crop)
    BV._set_destination(d, dst, cl, dtype, t, crop)
    f.frame_ptrs, f.frame_ptrs_dev, f.n_frame_ptrs = ptrs.data_ptr(), ptrs_dev.data_ptr(), ptrs.numel()
    call("pv_frame_views", f)
    return dst


# ----------------------------------------------------------------------------- kernel
@pytest.fixture(scope="module")
def small_videos():
    return [SU.clip((3, n, h, w), 930 + i) for i, (n, h, w) in enumerate(BV.SIZES)]


@pytest.mark.parametrize("form,dtype", BV.FORMS, ids=["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in BV.FORMS])
@pytest.mark.parametrize("layout,src_dtype", BV.SOURCES, ids=["planar_u8", "planar_f32", "interleaved_u8"])
def test_frame_views_writes_the_bits_of_batch_views_on_the_stacked_videos(small_videos, layout, src_dtype, form, dtype):
    """Three sources of different sizes in one launch, every frame its own allocation, the items scrambled across the
    sources and one repeated; every destination form x source form; 3 views and 1 view; the items behind the launch keep
    the sentinel."""
    lists = _rgb_lists(small_videos, layout, src_dtype)
    assert lists[0][5] is lists[0][1]
    stacked = [_stacked(own, layout) for own in lists]

    def fill_record(rec, own, slice_ptr):
        c, hs, ws, _ = TR.FrameList(own, layout).geometry(layout)
        BV._geometry(rec, slice_ptr, len(own), hs, ws, 64, 56, idxs)

    def fill_desc(d):
        d.src_dtype = L.PV_U8 if src_dtype == torch.uint8 else L.PV_F32
        d.src_layout = L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC

    for idxs in ((0, 1, 2), (2,)):
        triples = BV._scrambled(BV.TABLES, len(idxs))
        assert len({s for s, _, _ in triples[:4]}) > 1           # the launch does jump between sources
        got = _launch_frames(lists, fill_record, fill_desc, BV.TABLES, 5, idxs, triples, form, dtype, 56)
        want = BV._batch_rgb(stacked, layout, BV.TABLES, 5, 64, 56, idxs, triples, form, dtype)
        what = "%s %s -> %s %s views %s" % (layout, src_dtype, form, dtype, idxs)
        for i, (s, r, v) in enumerate(triples):
            assert BV._same_bits(got[i], want[i]), "%s: item %d = video %d clip %d view %d" % (what, i, s, r, v)
        assert not torch.all(got[:len(triples)] == BV.SENTINEL), what
        assert torch.all(got[len(triples):] == BV.SENTINEL), "items behind the launch were written: " + what


@pytest.mark.parametrize("pair", [("NV12", "NV21"), ("I420", "YV12")], ids=["nv12_nv21", "i420_yv12"])
def test_frame_views_yuv_reads_pitched_surfaces_at_odd_addresses(pair):
    """Per chroma form one launch with both chroma orders: surfaces with a row pitch above W (and, for the first source, a
    coded height above the display height), each its own allocation at an odd address.  Bits equal to pv_batch_views on a
    video built from the same surfaces with the same pitch."""
    ya, yb = YU.planes(10, 98, 132, 1210), YU.planes(7, 66, 50, 1211)
    packed = [YU.pack(*ya, pair[0], coded_height=112, pitch=160, garbage=5).frames(), YU.pack(*yb, pair[1], pitch=64).frames()]
    kws = [dict(coded_height=112, height=98), {}]
    lists = [_own_surfaces(p, 1400 + j) for j, p in enumerate(packed)]
    lists[1][3] = lists[1][6]                                    # one surface named twice
    assert all(f.stride(0) > f.shape[1] and f.data_ptr() % 2 == 1 for own in lists for f in own)
    videos = []
    for own, base in zip(lists, (3, 2)):                         # the same surfaces as ONE video of the same pitch
        rows, w, pitch = own[0].shape[0], own[0].shape[1], own[0].stride(0)
        buf = torch.full((base + len(own) * rows * pitch + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        for i, f in enumerate(own):
            buf[base + i * rows * pitch: base + (i + 1) * rows * pitch].copy_(torch.as_strided(f, (rows * pitch,), (1,)))
        videos.append(torch.as_strided(buf, (len(own), rows, w), (rows * pitch, pitch, 1), base))
    tables = [torch.tensor([[0, 2, 2, 9], [7, 9, 4, 5], [3, 2, 1, 0]], dtype=torch.int32),
              torch.tensor([[6, 0, 3, 3], [1, 2, 4, 6]], dtype=torch.int32)]
    matrix = BV.M601.float().reshape(12).cuda()
    every = [(s, r, v) for s in range(2) for r in range(tables[s].shape[0]) for v in range(3)]
    order = torch.randperm(len(every), generator=torch.Generator().manual_seed(5)).tolist()
    triples = [every[i] for i in order] + [every[order[0]]]
    geoms = [TR.yuv_geometry(own[0][None], layout, **kw) for own, layout, kw in zip(lists, pair, kws)]
    assert len({g["c_step"] for g in geoms}) == 1

    def fill_record(rec, own, slice_ptr):
        g = geoms[[id(x) for x in lists].index(id(own))]
        BV._geometry(rec, slice_ptr, len(own), g["Hs"], g["Ws"], 64, 56, (0, 1, 2))
        for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch"):
            setattr(rec, k, g[k])

    def fill_desc(d):
        d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U8, L.SRC_YUV420, geoms[0]["c_step"], matrix.data_ptr()

    for form, dtype in (("c4", torch.bfloat16), ("cl8_ld16", torch.bfloat16), ("cl8", torch.float32), ("planar", torch.bfloat16),
                        ("planar", torch.float32)):
        got = _launch_frames(lists, fill_record, fill_desc, tables, 4, (0, 1, 2), triples, form, dtype, 56)
        want = BV._batch_yuv(videos, pair, tables, 64, 56, (0, 1, 2), triples, form, dtype, matrix, kws)
        for i, (s, r, v) in enumerate(triples):
            assert BV._same_bits(got[i], want[i]), (pair, form, dtype, i, s, r, v)
        assert torch.all(got[len(triples):] == BV.SENTINEL) and not torch.all(got[:len(triples)] == BV.SENTINEL)


# ----------------------------------------------------------------------------- predictors
@pytest.fixture(scope="module")
def x3d6():
    return BV._x3d(6)


@pytest.fixture(scope="module")
def x3d6_split():
    dep = BV._x3d(6, streams=2)
    assert list(dep._splits) == [3, 3]
    return dep


def _frame_list(video, seed):
    """A [N,H,W,3] (or [N, rows, W]) device video as a FrameList of per-frame allocations."""
    return TR.FrameList(_own_frames(video.unbind(0), seed))


@pytest.mark.parametrize("streams", [1, 2])
def test_batch_predictor_on_frame_lists_equals_the_stacked_videos(streams, x3d6, x3d6_split):
    """x3d_xs at batch 6, three 180 x 240 videos of 24, 5 and 17 frames at 10 fps: 3 + 1 + 2 clips x 3 views."""
    dep = x3d6_split if streams == 2 else x3d6
    videos = [BV._nthwc_video(n, 180, 240, 960 + n) for n in (24, 5, 17)]
    lists = [_frame_list(v, 1500 + i) for i, v in enumerate(videos)]
    pred = VideoBatchPredictor(dep, D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)
    want, want_clips = pred(videos, 10, return_clip_scores=True)
    forwards = pred.forwards
    got, got_clips = pred(lists, 10, return_clip_scores=True)
    assert pred.forwards == forwards == 3
    assert torch.equal(got, want) and not torch.equal(got[0], got[1])
    assert len(got_clips) == 3 and all(torch.equal(a, b) for a, b in zip(got_clips, want_clips))
    assert pred.video_ensembler.counts.tolist() == [9, 3, 6]


def test_video_predictor_on_a_frame_list_equals_the_stacked_video(x3d6):
    video = BV._nthwc_video(23, 180, 240, 983)
    frames = _frame_list(video, 1510)
    pred = VideoPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10), Fraction(3, 10)), short_side=176, crop_size=160, **KW)
    want, want_clips = pred(video, 10, return_clip_scores=True)
    got, got_clips = pred(frames, 10, return_clip_scores=True)
    assert tuple(got_clips.shape) == (6, 400) and torch.equal(got, want) and torch.equal(got_clips, want_clips)
    assert torch.equal(pred(frames, 10), want)
    assert not torch.equal(got_clips[0], got_clips[5])


def test_keyframe_detector_on_frame_lists_equals_the_stacked_video():
    dm = KD._form("resnet_det_r50_small", torch.bfloat16, 48, 72)[0]
    box_list = KD._split(KD.box_set(60, 90), KD.COUNTS)
    video = KD._video(40, 60, 90, 4100).cuda()
    det = KeyframeDetector(dm, KD.DURATION, short_side=48, **KW)
    want = det(video, KD.FPS, KD.STAMPS, box_list).clone()
    got = det(_frame_list(video, 1520), KD.FPS, KD.STAMPS, box_list)
    assert tuple(got.shape) == (sum(KD.COUNTS), 16) and torch.equal(got, want) and det.forwards == 2
    # a list of videos, as FrameLists
    got2 = det([_frame_list(video, 1521), _frame_list(video[:30], 1522)], KD.FPS, [KD.STAMPS, KD.STAMPS[:2]], [box_list, box_list[:2]])
    want2 = det([video, video[:30].contiguous()], KD.FPS, [KD.STAMPS, KD.STAMPS[:2]], [box_list, box_list[:2]])
    assert torch.equal(got2, want2)
    # NV12 surfaces
    nv = YU.pack(*YU.planes(40, 60, 90, 4200), "NV12").frames("cuda")
    det = KeyframeDetector(dm, KD.DURATION, short_side=48, src_layout="NV12", yuv=("bt709", False), **KW)
    want = det(nv, KD.FPS, KD.STAMPS, box_list).clone()
    got = det(_frame_list(nv, 1523), KD.FPS, KD.STAMPS, box_list)
    assert torch.equal(got, want) and bool((got != 0).any())


# ----------------------------------------------------------------------------- streams
DUR, STRIDE, FPS = Fraction(8, 10), Fraction(3, 10), 10


@pytest.fixture(scope="module")
def stream_case(x3d6):
    """A 23-frame 180 x 240 stream and what `VideoPredictor` gives for its 6 windows, computed once."""
    video = BV._nthwc_video(23, 180, 240, 1600)
    frames = _own_frames(video.unbind(0), 1601)
    pred = VideoPredictor(x3d6, D.UniformClipSampler(DUR, STRIDE), short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)
    clip_scores = pred(video, FPS, return_clip_scores=True)[1].clone()
    assert tuple(clip_scores.shape) == (6, 400)
    return video, frames, clip_scores


def _stream(dep):
    return StreamPredictor(dep, DUR, STRIDE, FPS, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)


def test_stream_predictor_one_push_equals_the_video_predictor(x3d6, stream_case):
    video, frames, clip_scores = stream_case
    sp = _stream(x3d6)
    out = sp.push(frames)
    assert [k for k, _, _ in out] == list(range(6)) and [s for _, s, _ in out] == [k * STRIDE for k in range(6)]
    assert sp.forwards == 3                                      # 18 items in chunks of 6, from position 0
    for k, _, scores in out:
        assert scores.dtype == torch.float32 and tuple(scores.shape) == (400,) and scores.is_cuda
        assert torch.equal(scores, clip_scores[k]), k
    assert sp.frames_held <= sp.state.bound + len(frames)
    # a new stream on the same object: the same frames give the same scores
    sp.reset()
    assert sp.frames_held == 0
    again = sp.push(iter(frames))
    assert [k for k, _, _ in again] == list(range(6)) and all(torch.equal(a[2], b[2]) for a, b in zip(again, out))


def test_stream_predictor_scores_the_windows_each_push_completes(x3d6, stream_case):
    """Pushes of 7, 7, 7 and 2 frames emit 0, 3, 2 and 1 windows.  The oracle of an emission: the same rows of the stacked
    video at the same batch positions, through `fill_video`."""
    video, frames, clip_scores = stream_case
    sp = _stream(x3d6)
    p, t = sp.packer, sp.packer.clip_frames
    emitted, lo = [], 0
    for n, count in zip((7, 7, 7, 2), (0, 3, 2, 1)):
        out = sp.push(frames[lo:lo + n])
        lo += n
        assert len(out) == count and sp.frames_held <= sp.state.bound + n, (n, len(out), sp.frames_held)
        assert sp.frames_held == sp.state.held and sp.forwards == -(-count * 3 // 6)
        emitted.extend(out)
        if not out:
            continue
        out = [(k, s, scores.clone()) for k, s, scores in out]
        windows = D.stream_windows(DUR, STRIDE, FPS, lo, out[0][0])
        assert [w[0] for w in windows] == [k for k, _, _ in out]
        table = torch.stack([first + TR.temporal_indices(stop - first, t) for _, _, first, stop in windows])
        one = p.video_tables(table, video.shape[0])
        ce = VideoEnsembler(count, 400, "sum")
        for i0 in range(0, count * 3, 6):
            m = min(6, count * 3 - i0)
            p.fill_video(video, one, i0, m)
            ce.update(p.launch()[:m], torch.arange(i0, i0 + m, dtype=torch.int32, device="cuda") // 3)
        want = ce.result()
        for i, (k, _, scores) in enumerate(out):
            assert torch.equal(scores, want[i]), (n, k)
    assert [k for k, _, _ in emitted] == list(range(6))
    assert sp.state.base == 18 and sp.frames_held == 5           # window 6 starts at frame 18
    assert not torch.equal(emitted[0][2], emitted[5][2])


def test_stream_predictor_frame_by_frame_emits_the_same_windows(x3d6, stream_case):
    video, frames, clip_scores = stream_case
    sp = _stream(x3d6)
    seen = []
    for i, f in enumerate(frames):
        out = sp.push([f])
        assert len(out) <= 1 and sp.frames_held <= sp.state.bound + 1
        seen.extend((i, k, s) for k, s, _ in out)
    # window k completes with frame ceil(fps (k stride + d)) - 1
    assert [(i, k) for i, k, _ in seen] == [(7, 0), (10, 1), (13, 2), (16, 3), (19, 4), (22, 5)]
    assert [s for _, _, s in seen] == [k * STRIDE for k in range(6)]
    assert sp.push([]) == []


# ----------------------------------------------------------------------------- refusals
def test_frame_lists_are_refused_before_any_launch(x3d6):
    pred = VideoBatchPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, **KW)
    good = [BV._nthwc_video(12, 180, 240, 990), BV._nthwc_video(8, 200, 180, 991)]
    pred(good, 10)
    before, forwards = BV._input_items(pred.packer).clone(), pred.forwards
    lists = [TR.FrameList(v.unbind(0)) for v in good]
    with pytest.raises(ValueError, match="tensors.*FrameLists"):
        pred([good[0], lists[1]], 10)
    with pytest.raises(ValueError, match="tensors.*FrameLists"):
        pred([lists[0], good[1]], 10)
    with pytest.raises(RuntimeError, match="is on cpu"):
        pred([lists[0], TR.FrameList(good[1].cpu().unbind(0))], 10)
    one = VideoPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, **KW)
    with pytest.raises(RuntimeError, match="is on cpu"):
        one(TR.FrameList(good[0].cpu().unbind(0)), 10)
    with pytest.raises(RuntimeError, match="video_batch"):
        one.packer.fill_video(lists[0], one.packer.video_tables(torch.tensor([[0, 3, 7, 11]]), 12), 0, 3)
    with pytest.raises(RuntimeError, match="video_batch"):
        one.packer(lists[0])
    sp = _stream(x3d6)
    with pytest.raises(RuntimeError, match="on cpu"):
        sp.push(good[0].cpu().unbind(0))
    with pytest.raises(RuntimeError, match="shape"):
        sp.push([good[0][0], good[1][0]])
    assert sp.frames_held == 0 and sp.state.seen == 0
    dm = KD._form("resnet_det_r50_small", torch.bfloat16, 48, 72)[0]
    with pytest.raises(ValueError, match="classification"):
        StreamPredictor(dm, DUR, STRIDE, FPS, short_side=48, crop_size=48, **KW)
    assert torch.equal(BV._input_items(pred.packer), before) and pred.forwards == forwards
    assert torch.equal(pred(lists, 10), pred(good, 10))          # and the predictor still scores
