"""Whole-video inference on the MI355X: `pv_video_views` (clip sampling fused into the resampling ingest, include/pv_mi355x.h),
`DevicePacker.fill_video` and `inference.VideoPredictor`.

Reference, bit for bit (`torch.equal`, no tolerance): the pieces the existing suite already holds against the reference --
`pv_resample_crop` on the clips materialised by index_select (tests/test_gpu_resample.py pins it to the reference's
fixtures), and for whole models the SAME deploy form driven clip batch by clip batch through `DevicePacker.__call__` and
folded by `VideoEnsembler`.  The new path runs the same instruction sequence on the same taps and must feed the forward
identical bytes, so any difference is a bug.  No test here feeds the device a table that leaves the video: the range check
is the Python layer's (tests/test_clip_sampling.py) and the kernel's clamp is defence only."""
import os
from fractions import Fraction

import pytest
import torch

import spatial_util as SU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import VideoPredictor

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 7.0


# ----------------------------------------------------------------------------- kernel
def _video(n, hs, ws, seed):
    """uint8 [3, N, Hs, Ws] on the CPU."""
    return SU.clip((3, n, hs, ws), seed)


def _source(video_u8, layout, dtype):
    """The video on the device in one of the source forms pv_resample_crop accepts, and its materialiser."""
    if layout == "NTHWC":
        return video_u8.permute(1, 2, 3, 0).contiguous().cuda()
    return (video_u8.float() if dtype == torch.float32 else video_u8).cuda()


def _materialise(src, layout, table):
    """[n_clips, ...] clips by index_select, in the clip form of the same layout."""
    n_clips, t = table.shape
    flat = table.reshape(-1).long().to(src.device)
    if layout == "NTHWC":
        return src.index_select(0, flat).view(n_clips, t, *src.shape[1:]).contiguous()
    c = src.shape[0]
    return src.index_select(1, flat).view(c, n_clips, t, *src.shape[2:]).permute(1, 0, 2, 3, 4).contiguous()


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


def _both(src, layout, table, stride, size, crop, idxs, form, dtype, item0, n_items, extra=2, affine=True):
    """(pv_video_views on the video + table, pv_resample_crop on the materialised clips): two sentinel-filled destinations
    of `extra` more items than the window."""
    from gpu_util import call
    n_clips, t = table.shape
    clips = _materialise(src, layout, table)
    old = TR._resample_desc(clips, layout, size, crop, idxs)
    n = n_items if n_items else n_clips * len(idxs)
    keep = []
    if affine:
        scale, shift = [x.cuda() for x in SU.affine()]
        keep = [scale, shift]
    # the table on the device with a row stride of its own (the columns behind T are never read: poisoned with a valid frame)
    tab = torch.zeros((n_clips, stride), dtype=torch.int32)
    tab[:, :t] = table
    tab = tab.cuda()
    new = L.VideoViewsDesc()
    new.src, new.t_index = src.data_ptr(), tab.data_ptr()
    new.n_clips, new.C, new.T, new.t_stride = n_clips, old.C, t, stride
    new.N = src.shape[0] if layout == "NTHWC" else src.shape[1]
    new.Hs, new.Ws, new.src_dtype, new.src_layout = old.Hs, old.Ws, old.src_dtype, old.src_layout
    new.Hn, new.Wn, new.Ho, new.Wo, new.n_views = old.Hn, old.Wn, old.Ho, old.Wo, old.n_views
    for v in range(3):
        new.y_off[v], new.x_off[v] = old.y_off[v], old.x_off[v]
    out = []
    for d, entry in ((new, "pv_video_views"), (old, "pv_resample_crop")):
        d.item0, d.n_items = item0, n_items
        if affine:
            d.ch_scale, d.ch_shift = keep[0].data_ptr(), keep[1].data_ptr()
        dst, cl = _destination(form, dtype, n + extra, old.C, t, crop)
        _set_destination(d, dst, cl, dtype, t, crop)
        call(entry, d)
        out.append(dst)
    return out[0], out[1], n


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


FORMS = [("c4", torch.bfloat16), ("cl8", torch.bfloat16), ("cl8", torch.float32), ("cl8_ld16", torch.bfloat16), ("cl16", torch.float32),
         ("planar", torch.bfloat16), ("planar", torch.float32)]
SOURCES = [("NCTHW", torch.uint8), ("NCTHW", torch.float32), ("NTHWC", torch.uint8)]
# overlapping clips, frames repeated inside a clip, a clip running backwards, the first and the last frame of the video
TABLE = torch.tensor([[0, 2, 4], [3, 4, 5], [5, 5, 11], [11, 10, 0], [7, 7, 7]], dtype=torch.int32)


@pytest.mark.parametrize("form,dtype", FORMS, ids=["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS])
@pytest.mark.parametrize("layout,src_dtype", SOURCES, ids=["planar_u8", "planar_f32", "interleaved_u8"])
def test_video_views_writes_the_bits_of_resample_crop_on_materialised_clips(layout, src_dtype, form, dtype):
    """Every destination form x source layout x source dtype; 3 views and 1 view; the whole sequence and windows that start
    and end in the middle of a clip; the items behind the window keep the sentinel."""
    src = _source(_video(12, 97, 131, 900), layout, src_dtype)
    for idxs, windows in (((0, 1, 2), ((0, 0), (1, 4), (5, 9), (14, 1))), ((2,), ((0, 0), (1, 3), (4, 1)))):
        for item0, n_items in windows:
            new, old, n = _both(src, layout, TABLE, 5, 64, 56, idxs, form, dtype, item0, n_items)
            what = "%s %s -> %s %s views %s items [%d, +%d)" % (layout, src_dtype, form, dtype, idxs, item0, n_items)
            assert _same_bits(new, old), what
            assert torch.all(new[n:] == SENTINEL), "items behind the window were written: " + what
            assert not torch.all(new[:n] == SENTINEL), what


@pytest.mark.parametrize("hs,ws,n", [(128, 171, 9), (720, 1280, 6)], ids=["odd_171_upscale", "720p"])
def test_video_views_at_full_geometry(hs, ws, n):
    """Short side to 256, 224 crops: an odd row length (no source row is 16-byte aligned) that is upscaled, and a 720p video."""
    video = _video(n, hs, ws, 901 + hs)
    table = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5], [n - 1, n - 1, 0, n - 2]], dtype=torch.int32)
    for layout, src_dtype in SOURCES:
        src = _source(video, layout, src_dtype)
        for form, dtype in (("c4", torch.bfloat16), ("planar", torch.bfloat16), ("cl8", torch.float32)):
            for idxs, item0, n_items in (((0, 1, 2), 0, 0), ((0, 1, 2), 2, 5), ((1,), 1, 2)):
                new, old, cnt = _both(src, layout, table, 4, 256, 224, idxs, form, dtype, item0, n_items, extra=1)
                assert _same_bits(new, old), (layout, src_dtype, form, dtype, idxs, item0, n_items)
                assert torch.all(new[cnt:] == SENTINEL)


def test_video_views_without_the_affine_map_and_with_a_tight_table():
    """No ch_scale / ch_shift, row stride == T."""
    src = _source(_video(12, 49, 67, 903), "NCTHW", torch.float32)
    new, old, n = _both(src, "NCTHW", TABLE, 3, 32, 28, (0, 2), "planar", torch.float32, 3, 4, affine=False)
    assert _same_bits(new, old) and torch.all(new[n:] == SENTINEL)


# ----------------------------------------------------------------------------- models
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)


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
    return _video(n, hs, ws, seed).permute(1, 2, 3, 0).contiguous().cuda()


def _composed(dep, video, table, batch, short_side, crop, views, frame_ratios=None, method="sum"):
    """The existing pieces: clips materialised by index_select, `DevicePacker.__call__` on `batch // n_views` clips at a
    time (the last batch padded with clips that are never folded), `VideoEnsembler`.  (video scores, clip scores, rows)."""
    n_clips, n_views = table.shape[0], len(views)
    assert batch % n_views == 0
    per = batch // n_views
    packer = TR.DevicePacker(dep, frame_ratios=frame_ratios, short_side=short_side, crop_size=crop, spatial_idx=views,
                             src_layout="NTHWC", **KW)
    clips = _materialise(video, "NTHWC", table)
    ve = ce = None
    for c0 in range(0, n_clips, per):
        chunk = clips[c0:c0 + per]
        k = chunk.shape[0]
        if k < per:
            chunk = torch.cat([chunk, torch.full((per - k,) + tuple(chunk.shape[1:]), 200, dtype=chunk.dtype, device=chunk.device)])
        logits = packer(chunk)[:k * n_views].clone()
        if ve is None:
            ve, ce = VideoEnsembler(1, logits.shape[1], method), VideoEnsembler(n_clips, logits.shape[1], method)
        ve.update(logits, [0] * (k * n_views))
        ce.update(logits, [c0 + i // n_views for i in range(k * n_views)])
    return ve.result()[0].clone(), ce.result().clone(), int(ve.counts.item())


def _check_predictor(dep, sampler, video, fps, batch, short_side, crop, views, frame_ratios=None, method="sum", clip_frames=None):
    pred = VideoPredictor(dep, sampler, short_side=short_side, crop_size=crop, spatial_idx=views, frame_ratios=frame_ratios,
                          method=method, **KW)
    assert pred.packer.batch == batch
    table, infos = D.clip_frame_table(sampler, video.shape[0], fps, pred.packer.clip_frames)
    if clip_frames is not None:
        assert pred.packer.clip_frames == clip_frames
    n_clips, n_views = table.shape[0], len(views)
    scores, clip_scores = pred(video, fps, return_clip_scores=True)
    scores, clip_scores = scores.clone(), clip_scores.clone()
    # the tail hides nothing: exactly n_clips * n_views rows were folded, n_views into every clip
    assert int(pred.video_ensembler.counts.item()) == n_clips * n_views
    assert pred.clip_ensembler.counts.tolist() == [n_views] * n_clips
    want, want_clips, rows = _composed(dep, video, table, batch, short_side, crop, views, frame_ratios, method)
    assert rows == n_clips * n_views
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (want.shape[0],)
    assert tuple(clip_scores.shape) == (n_clips, want.shape[0])
    assert torch.equal(scores, want), "video scores differ by %.3e" % (scores - want).abs().max().item()
    assert torch.equal(clip_scores, want_clips), "clip scores differ by %.3e" % (clip_scores - want_clips).abs().max().item()
    assert torch.equal(pred(video, fps), scores)                 # without the clip scores: the same video scores
    if n_clips > 1:
        assert not torch.equal(clip_scores[0], clip_scores[-1])  # the clips are different frames
    return pred, scores, n_clips


@pytest.fixture(scope="module")
def x3d6():
    return _x3d(6)


def test_predictor_x3d_exact_multiple_ragged_tail_and_short_video(x3d6):
    """x3d_xs, batch 6 = 2 clips x 3 views, bf16 (the stem reads the packer's own NCDHW clip), a 180 x 240 video at 10 fps,
    clips of 8 frames subsampled to 4."""
    assert x3d6._pv_inputs.src_slot is not None and x3d6._pv_inputs.c4_readers == 0
    video = _nthwc_video(24, 180, 240, 910)
    clip = Fraction(8, 10)
    _, s4, n = _check_predictor(x3d6, D.ConstantClipsPerVideoSampler(clip, 4, 3), video, 10, 6, 176, 160, (0, 1, 2), clip_frames=4)
    assert n == 4                                                # 12 items: two full forwards
    _, s5, n = _check_predictor(x3d6, D.ConstantClipsPerVideoSampler(clip, 5), video, 10, 6, 176, 160, (0, 1, 2))
    assert n == 5 and not torch.equal(s4, s5)                    # 15 items: 6 + 6 + 3
    _, _, n = _check_predictor(x3d6, D.UniformClipSampler(clip, Fraction(3, 10), True), video, 10, 6, 176, 160, (0, 1, 2), method="max")
    assert n == 7                                                # overlapping clips, the last one back-padded; 21 items
    _, _, n = _check_predictor(x3d6, D.UniformClipSampler(clip), video[:3], 10, 6, 176, 160, (0, 1, 2))
    assert n == 1                                                # a video shorter than one clip: 3 items, frames repeated
    _, _, n = _check_predictor(x3d6, D.UniformClipSampler(clip), video[:17], 10, 6, 176, 160, (2, 0))
    assert n == 2                                                # two views: 4 of 6 items


def test_predictor_does_not_depend_on_what_ran_before(x3d6):
    """A long video, then a short one on the same predictor: the short one's scores are those of a predictor on a freshly
    converted deploy form that has never seen another video."""
    video = _nthwc_video(24, 180, 240, 911)
    sampler = D.UniformClipSampler(Fraction(8, 10))
    pred = VideoPredictor(x3d6, sampler, short_side=176, crop_size=160, **KW)
    long_scores = pred(video, 10).clone()
    assert int(pred.video_ensembler.counts.item()) == 9          # 3 clips x 3 views
    short, short_clips = pred(video[:5], 10, return_clip_scores=True)
    assert int(pred.video_ensembler.counts.item()) == 3
    fresh = VideoPredictor(_x3d(6), D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, **KW)
    want, want_clips = fresh(video[:5], 10, return_clip_scores=True)
    assert torch.equal(short, want) and torch.equal(short_clips, want_clips)
    assert not torch.equal(short, long_scores)


def _input_items(packer):
    """[B, elements] view of the buffer the forward reads for pathway 0: the packer's own NCDHW clip, or the arena buffer."""
    if packer._planar:
        return packer._planar[0].view(packer._planar[0].shape[0], -1)
    ref, sess = packer.refs[0], packer.sess
    return sess.arena_t[ref.off: ref.off + ref.B * ref.bs * ref.itemsize].view(ref.B, -1)


def test_a_short_chunk_zeroes_the_unwritten_tail_of_the_input_buffers(x3d6):
    """After a full chunk every item of the input buffer holds pixels; a short chunk then leaves items [n:] all zero --
    on the planar-stem path (bf16), in the arena's channels-last buffer (fp32), and in a sub-plan that gets no item."""
    video = _nthwc_video(24, 180, 240, 918)
    table, _ = D.clip_frame_table(D.UniformClipSampler(Fraction(8, 10)), 24, 10, 4)      # 3 clips x 3 views = 9 items
    for dep, planar in ((x3d6, True), (_x3d(6, dtype=torch.float32), False)):
        packer = TR.DevicePacker(dep, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
        tables = packer.video_tables(table, 24)
        packer.fill_video(video, tables, 0, 6)
        assert bool(packer._planar) == planar
        full = _input_items(packer).clone()
        assert all(bool((full[i] != 0).any()) for i in range(6))
        packer.fill_video(video, tables, 6, 3)
        short = _input_items(packer)
        assert all(bool((short[i] != 0).any()) for i in range(3))
        assert not bool((short[3:] != 0).any()), "items [3:] of a 3-item chunk must be zero"
        packer.fill_video(video, tables, 3, 3)                   # the same window of a full chunk's items: the same bytes
        assert torch.equal(_input_items(packer)[:3], full[3:6])
    split = _x3d(6, streams=2)
    packer = TR.DevicePacker(split, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
    tables = packer.video_tables(table, 24)
    packer.fill_video(video, tables, 0, 6)
    assert all(bool((_input_items(s)[i] != 0).any()) for s in packer.subs for i in range(3))
    packer.fill_video(video, tables, 7, 2)                       # 2 items: two of the first sub-plan's three, none of the second's
    first, second = [_input_items(s) for s in packer.subs]
    assert bool((first[0] != 0).any()) and bool((first[1] != 0).any())
    assert not bool((first[2:] != 0).any()) and not bool((second != 0).any())


def test_predictor_on_a_split_batch_deploy_form():
    """streams=2: sub-plans of 3 + 3 items; 5 clips x 2 views = 10 items = 6 + 4, so the last forward fills the first
    sub-plan and one item of the second; then 3 views x 3 clips = 9 = 6 + 3, where the second sub-plan gets nothing."""
    dep = _x3d(6, streams=2)
    assert list(dep._splits) == [3, 3]
    video = _nthwc_video(24, 180, 240, 912)
    _, _, n = _check_predictor(dep, D.ConstantClipsPerVideoSampler(Fraction(8, 10), 5), video, 10, 6, 176, 160, (0, 2))
    assert n == 5
    _, _, n = _check_predictor(dep, D.UniformClipSampler(Fraction(8, 10)), video, 10, 6, 176, 160, (0, 1, 2))
    assert n == 3


def test_predictor_on_the_fp32_plan():
    """fp32 session: the ingest writes the arena's channels-last buffer, whose tail is zeroed for the ragged chunk."""
    dep = _x3d(6, dtype=torch.float32)
    video = _nthwc_video(24, 180, 240, 913)
    pred, _, n = _check_predictor(dep, D.ConstantClipsPerVideoSampler(Fraction(8, 10), 3), video, 10, 6, 176, 160, (0, 1, 2))
    assert n == 3 and not pred.packer._planar


def test_predictor_slowfast_reads_both_pathways_through_column_subsets_of_one_table():
    """slowfast_r50_small (4 + 16 frames at 96 x 96), frame_ratios (4, 1), batch 4 = 2 clips x 2 views, a portrait
    131 x 113 video: 3 clips of 24 frames -> 6 items = 4 + 2."""
    from oracle.weights import deterministic_fill, seeded_input
    from pytorchvideo_amd.models import create_slowfast
    g = torch.load(os.path.join(GOLD, "slowfast_r50_small.pt"), weights_only=False)
    m = deterministic_fill(create_slowfast(**g["cfg"]), g["seed"]).eval()
    fast = seeded_input((4, 3, 16, 96, 96), 7)
    dep = _deploy(m, [TR.uniform_temporal_subsample(fast, 4, 2), fast])
    video = _nthwc_video(40, 131, 113, 914)
    _, _, n = _check_predictor(dep, D.ConstantClipsPerVideoSampler(Fraction(24, 20), 3, 2), video, 20, 4, 100, 96, (0, 2),
                               frame_ratios=(4, 1), clip_frames=16)
    assert n == 3


def test_predictor_mvit():
    """mvit_b_small (4 x 64 x 64, 16 classes), batch 6 = 2 clips x 3 views; 3 clips -> 9 items = 6 + 3."""
    from oracle.weights import deterministic_fill, seeded_input
    from pytorchvideo_amd.models import create_multiscale_vision_transformers
    g = torch.load(os.path.join(GOLD, "mvit_b_small.pt"), weights_only=False)
    m = deterministic_fill(create_multiscale_vision_transformers(**g["cfg"]), g["seed"]).eval()
    dep = _deploy(m, seeded_input((6, 3, 4, 64, 64), 8))
    video = _nthwc_video(20, 75, 101, 915)
    _, _, n = _check_predictor(dep, D.UniformClipSampler(Fraction(6, 10)), video, 10, 6, 70, 64, (0, 1, 2), clip_frames=4)
    assert n == 3


def test_predictor_refuses_what_it_cannot_score(x3d6):
    """Errors before any launch: a detection model, a table that leaves the video, a chunk that leaves the sequence."""
    from oracle.weights import detection_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    g = torch.load(os.path.join(GOLD, "resnet_det_r50_small.pt"), weights_only=False)
    m = detection_fill(create_resnet_with_roi_head(**g["cfg"]), g["seed"]).eval()
    transmute_model(m, "mi355x")
    x = SU.normalised(SU.clip((3, 4, 64, 64), 916))[None].repeat(2, 1, 1, 1, 1)
    dm = convert_to_deployable_form(m, (x.cuda().bfloat16(), g["boxes"]), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="detection"):
        VideoPredictor(dm, D.UniformClipSampler(1), short_side=72, crop_size=64, **KW)
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
    video = _nthwc_video(8, 180, 240, 917)
    table = torch.tensor([[0, 2, 4, 8]])
    with pytest.raises(ValueError):
        packer.video_tables(table, 8)                            # frame 8 of an 8-frame video
    tables = packer.video_tables(torch.tensor([[0, 2, 4, 7]]), 8)
    for i0, n in ((0, 4), (3, 1), (0, 0), (0, 7)):               # 1 clip x 3 views
        with pytest.raises(RuntimeError):
            packer.fill_video(video, tables, i0, n)
    with pytest.raises(RuntimeError):
        packer.fill_video(video.cpu(), tables, 0, 3)
    with pytest.raises(RuntimeError):
        TR.DevicePacker(x3d6, **KW).fill_video(video, tables, 0, 3)   # no resampling geometry
