"""Rotated and mirrored videos read in place on the MI355X: `pv_view_source.orient` through `pv_batch_views`,
`pv_frame_views` and `pv_box_views` (include/pv_mi355x.h), `DevicePacker.video_batch(..., orientation=)` and the predictors
of `inference`.

Reference, bit for bit (`torch.equal` on the raw bits, no tolerance): THE SAME LAUNCH with orient = 0 on a dense copy of the
video that was oriented beforehand (`torch.rot90` / `flip`; YUV: the Y, U and V planes oriented separately and repacked at
pitch W, tests/orient_util.py) -- the header's own statement of what an oriented record holds.  The upright kernels that
write the reference are the ones the existing suite holds against the reference's fixtures.  Boxes are compared with the host
mirror `transforms.boxes_to_view(..., orientation=)`, which tests/test_orient_ingest.py holds against the reference."""
import collections
from fractions import Fraction

import pytest
import torch

import orient_util as OU
import spatial_util as SU
import test_gpu_batch_views as BV
import test_gpu_frame_views as FV
import test_gpu_keyframe_detection as KD
import yuv16_util as Y16
import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import KeyframeDetector, StreamPredictor, VideoBatchPredictor, VideoPredictor

pytestmark = pytest.mark.gpu
KW = BV.KW
SENTINEL = BV.SENTINEL
TURNED = (1, 2, 3, 4, 5, 6, 7)
# what one launch reads a video as: the RGB / planar forms by (layout, dtype), the YUV forms by name
RGB_FORMS = {"nthwc_u8": ("NTHWC", torch.uint8), "ncthw_u8": ("NCTHW", torch.uint8), "ncthw_f32": ("NCTHW", torch.float32)}
YUV_FORMS = ("NV12", "I420", "P010", "I010")
ALL_FORMS = tuple(RGB_FORMS) + YUV_FORMS
MATRIX = {"NV12": TR.yuv_matrix("bt601", False), "I420": TR.yuv_matrix("bt601", False),
          "P010": TR.yuv_matrix("bt709", True, 10, True), "I010": TR.yuv_matrix("bt2020", False, 10)}
# T = 2 out of 3 frames: a row that repeats a frame and one that runs backwards
TABLES = torch.tensor([[2, 2], [1, 0]], dtype=torch.int32)

Src = collections.namedtuple("Src", "tensor n hs ws geom")       # geom: transforms.yuv_geometry, or None


# ----------------------------------------------------------------------------- sources and their pre-oriented copies
def _stored_and_turned(form, n, hs, ws, seed, codes, pitch=None, coded=None):
    """(stored source, {code: pre-oriented dense source}) of one seeded video in `form`, on the device."""
    if form in RGB_FORMS:
        layout, dtype = RGB_FORMS[form]
        video = SU.clip((3, n, hs, ws), seed)                    # uint8 [3, N, H, W]
        make = lambda v: Src(BV._source(v, layout, dtype), n, v.shape[2], v.shape[3], None)     # noqa: E731
        return make(video), {c: make(OU.turned(video, c)) for c in codes}
    wide = form in TR.YUV16_LAYOUTS
    util = Y16 if wide else YU
    planes = Y16.planes(n, hs, ws, seed, shift=6 if form == "P010" else 0) if wide else YU.planes(n, hs, ws, seed)

    def make(frames, **kw):
        g = TR.yuv_geometry(frames, form, **kw)
        return Src(frames, g["N"], g["Hs"], g["Ws"], g)

    packed = util.pack(*planes, form, coded_height=coded, pitch=pitch, base=2 if wide else 3, garbage=11)
    stored = make(packed.frames("cuda"), **(dict(coded_height=coded, height=hs) if coded else {}))
    assert (stored.hs, stored.ws) == (hs, ws)
    return stored, {c: make(OU.yuv_preoriented(*planes, form, c).frames("cuda")) for c in codes}


def _record(rec, src, orient, size, window, idxs, ptr=None, scaled=None):
    """The record of `src` under `orient`: stored sizes and planes, the views cut from the DISPLAYED frame -- short side to
    `size` (or the explicit `scaled` = (Hn, Wn)), then the `window` crop of every view, or (a pair) no crop."""
    hd, wd = OU.displayed_size(src.hs, src.ws, orient)
    hn, wn = scaled or TR.scaled_size(hd, wd, size)
    rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn = (src.tensor.data_ptr() if ptr is None else ptr), src.n, src.hs, src.ws, hn, wn
    rec.sy, rec.sx = BV._f32(hd, hn), BV._f32(wd, wn)
    rec.orient = orient
    for k, v in enumerate(idxs):
        if isinstance(window, int):
            assert window <= hn and window <= wn
            rec.y_off[k], rec.x_off[k] = TR.crop_offsets(hn, wn, window, v)
        else:
            assert tuple(window) == (hn, wn)
    for k in ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch") if src.geom else ():
        setattr(rec, k, src.geom[k])


def _form_fields(d, form, srcs, keep):
    if form in RGB_FORMS:
        layout, dtype = RGB_FORMS[form]
        d.src_layout = L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC
        d.src_dtype = L.PV_U8 if dtype == torch.uint8 else L.PV_F32
        return
    keep.append(MATRIX[form].float().reshape(12).cuda())
    d.src_layout, d.src_dtype = L.SRC_YUV420, (L.PV_U16 if form in TR.YUV16_LAYOUTS else L.PV_U8)
    d.c_step, d.yuv2rgb = srcs[0].geom["c_step"], keep[-1].data_ptr()


def _destination(dst_form, dtype, n, t, ho, wo):
    if dst_form == "planar":
        return torch.full((n, 3, t, ho, wo), SENTINEL, dtype=dtype, device="cuda"), None
    c_p, ld = {"c4": (4, 4), "cl8": (8, 8)}[dst_form]
    return torch.full((n, t, ho, wo, ld), SENTINEL, dtype=dtype, device="cuda"), (c_p, ld)


def _launch(form, srcs, orients, size, window, idxs, triples, dst=("c4", torch.bfloat16), tables=None, scaled=None):
    """pv_batch_views over `srcs` (record j under orients[j]) for the items `triples` = (source, clip, view); every source
    reads the same `tables`.  Returns the destination with two sentinel items behind the launch."""
    from gpu_util import call
    tables = [TABLES] * len(srcs) if tables is None else tables
    sources = (L.ViewSource * len(srcs))()
    for rec, src, code in zip(sources, srcs, orients):
        _record(rec, src, code, size, window, idxs, scaled=scaled)
    tab, row0 = BV._concat_tables(tables, 3)
    t = tables[0].shape[1]
    ho, wo = (window, window) if isinstance(window, int) else window
    keep = []
    d = L.BatchViewsDesc()
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], 3, 3, t
    d.Ho, d.Wo, d.n_views = ho, wo, len(idxs)
    _form_fields(d, form, srcs, keep)
    items = BV._items([(s, row0[s] + r, v) for s, r, v in triples])
    keep += [BV._upload(sources), BV._upload(items)] + [x.cuda() for x in SU.affine()]
    d.sources, d.sources_dev = BV.C.addressof(sources), keep[-4].data_ptr()
    d.items, d.items_dev = BV.C.addressof(items), keep[-3].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.ch_scale, d.ch_shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    out, cl = _destination(dst[0], dst[1], len(items) + 2, t, ho, wo)
    d.dst, d.dst_dtype = out.data_ptr(), (L.PV_BF16 if dst[1] == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], t * ho * wo * cl[1]
    call("pv_batch_views", d)
    torch.cuda.synchronize()
    return out


def _every(n_sources, n_views, clips=2):
    return [(s, r, v) for s in range(n_sources) for r in range(clips) for v in range(n_views)]


def _check_codes(form, stored, turned, codes, size, window, idxs, dst=("c4", torch.bfloat16), scaled=None, tables=None):
    """One launch with a record per code on the ONE stored video against one launch of upright records on the pre-oriented
    copies: every item, the sentinel behind."""
    clips = TABLES.shape[0] if tables is None else tables[0].shape[0]
    triples = _every(len(codes), len(idxs), clips)
    got = _launch(form, [stored] * len(codes), codes, size, window, idxs, triples, dst, tables, scaled)
    want = _launch(form, [turned[c] for c in codes], [0] * len(codes), size, window, idxs, triples, dst, tables, scaled)
    for i, (s, r, v) in enumerate(triples):
        assert BV._same_bits(got[i], want[i]), "%s -> %s %s: code %d clip %d view %d" % (form, dst[0], dst[1], codes[s], r, v)
    assert not torch.all(got[:len(triples)] == SENTINEL)
    assert torch.all(got[len(triples):] == SENTINEL) and torch.all(want[len(triples):] == SENTINEL)
    assert not BV._same_bits(got[0], got[len(idxs) * clips])     # two codes do show different pictures
    return got


# ----------------------------------------------------------------------------- kernel: every code x every source form
@pytest.mark.parametrize("regime", ["downscale", "upscale"])
@pytest.mark.parametrize("form", ALL_FORMS)
def test_every_code_writes_the_bits_of_the_preoriented_copy(form, regime):
    """Codes 1..7 in one launch.  downscale: stored 45 x 71 (YUV: 46 x 70 at pitch 80, coded height 48, an unaligned base), short
    side 24, crop 24 -- the strips' paired-rows regime; upscale: stored 20 x 30 (YUV: pitch 40, coded 24), short side 32, crop
    32 -- the dense one.  Three views, T = 2, the 4-channel bf16 destination."""
    yuv = form in YUV_FORMS
    if regime == "downscale":
        (hs, ws), size, crop, geo = ((46, 70) if yuv else (45, 71)), 24, 24, dict(pitch=80, coded=48)
    else:
        (hs, ws), size, crop, geo = (20, 30), 32, 32, dict(pitch=40, coded=24)
    stored, turned = _stored_and_turned(form, 3, hs, ws, 1700, TURNED, **(geo if yuv else {}))
    _check_codes(form, stored, turned, TURNED, size, crop, (0, 1, 2))


@pytest.mark.parametrize("dst", [("planar", torch.bfloat16), ("planar", torch.float32), ("cl8", torch.bfloat16)],
                         ids=["planar_bf16", "planar_f32", "cl8_bf16"])
@pytest.mark.parametrize("form", ["nthwc_u8", "NV12"])
def test_the_other_destination_forms(form, dst):
    """Codes 1 and 7 of one RGB and one YUV form into the planar and the channels-last destinations (G = 8, 4 and 1 pixels
    per thread); 24 is a multiple of neither 32 nor 16, so every tile row ends in a cut group."""
    (hs, ws), geo = ((46, 70), dict(pitch=80, coded=48)) if form == "NV12" else ((45, 71), {})
    stored, turned = _stored_and_turned(form, 3, hs, ws, 1710, (1, 7), **geo)
    _check_codes(form, stored, turned, (1, 7), 24, 24, (0, 1, 2), dst)
    _check_codes(form, stored, turned, (1, 7), 27, 27, (0, 2), dst)      # an odd window: no group is 16-byte aligned


@pytest.mark.parametrize("form", ["NV12", "nthwc_u8"])
def test_tile_seams(form):
    """Stored 400 x 300, codes 1 and 6, short side 160, crop 160: five tiles of 32 (ten of 16, ...) in either direction, so
    every seam between tiles lies inside the window whatever tile the launch was sized to."""
    stored, turned = _stored_and_turned(form, 2, 400, 300, 1720, (1, 6))
    tables = [torch.tensor([[1, 0]], dtype=torch.int32)] * 2
    _check_codes(form, stored, turned, (1, 6), 160, 160, (0, 1, 2), tables=tables)


@pytest.mark.parametrize("form", ["NV12", "nthwc_u8"])
def test_no_crop_into_a_rectangular_window(form):
    """A stored 64 x 36 frame under code 3 is displayed 36 x 64 and written whole into a 64 x 36 window (Hn x Wn = 64 x 36, no
    crop: rows upscaled, columns downscaled), beside code 5."""
    stored, turned = _stored_and_turned(form, 3, 64, 36, 1730, (3, 5))
    _check_codes(form, stored, turned, (3, 5), None, (64, 36), (1,), scaled=(64, 36))


@pytest.mark.parametrize("dst", [("c4", torch.bfloat16), ("planar", torch.float32)], ids=["c4", "planar_f32"])
@pytest.mark.parametrize("form", ["nthwc_u8", "NV12"])
def test_one_launch_mixes_orientations(form, dst):
    """Five items over five sources of codes 0, 1, 4, 7, 0 and different sizes: an upright run, an oriented run, an upright
    run.  Every item equals the item of its one-video launch -- for the two upright ones that is the launch of a record whose
    field was left 0, the strips as they always ran."""
    codes = (0, 1, 4, 7, 0)
    sizes = ((46, 70), (40, 52), (34, 48), (50, 38), (30, 62)) if form == "NV12" else ((45, 71), (40, 52), (33, 47), (50, 38), (29, 61))
    srcs = [_stored_and_turned(form, 3, h, w, 1740 + j, ())[0] for j, (h, w) in enumerate(sizes)]
    triples = [(0, 0, 0), (1, 1, 2), (2, 0, 1), (3, 1, 0), (4, 0, 2)]
    got = _launch(form, srcs, codes, 24, 24, (0, 1, 2), triples, dst)
    for i, (s, r, v) in enumerate(triples):
        alone = _launch(form, [srcs[s]], [codes[s]], 24, 24, (0, 1, 2), [(0, r, v)], dst)
        assert BV._same_bits(got[i], alone[0]), "%s %s: item %d, code %d" % (form, dst[0], i, codes[s])
        assert torch.all(alone[1:] == SENTINEL)
    assert torch.all(got[5:] == SENTINEL) and not any(bool(torch.all(got[i] == SENTINEL)) for i in range(5))
    # the oriented items against the pre-oriented copies too
    for i in (1, 2, 3):
        s, r, v = triples[i]
        turned = _stored_and_turned(form, 3, *sizes[s], 1740 + s, (codes[s],))[1][codes[s]]
        want = _launch(form, [turned], [0], 24, 24, (0, 1, 2), [(0, r, v)], dst)
        assert BV._same_bits(got[i], want[0]), (form, dst[0], i)


def test_frame_views_reads_turned_surfaces_where_they_lie():
    """pv_frame_views under code 3: pitched NV12 surfaces (46 x 70 at pitch 80, coded height 48), each its own allocation at an
    odd address, against pv_batch_views on the pre-oriented dense copy."""
    planes = YU.planes(5, 46, 70, 1750)
    packed = YU.pack(*planes, "NV12", coded_height=48, pitch=80, garbage=5).frames()
    lists = [FV._own_surfaces(packed, 1751)]
    assert all(f.stride(0) == 80 and f.data_ptr() % 2 == 1 for f in lists[0])
    geom = TR.yuv_geometry(lists[0][0][None], "NV12", coded_height=48, height=46)
    matrix = MATRIX["NV12"].float().reshape(12).cuda()
    tables = [torch.tensor([[4, 4, 0], [3, 2, 1]], dtype=torch.int32)]
    triples = _every(1, 3)

    def fill_record(rec, own, slice_ptr):
        _record(rec, Src(None, len(own), 46, 70, geom), 3, 24, 24, (0, 1, 2), ptr=slice_ptr)

    def fill_desc(d):
        d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U8, L.SRC_YUV420, geom["c_step"], matrix.data_ptr()

    turned = OU.yuv_preoriented(*planes, "NV12", 3).frames("cuda")
    g = TR.yuv_geometry(turned, "NV12")
    for form, dtype in (("c4", torch.bfloat16), ("planar", torch.bfloat16)):
        got = FV._launch_frames(lists, fill_record, fill_desc, tables, 3, (0, 1, 2), triples, form, dtype, 24)
        want = _launch("NV12", [Src(turned, g["N"], g["Hs"], g["Ws"], g)], [0], 24, 24, (0, 1, 2), triples, (form, dtype), tables)
        for i in range(len(triples)):
            assert BV._same_bits(got[i], want[i]), (form, i)
        assert torch.all(got[len(triples):] == SENTINEL) and not torch.all(got[:len(triples)] == SENTINEL)


# ----------------------------------------------------------------------------- boxes
@pytest.mark.parametrize("clip", [False, True], ids=["as_given", "clip_to_source"])
def test_box_views_maps_stored_boxes_into_the_displayed_view(clip):
    """Eight 60 x 90 sources, one per code, three views each; 9 boxes per item (inside, fractional, partly outside on every
    side, wholly outside, negative, on and past the border) against boxes_to_view(..., orientation=) bit for bit; the rows
    behind the launch are {-1, 0, 0, 0, 0}."""
    from gpu_util import call
    videos = [torch.zeros(2, 60, 90, 3, dtype=torch.uint8, device="cuda") for _ in range(8)]
    tables = [torch.zeros(1, 4, dtype=torch.int32)] * 8
    batch = TR.build_video_batch(videos, tables, "NTHWC", 56, 48, (0, 1, 2), [4], 3, torch.device("cuda"), lambda t: t.cuda(),
                                 orientation=list(OU.CODES))
    nine = KD.box_set(60, 90)[:9]
    assert bool((nine < 0).any()) and bool((nine[:, 2] > 89).any())
    boxes = nine.repeat(batch.total, 1)
    box_item = torch.arange(batch.total, dtype=torch.int32).repeat_interleave(9)
    n, capacity = boxes.shape[0], 256
    assert batch.total == 24 and n == 216
    boxes_d, item_d = boxes.cuda(), box_item.cuda()
    dst = torch.full((capacity + 2, 5), 7.0, device="cuda")
    d = L.BoxViewsDesc()
    d.boxes, d.box_item, d.dst = boxes_d.data_ptr(), item_d.data_ptr(), dst.data_ptr()
    d.sources_dev, d.items_dev = batch.sources_dev.data_ptr(), batch.items_dev.data_ptr()
    d.n_boxes, d.n_seq, d.n_sources, d.n_views = n, batch.total, 8, 3
    d.box0, d.n_launch, d.item0, d.n_items = 0, n, 0, batch.total
    d.Ho, d.Wo, d.capacity, d.clip_to_source = 48, 48, capacity, int(clip)
    call("pv_box_views", d)
    got = dst.cpu()
    for i in range(batch.total):
        code, _, view, _ = batch.item_rows[i].tolist()
        want = TR.boxes_to_view(nine, 60, 90, 56, 48, view, clip, orientation=code)
        rows = got[9 * i: 9 * i + 9]
        assert torch.equal(rows[:, 0], torch.full((9,), float(i))) and torch.equal(rows[:, 1:], want), (code, view)
        assert bool((rows[:, 1] <= rows[:, 3]).all()) and bool((rows[:, 2] <= rows[:, 4]).all())
    assert torch.equal(got[n:capacity], torch.tensor([-1.0, 0, 0, 0, 0]).repeat(capacity - n, 1))
    assert bool((got[capacity:] == 7.0).all())
    views = {c: got[9 * 3 * c: 9 * 3 * c + 27, 1:] for c in OU.CODES}
    assert not torch.equal(views[0], views[4]) and not torch.equal(views[1], views[3])


# ----------------------------------------------------------------------------- the whole path
@pytest.fixture(scope="module")
def x3d6():
    return BV._x3d(6)


def _turned_video(video, code):
    """The dense pre-oriented copy of a [N, H, W, 3] device video."""
    return TR.oriented(video, code, 1, 2).contiguous()


def test_video_predictor_scores_a_stored_portrait_clip(x3d6):
    """A phone clip recorded upright: stored 180 x 240, "rotate 90"."""
    video = BV._nthwc_video(23, 180, 240, 1760)
    pred = VideoPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10), Fraction(3, 10)), short_side=176, crop_size=160, **KW)
    want, want_clips = pred(_turned_video(video, 1), 10, return_clip_scores=True)
    want, want_clips = want.clone(), want_clips.clone()
    lying = pred(video, 10).clone()
    got, got_clips = pred(video, 10, return_clip_scores=True, orientation=TR.orientation_code(90))
    assert tuple(got_clips.shape) == (6, 400) and torch.equal(got, want) and torch.equal(got_clips, want_clips)
    assert not torch.equal(got, lying)                           # scored lying on its side it is another answer
    assert torch.equal(pred(TR.FrameList(list(video.unbind(0))), 10, orientation=1), want)
    assert torch.equal(pred(video, 10, orientation=0), lying)


def test_batch_predictor_takes_a_code_per_video(x3d6):
    codes = [0, 3, 5]
    videos = [BV._nthwc_video(n, 180, 240, 1770 + n) for n in (24, 5, 17)]
    pred = VideoBatchPredictor(x3d6, D.UniformClipSampler(Fraction(8, 10)), short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)
    want, want_clips = pred([_turned_video(v, c) for v, c in zip(videos, codes)], 10, return_clip_scores=True)
    want, want_clips = want.clone(), [c.clone() for c in want_clips]
    got, got_clips = pred(videos, 10, return_clip_scores=True, orientation=codes)
    assert pred.forwards == 3 and pred.video_ensembler.counts.tolist() == [9, 3, 6]
    assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(got_clips, want_clips))
    assert not torch.equal(got[1], pred(videos, 10)[1])


def test_keyframe_detector_takes_stored_boxes_of_a_mirrored_video():
    """Code 4 on the small detection form: the scores of the flipped video with the flipped boxes."""
    dm = KD._form("resnet_det_r50_small", torch.bfloat16, 48, 48)[0]
    box_list = KD._split(KD.box_set(60, 90), KD.COUNTS)
    video = KD._video(40, 60, 90, 4300).cuda()
    det = KeyframeDetector(dm, KD.DURATION, short_side=56, crop_size=48, spatial_idx=2, **KW)
    want = det(_turned_video(video, 4), KD.FPS, KD.STAMPS, [TR.orient_boxes(b, 60, 90, 4) for b in box_list]).clone()
    plain = det(video, KD.FPS, KD.STAMPS, box_list).clone()
    got = det(video, KD.FPS, KD.STAMPS, box_list, orientation=4)
    assert tuple(got.shape) == (sum(KD.COUNTS), 16) and torch.equal(got, want) and not torch.equal(got, plain)


def test_stream_predictor_has_one_orientation(x3d6):
    dur, stride = Fraction(8, 10), Fraction(3, 10)
    video = BV._nthwc_video(23, 180, 240, 1780)
    pred = VideoPredictor(x3d6, D.UniformClipSampler(dur, stride), short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)
    clip_scores = pred(_turned_video(video, 2), 10, return_clip_scores=True)[1].clone()
    sp = StreamPredictor(x3d6, dur, stride, 10, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), orientation=2, **KW)
    out = sp.push(list(video[:12].unbind(0))) + sp.push(list(video[12:].unbind(0)))
    assert [k for k, _, _ in out] == list(range(6))
    for k, _, scores in out:
        assert torch.equal(scores, clip_scores[k]), k


def test_the_clip_at_a_time_call_names_video_batch(x3d6):
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
    with pytest.raises(RuntimeError, match="video_batch"):
        packer(torch.zeros((2, 4, 180, 240, 3), dtype=torch.uint8), orientation=1)
