"""Packed pixels on the MI355X (include/pv_mi355x.h "packed pixels"): `pv_batch_views`, `pv_frame_views`, `pv_region_views` and
`pv_area_views` on BGR / RGBA / BGRA / ARGB / ABGR surfaces read where they lie.

Reference, bit for bit (`torch.equal`, no tolerance -- the guarantee is bit equality and the reference is the existing path):
the SAME entry point with `PV_SRC_NTHWC` on `packed_to_rgb(video).contiguous()`, the dense R, G, B copy of the same frames.
The frames are a view into a larger random buffer (tests/packed_util.py): 46 x 70, five frames, one pixel into the buffer (BGR:
two more bytes, `addr & 15` odd), a row pitch of 70 * PB + 12 (BGR: 70 * 3 + 7), so staged spans straddle 16-byte granules at
varying offsets; alpha and padding are random.  Short side 36, crop 32, views (0, 1, 2)."""
import pytest
import torch

import packed_util as PU
from pytorchvideo_amd import transforms as TR

pytestmark = pytest.mark.gpu

N, HS, WS, SHORT, CROP, VIEWS = 5, 46, 70, 36, 32, (0, 1, 2)
TABLE = torch.tensor([[0, 2, 4], [3, 3, 1]], dtype=torch.int32)              # 2 rows x 3 frames, one repeated
ITEMS = [(0, 0, 0), (0, 1, 2), (0, 0, 1), (0, 1, 0)]                          # (source, row, view): every view, both rows


def _pair(layout, n=N, h=HS, w=WS, seed=0):
    """(buffer, packed view, dense R,G,B copy) on the device."""
    buf, view = PU.surface(layout, n, h, w, 100 + seed + PU.layout_bytes(layout), "cuda")
    assert view.data_ptr() % 16 == (5 if layout == "BGR" else 4) and not view.is_contiguous()
    return buf, view, PU.dense_rgb(view, layout)


def _equal(got, want):
    return torch.equal(PU.bits(got[0]), PU.bits(want[0]))


def _check_footprint(dst, cl, n_written):
    inside, outside = PU.footprint(dst, cl, n_written)
    assert not torch.isnan(dst[inside].float()).any() and torch.isnan(dst[outside].float()).all()


# ----------------------------------------------------------------------------- 1: upright bilinear
@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("form,dtype", PU.FORMS, ids=PU.FORM_IDS)
@pytest.mark.parametrize("layout", PU.LAYOUTS)
def test_upright_items_hold_the_bits_of_the_dense_rgb_copy(layout, form, dtype, frames):
    buf, view, rgb = _pair(layout)
    kw = dict(short=SHORT, crop=CROP, idxs=VIEWS, frames=frames)
    got = PU.launch(layout, [view], TABLE, ITEMS, form, dtype, **kw)
    want = PU.launch("NTHWC", [rgb], TABLE, ITEMS, form, dtype, **kw)
    assert _equal(got, want)
    _check_footprint(got[0], got[1], len(ITEMS))                 # 5: outside the items' footprint the NaN is still there
    # 5: nothing but R, G and B enters a value -- other alpha, other padding, the same bytes out
    other = PU.scrambled(buf, layout, N, HS, WS, 7)
    assert not torch.equal(other, buf)
    again = PU.launch(layout, [PU.view_of(other, layout, N, HS, WS)], TABLE, ITEMS, form, dtype, **kw)
    assert _equal(again, got)
    # 6: an item equals the same item launched alone
    alone = PU.launch(layout, [view], TABLE, ITEMS[1:2], form, dtype, **kw)
    assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][1]))


def test_two_surfaces_of_different_sizes_share_a_launch():
    """Records with different frame sizes, pitches and alignments in one launch, items interleaved."""
    _, a, a_rgb = _pair("BGRA")
    _, b, b_rgb = _pair("BGRA", 3, 61, 39, seed=3)
    table = torch.tensor([[0, 2, 1], [2, 0, 0]], dtype=torch.int32)
    items = [(1, 0, 2), (0, 1, 0), (1, 1, 1), (0, 0, 1)]
    for form, dtype in PU.FORMS[:2]:
        kw = dict(short=SHORT, crop=CROP, idxs=VIEWS)
        assert _equal(PU.launch("BGRA", [a, b], table, items, form, dtype, **kw), PU.launch("NTHWC", [a_rgb, b_rgb], table, items, form, dtype, **kw))


# ----------------------------------------------------------------------------- 2: oriented records
@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("orient", [1, 4, 7])
@pytest.mark.parametrize("layout", ["BGR", "BGRA", "ARGB"])
def test_oriented_items_mixed_with_an_upright_record(layout, orient, frames):
    """Source 0 upright, source 1 the same surface stored turned / mirrored: strips and tiles in one call."""
    _, view, rgb = _pair(layout)
    items = [(1, 0, 0), (0, 1, 1), (1, 1, 2), (1, 0, 1), (0, 0, 2)]
    for form, dtype in (PU.FORMS[0], PU.FORMS[2], PU.FORMS[4]):
        kw = dict(short=SHORT, crop=CROP, idxs=VIEWS, frames=frames, orients=[0, orient])
        got = PU.launch(layout, [view, view], TABLE, items, form, dtype, **kw)
        want = PU.launch("NTHWC", [rgb, rgb], TABLE, items, form, dtype, **kw)
        assert _equal(got, want), (form, dtype)
        _check_footprint(got[0], got[1], len(items))
        for k in (0, 1):                                         # 6: the oriented and the upright item, each launched alone
            alone = PU.launch(layout, [view, view], TABLE, items[k:k + 1], form, dtype, **kw)
            assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][k])), (form, dtype, k)
    assert not torch.equal(got[0][0], got[0][3])                 # (the views differ: the windows are honoured)


# ----------------------------------------------------------------------------- 3: the box filter
AREA = {"46x70_to_36_crop32": (HS, WS, dict(short=SHORT, crop=CROP, idxs=VIEWS), ITEMS),
        "93x141_to_36_crop32": (93, 141, dict(short=SHORT, crop=CROP, idxs=VIEWS), ITEMS),          # ratio ~2.6: windows of 3 to 4
        "64x144_to_32x72_no_crop": (64, 144, dict(short=32, window=(32, 72), idxs=(1,)), [(0, 0, 0), (0, 1, 0)])}   # two column tiles


@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("case", list(AREA))
@pytest.mark.parametrize("layout", ["BGR", "BGRA", "ABGR"])
def test_area_items_hold_the_bits_of_the_dense_rgb_copy(layout, case, frames):
    h, w, kw, items = AREA[case]
    buf, view, rgb = _pair(layout, N, h, w)
    for form, dtype in PU.FORMS:
        got = PU.launch(layout, [view], TABLE, items, form, dtype, area=True, frames=frames, **kw)
        want = PU.launch("NTHWC", [rgb], TABLE, items, form, dtype, area=True, frames=frames, **kw)
        assert _equal(got, want), (form, dtype)
        _check_footprint(got[0], got[1], len(items))
    form, dtype = PU.FORMS[1]
    other = PU.view_of(PU.scrambled(buf, layout, N, h, w, 11), layout, N, h, w)
    full = PU.launch(layout, [view], TABLE, items, form, dtype, area=True, frames=frames, **kw)
    assert _equal(PU.launch(layout, [other], TABLE, items, form, dtype, area=True, frames=frames, **kw), full)
    alone = PU.launch(layout, [view], TABLE, items[1:2], form, dtype, area=True, frames=frames, **kw)
    assert torch.equal(PU.bits(alone[0][0]), PU.bits(full[0][1]))


@pytest.mark.parametrize("layout", ["BGR", "BGRA", "ABGR"])
def test_area_at_the_identity_geometry_is_the_bilinear_launch(layout):
    """Short side = the frame's own: every window is one pixel and every blend weight is 0 or 1."""
    _, view, _ = _pair(layout)
    kw = dict(short=HS, crop=CROP, idxs=VIEWS)
    for form, dtype in PU.FORMS[:3]:
        assert _equal(PU.launch(layout, [view], TABLE, ITEMS, form, dtype, area=True, **kw), PU.launch(layout, [view], TABLE, ITEMS, form, dtype, **kw))


# ----------------------------------------------------------------------------- 4: rectangles
@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("layout", ["BGR", "BGRA"])
def test_region_items_hold_the_bits_of_the_dense_rgb_copy(layout, frames):
    """A rectangle per destination frame with odd `left` and `top`; some touch the right and the bottom edge."""
    buf, view, rgb = _pair(layout)
    regions = torch.tensor([[[1, 3, 30, 41], [7, 29, HS - 7, WS - 29], [5, 1, 17, 23]],
                            [[HS - 21, WS - 33, 21, 33], [3, 5, 40, 60], [11, 13, 8, 9]]])          # (top, left, h, w)
    items = [(0, 1, 0), (0, 0, 0)]
    for form, dtype in PU.FORMS:
        kw = dict(window=(CROP, 40), regions=regions, frames=frames)
        got = PU.launch(layout, [view], TABLE, items, form, dtype, **kw)
        want = PU.launch("NTHWC", [rgb], TABLE, items, form, dtype, **kw)
        assert _equal(got, want), (form, dtype)
        _check_footprint(got[0], got[1], len(items))
    other = PU.view_of(PU.scrambled(buf, layout, N, HS, WS, 13), layout, N, HS, WS)
    assert _equal(PU.launch(layout, [other], TABLE, items, form, dtype, **kw), got)


# ----------------------------------------------------------------------------- the Python surface
def test_device_scale_crop_and_resized_crop_read_pitched_clips_in_place():
    for layout in ("BGR", "BGRA"):
        _, view, rgb = _pair(layout, 8)
        clips, dense = view.unflatten(0, (2, 4)), rgb.unflatten(0, (2, 4))
        assert not clips.is_contiguous()
        kw = dict(mean=PU.MEAN, std=PU.STD, div255=True, spatial_idx=VIEWS)
        for mode in ("bilinear", "area"):
            got = TR.device_scale_crop(clips, SHORT, CROP, src_layout=layout, interpolation=mode, num_frames=3, **kw)
            want = TR.device_scale_crop(dense, SHORT, CROP, src_layout="NTHWC", interpolation=mode, num_frames=3, **kw)
            assert got.shape == (6, 3, 3, CROP, CROP) and torch.equal(got, want), (layout, mode)
        regions = torch.tensor([[[1, 3, 30, 41]] * 4, [[HS - 21, WS - 33, 21, 33]] * 4])
        got = TR.device_resized_crop(clips, regions, (CROP, 40), PU.MEAN, PU.STD, True, src_layout=layout)
        assert torch.equal(got, TR.device_resized_crop(dense, regions, (CROP, 40), PU.MEAN, PU.STD, True, src_layout="NTHWC"))


# ----------------------------------------------------------------------------- 7: end to end
KW = dict(mean=PU.MEAN, std=PU.STD, div255=True)


@pytest.fixture(scope="module")
def x3d6():
    """x3d_xs (4 x 160 x 160, 400 classes) converted for 6 items: the recipe of tests/test_gpu_batch_views.py."""
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    m = trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()
    transmute_model(m, "mi355x")
    return convert_to_deployable_form(m, seeded_input((6, 3, 4, 160, 160), 6).cuda().bfloat16(), dtype=torch.bfloat16)


def _video(layout, n, h, w, seed):
    """A pitched packed video whose R and B planes differ by construction, its dense R,G,B copy and the copy with R and B
    swapped."""
    _, view, rgb = _pair(layout, n, h, w, seed)
    assert not torch.equal(rgb[..., 0], rgb[..., 2])
    return view, rgb, rgb[..., [2, 1, 0]].contiguous()


def test_video_predictor_scores_a_pitched_bgra_surface(x3d6):
    from pytorchvideo_amd import data as D
    from pytorchvideo_amd.inference import VideoPredictor
    view, rgb, swapped = _video("BGRA", 12, 180, 240, 20)
    sampler = D.UniformClipSampler(0.8)
    got = VideoPredictor(x3d6, sampler, PU.MEAN, PU.STD, True, 176, 160, src_layout="BGRA")(view, 10).clone()
    dense = VideoPredictor(x3d6, sampler, PU.MEAN, PU.STD, True, 176, 160, src_layout="NTHWC")
    want, other = dense(rgb, 10).clone(), dense(swapped, 10).clone()
    assert tuple(got.shape) == (400,) and torch.isfinite(got).all()
    assert torch.equal(got, want) and not torch.equal(got, other)
    # the same through a FrameList, the clip-at-a-time call and fill_video
    frames = VideoPredictor(x3d6, sampler, PU.MEAN, PU.STD, True, 176, 160, src_layout="BGRA")(TR.FrameList(list(view.unbind(0)), "BGRA"), 10)
    assert torch.equal(frames, want)
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="BGRA", **KW)
    ref = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
    clips = view[:8].unflatten(0, (2, 4))
    assert torch.equal(packer(clips).clone(), ref(rgb[:8].unflatten(0, (2, 4))).clone())
    table = torch.tensor([[0, 3, 6, 9], [11, 7, 2, 2]])
    packer.fill_video(view, packer.video_tables(table, 12), 0, 6)
    a = packer.launch().clone()
    ref.fill_video(rgb, ref.video_tables(table, 12), 0, 6)
    assert torch.equal(a, ref.launch())


def test_tube_predictor_scores_bgr_frames(x3d6):
    from pytorchvideo_amd.inference import TubePredictor
    view, rgb, swapped = _video("BGR", 9, 180, 240, 21)
    stamps, boxes = [[0.5, 1.5]], [[torch.tensor([[21.0, 11.0, 121.0, 111.0]]), torch.tensor([[101.0, 31.0, 240.0, 170.0]])]]
    got = TubePredictor(x3d6, 1.0, crop_size=160, context=1.0, square=True, src_layout="BGR", **KW)([view], 4, stamps, boxes).clone()
    dense = TubePredictor(x3d6, 1.0, crop_size=160, context=1.0, square=True, src_layout="NTHWC", **KW)
    want, other = dense([rgb], 4, stamps, boxes).clone(), dense([swapped], 4, stamps, boxes).clone()
    assert tuple(got.shape) == (2, 400) and torch.equal(got, want) and not torch.equal(got, other)


def test_keyframe_detector_scores_a_bgra_surface():
    """The detection form and the boxes of tests/test_gpu_keyframe_detection.py, its no-crop protocol."""
    import test_gpu_keyframe_detection as KD
    from pytorchvideo_amd.inference import KeyframeDetector
    dm = KD._form("resnet_det_r50_small", torch.bfloat16, 48, 72)[0]
    view, rgb, swapped = _video("BGRA", 40, 60, 90, 22)
    box_list = KD._split(KD.box_set(60, 90), KD.COUNTS)
    got = KeyframeDetector(dm, KD.DURATION, short_side=48, src_layout="BGRA", **KW)(view, KD.FPS, KD.STAMPS, box_list).clone()
    dense = KeyframeDetector(dm, KD.DURATION, short_side=48, src_layout="NTHWC", **KW)
    want, other = dense(rgb, KD.FPS, KD.STAMPS, box_list).clone(), dense(swapped, KD.FPS, KD.STAMPS, box_list).clone()
    assert tuple(got.shape) == (sum(KD.COUNTS), 16) and torch.equal(got, want) and not torch.equal(got, other)
