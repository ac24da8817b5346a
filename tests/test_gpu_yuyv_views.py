"""Packed YUV 4:2:2 on the MI355X (include/pv_mi355x.h "packed YUV 4:2:2"): `pv_batch_views`, `pv_frame_views`,
`pv_region_views` and `pv_area_views` on YUY2 / YVYU / UYVY / VYUY frames of 8-bit samples and Y210 / Y212 / Y216 frames of 16-bit
samples, read where they lie.

The frames are views into a larger random buffer (tests/yuyv_util.py): one sample into the buffer (an odd address for 8-bit
samples, an address that is 2 mod 4 for 16-bit samples), a pitch that exceeds the row and is no multiple of 16.  46 x 70 -- 35
macropixels a row, an odd count --, five frames; short side 36, crop 32, views (0, 1, 2); the table repeats a frame and leaves
the video.  These are the smallest sizes with a span that starts in the middle of a macropixel (the view offsets and the
scale put xs0 at odd columns), taps that straddle two macropixels, the right-edge column, both staging modes (short 16:
sparse), the tile footprint (oriented records) and the box filter's, with two column tiles.

The contract is ONE sentence, and every comparison is `torch.equal` on the bits: an item holds what the same entry point writes
with PV_SRC_YUV422, c_step 1, the same matrix and the same sample width for the de-interleaved planes of the same frames.
  1. every layout and every entry point against that planar launch;  2. orientation;  3. mixed sample orders in one launch;
  4. padding;  5. the offsets are read;  6. the public functions;  7. the predictors."""
import pytest
import torch

import packed_util as PU
import yuv4_util as Y4
import yuyv_util as YU
from pytorchvideo_amd import transforms as TR

pytestmark = pytest.mark.gpu

N, H, W, SHORT, CROP, VIEWS = 5, 46, 70, 36, 32, (0, 1, 2)
TABLE = torch.tensor([[0, 2, 2, -3, 9], [4, 99, 1, 3, 0]], dtype=torch.int32)   # a repeated frame, entries outside the video
ITEMS = [(0, 0, 0), (0, 1, 2), (0, 0, 1), (0, 1, 0)]                            # (source, row, view): every view, both rows
F32, C4 = PU.FORMS[1], PU.FORMS[2]                               # planar fp32 (every bit of a result), the 4-channel layout
# three bilinear geometries: the suite's (dense staging), a downscale above 2x (sparse staging), an upscale (dense)
BILINEAR = [dict(short=SHORT, crop=CROP, idxs=VIEWS), dict(short=16, crop=16, idxs=VIEWS), dict(short=60, crop=56, idxs=VIEWS)]
# rectangles with an even left and w, odd tops and heights among them, one of a single macropixel (w == 2)
REGIONS = torch.tensor([[[3, 4, 19, 30], [5, 28, 41, 42], [1, 0, 45, 2], [0, 0, 46, 70], [27, 38, 19, 32]],
                        [[0, 0, 46, 70], [1, 6, 39, 60], [11, 12, 7, 10], [13, 68, 31, 2], [3, 4, 5, 4]]])
# layout -> (sample order, sample bytes, bit depth, MSB-aligned): the strings, and VYUY through the raw descriptor
ALL = dict(YU.LAYOUT, VYUY=("VYUY", 1, 8, False))


def _matrix(sb, bits=8, msb=False, standard="bt601", full=False):
    return TR.yuv_matrix(standard, full, bits if sb == 2 else 8, msb if sb == 2 else False)


def _equal(got, want):
    return torch.equal(PU.bits(got[0]), PU.bits(want[0]))


def _check_footprint(dst, cl, n_written):
    inside, outside = PU.footprint(dst, cl, n_written)
    assert not torch.isnan(dst[inside].float()).any() and torch.isnan(dst[outside].float()).all()


def _cases(frames):
    """(name, launch keywords, items) of every entry point on a 46 x 70 source."""
    out = [("bilinear%d" % k, dict(frames=frames, **kw), ITEMS) for k, kw in enumerate(BILINEAR)]
    out.append(("region_up", dict(frames=frames, regions=REGIONS, window=(CROP, 40)), [(0, 1, 0), (0, 0, 0)]))
    out.append(("region_down", dict(frames=frames, regions=REGIONS, window=(5, 6)), [(0, 1, 0), (0, 0, 0)]))
    out.append(("area_36", dict(frames=frames, area=True, short=SHORT, crop=CROP, idxs=VIEWS), ITEMS))
    out.append(("area_2.6", dict(frames=frames, area=True, short=18, crop=16, idxs=VIEWS), ITEMS))          # windows of 2 to 3 rows, 3 to 4 ...
    out.append(("area_two_column_tiles", dict(frames=frames, area=True, short=46, window=(46, 70), idxs=(1,)), [(0, 0, 0), (0, 1, 0)]))
    return out


@pytest.fixture(scope="module")
def sources():
    """Per sample width: the planes, their planar PV_SRC_YUV422 surface (the reference of every launch) and a cache of the
    reference launches, which several tests share."""
    out = {}
    for sb, bits, msb in ((1, 8, False), (2, 10, True)):
        y, u, v = YU.planes(N, H, W, 300 + sb, sb, bits, msb)
        out[sb] = dict(planes=(y, u, v), planar=YU.planar_of(y, u, v, sb, 1, "cuda"), m=_matrix(sb, bits, msb), cache={})
    return out


def _reference(src, key, items, form, dtype, **kw):
    k = (key, form, dtype)
    if k not in src["cache"]:
        src["cache"][k] = Y4.launch([src["planar"]], TABLE, items, form, dtype, src["m"], **kw)
    return src["cache"][k]


# ----------------------------------------------------------------------------- 1: every layout, every entry point
@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("layout", list(ALL))
def test_every_layout_equals_the_planar_422_launch_on_the_deinterleaved_planes(sources, layout, frames):
    order, sb, _, _ = ALL[layout]
    src = sources[sb]                                            # (the bit depth lives in the matrix: Y212 / Y216 read the same codes)
    packed = YU.Packed(*src["planes"], order, sb, 2, "cuda")
    if layout in TR.YUYV_LAYOUTS:                                # the strings name the very fields the surface was built with
        assert packed.geom == {k: TR.yuyv_geometry(packed.view, layout)[k] for k in packed.geom}
    forms = PU.FORMS if layout in ("YUY2", "Y210") else (F32, C4)
    for name, kw, items in _cases(frames):
        for form, dtype in forms:
            got = Y4.launch([packed], TABLE, items, form, dtype, src["m"], **kw)
            assert _equal(got, _reference(src, (name, frames), items, form, dtype, **kw)), (name, form, dtype)
            _check_footprint(got[0], got[1], len(items))
    assert not torch.equal(got[0][0], got[0][1])                 # (the items differ)


# ----------------------------------------------------------------------------- 2: orientation
@pytest.mark.parametrize("layout", ["YUY2", "UYVY", "Y210"])
def test_oriented_records_equal_the_planar_launch_of_the_same_records(sources, layout):
    """Orients 1, 4 and 7 mixed with an upright record in one launch: strips and tiles."""
    order, sb, _, _ = ALL[layout]
    src = sources[sb]
    packed = YU.Packed(*src["planes"], order, sb, 3, "cuda")
    items = [(1, 0, 0), (0, 1, 1), (2, 1, 2), (3, 0, 1), (0, 0, 2), (1, 1, 1)]
    for frames in (False, True):
        for form, dtype in (F32, C4, PU.FORMS[4]):
            for geo in BILINEAR[:2]:
                kw = dict(frames=frames, orients=[0, 1, 4, 7], **geo)
                got = Y4.launch([packed] * 4, TABLE, items, form, dtype, src["m"], **kw)
                assert _equal(got, Y4.launch([src["planar"]] * 4, TABLE, items, form, dtype, src["m"], **kw)), (frames, form, geo)
                _check_footprint(got[0], got[1], len(items))
    alone = Y4.launch([packed] * 4, TABLE, items[3:4], form, dtype, src["m"], **kw)        # an oriented item launched alone
    assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][3]))


# ----------------------------------------------------------------------------- 3: one launch, several sample orders
@pytest.mark.parametrize("sb", [1, 2], ids=["u8", "u16"])
def test_records_of_different_orders_sizes_and_pitches_share_a_launch(sb):
    """Items interleaved over four records -- one per sample order, two frame sizes and pitches --: each item is the item of
    its source launched alone, and the item of the planar launch."""
    m = _matrix(sb, 12, True)
    sizes = [(N, 46, 70), (3, 61, 40), (3, 33, 46), (4, 46, 70)]
    planes = [YU.planes(n, h, w, 700 + k, sb, 12, True) for k, (n, h, w) in enumerate(sizes)]
    packed = [YU.Packed(*p, order, sb, 12 + k, "cuda") for k, (p, order) in enumerate(zip(planes, YU.ORDERS))]
    planar = [YU.planar_of(*p, sb, 20 + k, "cuda") for k, p in enumerate(planes)]
    assert len({s.geom["y_pitch"] for s in packed}) == 3 and len({(s.geom["u_offset"], s.geom["v_offset"]) for s in packed}) == 4
    table = torch.tensor([[0, 2, 1], [2, 0, 0]], dtype=torch.int32)
    items = [(1, 0, 2), (0, 1, 0), (3, 1, 1), (2, 0, 1), (0, 0, 1), (2, 1, 0), (3, 0, 2), (1, 1, 1)]
    for kw in (BILINEAR[0], dict(area=True, **BILINEAR[0])):
        for frames in (False, True):
            got = Y4.launch(packed, table, items, *F32, m, frames=frames, **kw)
            assert _equal(got, Y4.launch(planar, table, items, *F32, m, frames=frames, **kw)), (kw, frames)
            for k, (s, row, view) in enumerate(items[:4]):
                alone = Y4.launch([packed[s]], table, [(0, row, view)], *F32, m, frames=frames, **kw)
                assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][k])), (k, frames)


# ----------------------------------------------------------------------------- 4: padding;  5: the offsets are read
@pytest.mark.parametrize("layout", ["YVYU", "UYVY", "Y216"])
def test_the_padding_changes_no_bit_and_the_offsets_are_read(sources, layout):
    order, sb, _, _ = ALL[layout]
    src = sources[sb]
    y, u, v = src["planes"]
    a, b = YU.Packed(y, u, v, order, sb, 10, "cuda"), YU.Packed(y, u, v, order, sb, 11, "cuda")
    assert not torch.equal(a.buf, b.buf) and a.geom == b.geom   # other bytes between 2 * Ws * SB and the pitch, and between frames
    assert torch.equal(a.view, b.view)
    swapped = YU.Packed(y, u, v, order, sb, 10, "cuda")         # the same bytes, U and V swapped in the record
    swapped.geom = dict(a.geom, u_offset=a.geom["v_offset"], v_offset=a.geom["u_offset"])
    exchanged = YU.planar_of(y, v, u, sb, 4, "cuda")            # ... which reads the frames whose chroma planes are exchanged
    for kw in (BILINEAR[0], BILINEAR[1], dict(area=True, **BILINEAR[0]), dict(regions=REGIONS, window=(CROP, 40)),
               dict(orients=[5], **BILINEAR[0])):
        items = ITEMS if "regions" not in kw else [(0, 1, 0), (0, 0, 0)]
        for form, dtype in (F32, C4):
            got = Y4.launch([a], TABLE, items, form, dtype, src["m"], **kw)
            _check_footprint(got[0], got[1], len(items))
            assert _equal(Y4.launch([b], TABLE, items, form, dtype, src["m"], **kw), got)
            alone = Y4.launch([a], TABLE, items[1:2], form, dtype, src["m"], **kw)
            assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][1]))
            other = Y4.launch([swapped], TABLE, items, form, dtype, src["m"], **kw)
            assert not _equal(other, got) and _equal(other, Y4.launch([exchanged], TABLE, items, form, dtype, src["m"], **kw))


# ----------------------------------------------------------------------------- 6: through the public API
KW = dict(mean=PU.MEAN, std=PU.STD, div255=True)
YUV = ("bt601", False)
ALL_ITEMS = [(0, r, v) for r in (0, 1) for v in (0, 1, 2)]


@pytest.mark.parametrize("layout", TR.YUYV_LAYOUTS + ("YUYV",))
def test_device_scale_crop_and_resized_crop_are_the_raw_launches(layout):
    order, sb, bits, msb = YU.LAYOUT.get(layout, YU.LAYOUT["YUY2"])
    y, u, v = YU.planes(8, H, W, 800 + sb, sb, bits, msb)
    s = YU.Packed(y, u, v, order, sb, 14, "cuda")
    planar = YU.planar_of(y, u, v, sb, 15, "cuda")
    clips = s.view.unflatten(0, (2, 4))
    assert not clips.is_contiguous()
    m = TR._yuv_matrix_of(YUV, layout)
    table = torch.arange(8, dtype=torch.int32).reshape(2, 4)
    for mode in ("bilinear", "area"):
        got = TR.device_scale_crop(clips, SHORT, CROP, VIEWS, dtype=torch.float32, src_layout=layout, yuv=YUV, interpolation=mode, **KW)
        for surface in (s, planar):
            raw, _ = Y4.launch([surface], table, ALL_ITEMS, *F32, m, short=SHORT, crop=CROP, idxs=VIEWS, area=mode == "area")
            assert got.shape == (6, 3, 4, CROP, CROP) and torch.equal(got, raw[:6]), mode
    regions = torch.tensor([[[1, 2, 30, 40]] * 4, [[H - 21, W - 34, 21, 32]] * 4])
    got = TR.device_resized_crop(clips, regions, (CROP, 40), dtype=torch.float32, src_layout=layout, yuv=YUV, **KW)
    for surface in (s, planar):
        raw, _ = Y4.launch([surface], table, [(0, 0, 0), (0, 1, 0)], *F32, m, regions=regions, window=(CROP, 40))
        assert torch.equal(got, raw[:2])
    # a pitched column slice that starts at an even column is read in place: it is the launch on the planes' columns
    cut = TR.device_scale_crop(clips[:, :, :, 6:54], 30, 28, VIEWS, dtype=torch.float32, src_layout=layout, yuv=YUV, **KW)
    part = YU.planar_of(y[:, :, 6:54].contiguous(), u[:, :, 3:27].contiguous(), v[:, :, 3:27].contiguous(), sb, 16, "cuda")
    raw, _ = Y4.launch([part], table, ALL_ITEMS, *F32, m, short=30, crop=28, idxs=VIEWS)
    assert torch.equal(cut, raw[:6])


@pytest.fixture(scope="module")
def x3d6():
    """x3d_xs (4 x 160 x 160, 400 classes) converted for 6 items: the recipe of tests/test_gpu_yuv4_views.py."""
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    m = trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()
    transmute_model(m, "mi355x")
    return convert_to_deployable_form(m, seeded_input((6, 3, 4, 160, 160), 6).cuda().bfloat16(), dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def videos():
    """A 23-frame 64 x 86 YUY2 video, contiguous [N, H, W, 2], and its I422 copy [N, 2H, W]."""
    y, u, v = YU.planes(23, 64, 86, 900)
    yuy2 = torch.stack([y, torch.stack([u, v], -1).reshape(23, 64, 86)], -1).to(torch.uint8)
    assert torch.equal(yuy2[:, :, 0::2, 1].long(), u) and torch.equal(yuy2[:, :, 1::2, 1].long(), v) and torch.equal(yuy2[..., 0].long(), y)
    planar = TR.yuyv_to_planar(yuy2, "YUY2")
    assert torch.equal(planar, torch.cat([p.reshape(23, -1) for p in (y, u, v)], 1).reshape(23, 128, 86).to(torch.uint8))
    return yuy2.cuda(), planar.cuda()


@pytest.mark.parametrize("layout", ["YUY2", "UYVY", "Y210"])
def test_device_packer_is_the_forward_on_the_views_of_device_scale_crop(x3d6, layout):
    order, sb, bits, msb = YU.LAYOUT[layout]
    s = YU.Packed(*YU.planes(8, 180, 240, 850 + sb, sb, bits, msb), order, sb, 15, "cuda")
    clips = s.view.unflatten(0, (2, 4))
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=VIEWS, src_layout=layout, yuv=YUV, **KW)
    logits = packer(clips).clone()
    views = TR.device_scale_crop(clips, 176, 160, VIEWS, src_layout=layout, yuv=YUV, **KW)
    assert tuple(logits.shape) == (6, 400) and torch.isfinite(logits).all() and torch.equal(logits, x3d6(views).clone())


# ----------------------------------------------------------------------------- 7: the predictors
def test_video_predictor_scores_yuy2_as_its_i422_copy(x3d6, videos):
    from pytorchvideo_amd import data as D
    from pytorchvideo_amd.inference import VideoPredictor
    yuy2, i422 = videos
    sampler = D.UniformClipSampler(0.8)
    args = dict(short_side=176, crop_size=160, spatial_idx=VIEWS, yuv=YUV, **KW)
    got = VideoPredictor(x3d6, sampler, src_layout="YUY2", **args)(yuy2, 10).clone()
    want = VideoPredictor(x3d6, sampler, src_layout="I422", **args)(i422, 10).clone()
    swapped = VideoPredictor(x3d6, sampler, src_layout="YVYU", **args)(yuy2, 10).clone()
    assert tuple(got.shape) == (400,) and torch.isfinite(got).all()
    assert torch.equal(got, want) and not torch.equal(got, swapped)
    frames = VideoPredictor(x3d6, sampler, src_layout="YUYV", **args)(TR.FrameList(list(yuy2.unbind(0)), "YUYV"), 10)
    assert torch.equal(frames, want)


def test_stream_predictor_scores_yuy2_frames_as_their_i422_copies(x3d6, videos):
    from fractions import Fraction
    from pytorchvideo_amd.inference import StreamPredictor
    yuy2, i422 = videos
    dur, stride, fps = Fraction(8, 10), Fraction(3, 10), 10
    args = dict(short_side=176, crop_size=160, spatial_idx=VIEWS, yuv=YUV, **KW)
    got = StreamPredictor(x3d6, dur, stride, fps, src_layout="YUY2", **args).push([f.clone() for f in yuy2.unbind(0)])
    want = StreamPredictor(x3d6, dur, stride, fps, src_layout="I422", **args).push([f.clone() for f in i422.unbind(0)])
    assert [k for k, _, _ in got] == list(range(6)) == [k for k, _, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0][2], got[5][2])
