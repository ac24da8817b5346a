"""YUV 4:2:2 and 4:4:4 on the MI355X (include/pv_mi355x.h "YUV 4:2:2 and 4:4:4"): `pv_batch_views`, `pv_frame_views`,
`pv_region_views` and `pv_area_views` on planar and semi-planar frames of 8- and 16-bit samples, read where they lie.

The frames are views into a larger random buffer (tests/yuv4_util.py): one sample into the buffer (an odd address for 8-bit
samples, an even one for 16-bit samples), a pitch that is no multiple of 16, a coded height above the display height.  4:2:2 is
46 x 70 and 4:4:4 is 45 x 71, five frames; short side 36, crop 32, views (0, 1, 2); the table repeats a frame and leaves the
video.  Every comparison is `torch.equal` on the bits, except against the host mirror (section 3):
  1. the unchanged 4:2:0 launch is the reference: it equals the 4:4:4 launch on the copy whose chroma is replicated 2 x 2 and the
     4:2:2 launch on the copy whose chroma rows are replicated;
  2. every 4:2:2 layout equals the 4:4:4 launch on its column-replicated copy;
  3. unrelated full-resolution chroma against `yuv_to_rgb` + the pinned formula, with the bound of tests/test_gpu_yuv_ingest.py;
  4. footprint and independence;  5. the public API."""
import pytest
import torch

import packed_util as PU
import spatial_util as SU
import yuv4_util as Y4
from pytorchvideo_amd import transforms as TR

pytestmark = pytest.mark.gpu

N, SHORT, CROP, VIEWS = 5, 36, 32, (0, 1, 2)
TABLE = torch.tensor([[0, 2, 2, -3, 9], [4, 99, 1, 3, 0]], dtype=torch.int32)   # a repeated frame, entries outside the video
ITEMS = [(0, 0, 0), (0, 1, 2), (0, 0, 1), (0, 1, 0)]                            # (source, row, view): every view, both rows
TAP = 4 * 2.0 ** -14                                             # tests/test_gpu_yuv_ingest.py's constants
MAX_SCALE = 1.0 / (255.0 * min(PU.STD))
F32, C4 = PU.FORMS[1], PU.FORMS[2]                               # planar fp32 (every bit of a result), the 4-channel layout
# three bilinear geometries: the suite's (dense staging), a downscale above 2x (sparse staging), an upscale (dense)
BILINEAR = [dict(short=SHORT, crop=CROP, idxs=VIEWS), dict(short=16, crop=16, idxs=VIEWS), dict(short=60, crop=56, idxs=VIEWS)]


def _matrix(sb, bits=8, msb=False, standard="bt601", full=False):
    return TR.yuv_matrix(standard, full, bits if sb == 2 else 8, msb if sb == 2 else False)


def _equal(got, want):
    return torch.equal(PU.bits(got[0]), PU.bits(want[0]))


def _check_footprint(dst, cl, n_written):
    inside, outside = PU.footprint(dst, cl, n_written)
    assert not torch.isnan(dst[inside].float()).any() and torch.isnan(dst[outside].float()).all()


def _cases(frames):
    """(name, launch keywords, items) of every entry point on a 46 x 70 source with even rectangles."""
    regions = torch.tensor([[[2, 4, 20, 30], [6, 28, 40, 42], [4, 0, 18, 24], [0, 0, 46, 70], [26, 38, 20, 32]],
                            [[0, 0, 46, 70], [2, 6, 40, 60], [10, 12, 8, 10], [12, 2, 30, 40], [4, 4, 4, 4]]])
    out = [("bilinear%d" % k, dict(frames=frames, **kw), ITEMS) for k, kw in enumerate(BILINEAR)]
    out.append(("region_up", dict(frames=frames, regions=regions, window=(CROP, 40)), [(0, 1, 0), (0, 0, 0)]))
    out.append(("region_down", dict(frames=frames, regions=regions[:, :, :] * 0 + torch.tensor([0, 0, 46, 70]), window=(16, 16)),
                [(0, 1, 0), (0, 0, 0)]))
    out.append(("area_36", dict(frames=frames, area=True, short=SHORT, crop=CROP, idxs=VIEWS), ITEMS))
    out.append(("area_2.6", dict(frames=frames, area=True, short=18, crop=16, idxs=VIEWS), ITEMS))          # windows of 2 to 3 rows, 3 to 4 ...
    out.append(("area_two_column_tiles", dict(frames=frames, area=True, short=46, window=(46, 70), idxs=(1,)), [(0, 0, 0), (0, 1, 0)]))
    return out


# ----------------------------------------------------------------------------- 1: the existing path is the reference
@pytest.mark.parametrize("frames", [False, True], ids=["video", "framelist"])
@pytest.mark.parametrize("layout", ["NV12", "I420", "P010", "I010"])
def test_the_420_launch_equals_the_launches_on_its_replicated_copies(layout, frames):
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    y, u, v = Y4.planes(N, 46, 70, Y4.SUB420, 300 + sb + c_step, sb, bits, msb)
    m = _matrix(sb, bits, msb)
    s420 = Y4.Surface(y, u, v, Y4.SUB420, c_step, v_first, sb, 1, "cuda")
    s422 = Y4.Surface(*Y4.replicated(y, u, v, Y4.SUB420, Y4.SUB422), Y4.SUB422, c_step, v_first, sb, 2, "cuda")
    s444 = Y4.Surface(*Y4.replicated(y, u, v, Y4.SUB420, Y4.SUB444), Y4.SUB444, c_step, v_first, sb, 3, "cuda")
    for name, kw, items in _cases(frames):
        for form, dtype in PU.FORMS:
            want = Y4.launch([s420], TABLE, items, form, dtype, m, **kw)
            for s in (s422, s444):
                got = Y4.launch([s], TABLE, items, form, dtype, m, **kw)
                assert _equal(got, want), (name, form, dtype, s.sub)
                _check_footprint(got[0], got[1], len(items))
    assert not torch.equal(want[0][0], want[0][1])               # (the items differ)


# ----------------------------------------------------------------------------- 2: subsampled equals replicated
@pytest.mark.parametrize("layout", TR.YUV422_LAYOUTS)
def test_every_422_layout_equals_the_444_launch_on_its_column_replicated_copy(layout):
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    y, u, v = Y4.planes(N, 46, 70, Y4.SUB422, 400 + sb + c_step, sb, bits, msb)
    m = _matrix(sb, bits, msb, "bt709", True)
    s422 = Y4.surface_of(layout, y, u, v, 4, "cuda")
    s444 = Y4.Surface(*Y4.replicated(y, u, v, Y4.SUB422, Y4.SUB444), Y4.SUB444, c_step, v_first, sb, 5, "cuda")
    assert s422.geom == {k: TR.yuv_geometry(s422.view, layout, height=46)[k] for k in s422.geom}
    for name, kw, items in _cases(False):
        if name in ("region_up", "region_down"):                 # 4:2:2: only left and w are even
            kw = dict(kw, regions=kw["regions"] + torch.tensor([1, 0, -1, 0]))
        for form, dtype in (F32, C4):
            got = Y4.launch([s422], TABLE, items, form, dtype, m, **kw)
            assert _equal(got, Y4.launch([s444], TABLE, items, form, dtype, m, **kw)), (name, form)
            _check_footprint(got[0], got[1], len(items))
    # orient 1, 4 and 7 mixed with an upright record in one launch: strips and tiles
    items = [(1, 0, 0), (0, 1, 1), (2, 1, 2), (3, 0, 1), (0, 0, 2), (1, 1, 1)]
    for frames in (False, True):
        for form, dtype in (F32, C4, PU.FORMS[4]):
            kw = dict(short=SHORT, crop=CROP, idxs=VIEWS, frames=frames, orients=[0, 1, 4, 7])
            got = Y4.launch([s422] * 4, TABLE, items, form, dtype, m, **kw)
            assert _equal(got, Y4.launch([s444] * 4, TABLE, items, form, dtype, m, **kw)), (frames, form)
            _check_footprint(got[0], got[1], len(items))
    alone = Y4.launch([s422] * 4, TABLE, items[3:4], form, dtype, m, **kw)        # an oriented item launched alone
    assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][3]))


def test_an_oriented_422_record_is_the_upright_launch_on_the_oriented_444_copy():
    """The orientation contract: a quarter turn of a subsampled frame is no layout of its own, so the oriented item equals the
    upright 4:4:4 launch on the column-replicated copy oriented beforehand."""
    y, u, v = Y4.planes(N, 46, 70, Y4.SUB422, 450)
    m = _matrix(1)
    s422 = Y4.surface_of("NV16", y, u, v, 6, "cuda")
    full = Y4.replicated(y, u, v, Y4.SUB422, Y4.SUB444)
    for orient in (1, 2, 5, 7):
        turned = [TR.oriented(p, orient).contiguous() for p in full]
        s444 = Y4.Surface(*turned, Y4.SUB444, 2, False, 1, 7, "cuda")
        kw = dict(short=SHORT, crop=CROP, idxs=VIEWS)
        got = Y4.launch([s422], TABLE, ITEMS, *F32, m, orients=[orient], **kw)
        assert _equal(got, Y4.launch([s444], TABLE, ITEMS, *F32, m, **kw)), orient


# ----------------------------------------------------------------------------- 3: independent full-resolution chroma
def _resampled(rgb, table, short, crop, idxs, affine=True):
    """[N, 3, Hs, Ws] virtual RGB frames -> planar [rows * views, 3, T, crop, crop] by the pinned formula."""
    n, _, hs, ws = rgb.shape
    clips = rgb[table.long().clamp(0, n - 1)].permute(0, 2, 1, 3, 4)
    hn, wn = TR.scaled_size(hs, ws, short)
    scale, shift = PU.affine("cpu") if affine else (None, None)
    out = [SU.pinned_resample(clips, hn, wn, *TR.crop_offsets(hn, wn, crop, v), crop, crop, scale, shift) for v in idxs]
    return torch.stack(out, dim=1).reshape(table.shape[0] * len(idxs), 3, table.shape[1], crop, crop)


def _check(got, ref, hs, ws, max_scale, bf16, what):
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).abs()
    tol = SU.bound(ref, hs, ws, max_scale, bf16) + TAP * max_scale
    print("%s: worst |d| %.3e, smallest bound %.3e" % (what, err.max().item(), tol.min().item()))
    assert bool((err <= tol).all()), "%s: %d elements over the bound, worst %.3e" % (what, int((err > tol).sum()), err.max().item())


ALL_ITEMS = [(0, r, v) for r in (0, 1) for v in (0, 1, 2)]


@pytest.mark.parametrize("standard,full", [("bt601", False), ("bt709", True)], ids=["bt601_limited", "bt709_full"])
@pytest.mark.parametrize("layout", ["I444", "I410", "NV24", "I422"])
def test_unrelated_chroma_planes_against_the_host_mirror(layout, standard, full):
    name = "I444" if layout == "NV24" else layout
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[name]
    h, w = (46, 70) if sub == Y4.SUB422 else (45, 71)            # 4:4:4: odd sizes
    y, u, v = Y4.planes(N, h, w, sub, 500 + sb, sb, bits, msb)
    m = TR._yuv_matrix_of((standard, full), name)
    host = Y4.surface_of(name, y, u, v, 8)
    rgb = TR.yuv_to_rgb(host.view, name, m.float().double(), height=h)
    dev = Y4.Surface(y, u, v, sub, 2, False, sb, 9, "cuda") if layout == "NV24" else Y4.surface_of(name, y, u, v, 8, "cuda")
    for kw in BILINEAR[:2]:
        want = _resampled(rgb, TABLE, kw["short"], kw["crop"], VIEWS)
        for form, dtype in (F32, PU.FORMS[0]):
            dst, _ = Y4.launch([dev], TABLE, ALL_ITEMS, form, dtype, m, **kw)
            _check(dst[:6], want, h, w, MAX_SCALE, dtype == torch.bfloat16, "%s %s %s" % (layout, standard, kw["short"]))


def test_the_clamp_sits_on_the_taps():
    """Frames of (Y, U, V) corners, far out of gamut, equal the CLAMPED mirror -- and neither a clamp behind the blend nor no
    clamp at all would (tests/test_gpu_yuv_ingest.py::test_yuv_views_clamps_every_tap_before_the_blend, at full chroma)."""
    g = torch.Generator().manual_seed(1206)
    y, u, v = [torch.randint(0, 2, (2, 33, 45), generator=g, dtype=torch.int64) * 255 for _ in range(3)]
    table = torch.tensor([[0, 1]], dtype=torch.int32)
    m = TR.yuv_matrix("bt601", False)
    want = _resampled(TR.yuv_to_rgb(Y4.surface_of("I444", y, u, v).view, "I444", m.float().double(), height=33), table, 41, 37, (1,), False)
    dst, _ = Y4.launch([Y4.surface_of("I444", y, u, v, 1, "cuda")], table, [(0, 0, 0)], *F32, m, short=41, crop=37, idxs=(1,), affine=False)
    _check(dst[:1], want, 33, 45, 1.0, False, "I444 corners")
    assert want.min().item() >= 0.0 and want.max().item() <= 255.0
    md = m.float().double()
    raw = torch.stack([md[c, 0] * y.double() + md[c, 1] * u.double() + md[c, 2] * v.double() + md[c, 3] for c in range(3)], dim=1).float()
    assert raw.min().item() < -100 and raw.max().item() > 400
    unclamped = _resampled(raw, table, 41, 37, (1,), False)
    tol = SU.bound(want, 33, 45, 1.0) + TAP
    assert bool(((unclamped - want).abs() > 100 * tol).any())
    assert bool(((torch.clamp(unclamped, 0, 255) - want).abs() > 100 * tol).any())


# ----------------------------------------------------------------------------- 4: footprint and independence
@pytest.mark.parametrize("layout", ["I422", "NV61", "I210", "I444", "I416"])
def test_padding_and_coded_rows_change_no_bit_and_items_are_independent(layout):
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    h, w = (46, 70) if sub == Y4.SUB422 else (45, 71)
    y, u, v = Y4.planes(N, h, w, sub, 600 + sb, sb, bits, msb)
    m = _matrix(sb, bits, msb)
    a, b = Y4.surface_of(layout, y, u, v, 10, "cuda"), Y4.surface_of(layout, y, u, v, 11, "cuda")
    assert not torch.equal(a.buf, b.buf) and a.geom == b.geom   # other padding, other rows behind the display height
    regions = torch.tensor([[[1, 2, 21, 30]] * 5, [[0, 0, h, w - w % 2]] * 5])
    for kw in (BILINEAR[0], BILINEAR[1], dict(area=True, **BILINEAR[0]), dict(regions=regions, window=(CROP, 40))):
        items = ITEMS if "regions" not in kw else [(0, 1, 0), (0, 0, 0)]
        for form, dtype in (F32, C4):
            got = Y4.launch([a], TABLE, items, form, dtype, m, **kw)
            _check_footprint(got[0], got[1], len(items))
            assert _equal(Y4.launch([b], TABLE, items, form, dtype, m, **kw), got)
            alone = Y4.launch([a], TABLE, items[1:2], form, dtype, m, **kw)
            assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][1]))


@pytest.mark.parametrize("sub", [Y4.SUB422, Y4.SUB444], ids=["422", "444"])
def test_two_sources_of_different_sizes_and_pitches_share_a_launch(sub):
    """Records with different frame sizes, pitches and alignments in one launch, items interleaved: each item is the item of
    its source launched alone."""
    m = _matrix(1)
    a = Y4.Surface(*Y4.planes(N, 46, 70, sub, 700), sub, 1, False, 1, 12, "cuda")
    b = Y4.Surface(*Y4.planes(3, 61, 40 if sub[1] else 39, sub, 701), sub, 1, True, 1, 13, "cuda")
    assert a.geom["y_pitch"] != b.geom["y_pitch"]
    table = torch.tensor([[0, 2, 1], [2, 0, 0]], dtype=torch.int32)
    items = [(1, 0, 2), (0, 1, 0), (1, 1, 1), (0, 0, 1)]
    for kw in (BILINEAR[0], dict(area=True, **BILINEAR[0])):
        for frames in (False, True):
            got = Y4.launch([a, b], table, items, *F32, m, frames=frames, **kw)
            for k, (src, row, view) in enumerate(items):
                alone = Y4.launch([(a, b)[src]], table, [(0, row, view)], *F32, m, frames=frames, **kw)
                assert torch.equal(PU.bits(alone[0][0]), PU.bits(got[0][k])), (k, frames)


# ----------------------------------------------------------------------------- 5: through the public API
KW = dict(mean=PU.MEAN, std=PU.STD, div255=True)
YUV = ("bt601", False)


@pytest.mark.parametrize("layout", ["I422", "NV16", "I210", "I444"])
def test_device_scale_crop_and_resized_crop_are_the_raw_launches(layout):
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    h, w = (46, 70) if sub == Y4.SUB422 else (45, 71)
    s = Y4.surface_of(layout, *Y4.planes(8, h, w, sub, 800 + sb, sb, bits, msb), 14, "cuda")
    clips = s.view.unflatten(0, (2, 4))
    assert not clips.is_contiguous()
    m = TR._yuv_matrix_of(YUV, layout)
    table = torch.arange(8, dtype=torch.int32).reshape(2, 4)
    for mode in ("bilinear", "area"):
        got = TR.device_scale_crop(clips, SHORT, CROP, VIEWS, dtype=torch.float32, src_layout=layout, yuv=YUV, height=h,
                                   interpolation=mode, **KW)
        raw, _ = Y4.launch([s], table, ALL_ITEMS, *F32, m, short=SHORT, crop=CROP, idxs=VIEWS, area=mode == "area")
        assert got.shape == (6, 3, 4, CROP, CROP) and torch.equal(got, raw[:6]), mode
    regions = torch.tensor([[[1, 2, 30, 40]] * 4, [[h - 21, w - 34 - w % 2, 21, 32]] * 4])
    got = TR.device_resized_crop(clips, regions, (CROP, 40), dtype=torch.float32, src_layout=layout, yuv=YUV, height=h, **KW)
    raw, _ = Y4.launch([s], table, [(0, 0, 0), (0, 1, 0)], *F32, m, regions=regions, window=(CROP, 40))
    assert torch.equal(got, raw[:2])


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


def _dense(layout, y, u, v):
    """The contiguous frames (pitch W) of a planar layout: [N, rows, W] on the device."""
    sb = Y4.LAYOUT[layout][3]
    n, _, w = y.shape
    flat = torch.cat([p.reshape(n, -1) for p in (y, u, v)], 1).reshape(n, -1, w)
    return flat.to(torch.uint8 if sb == 1 else torch.int16).cuda()


@pytest.fixture(scope="module")
def videos():
    """A 23-frame 64 x 86 4:2:2 video, contiguous, and its column-replicated 4:4:4 copy."""
    y, u, v = Y4.planes(23, 64, 86, Y4.SUB422, 900)
    return _dense("I422", y, u, v), _dense("I444", *Y4.replicated(y, u, v, Y4.SUB422, Y4.SUB444))


@pytest.mark.parametrize("layout", ["I422", "NV16", "I210", "I444"])
def test_device_packer_is_the_forward_on_the_views_of_device_scale_crop(x3d6, layout):
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    s = Y4.surface_of(layout, *Y4.planes(8, 180, 240, sub, 850 + sb, sb, bits, msb), 15, "cuda")
    clips = s.view.unflatten(0, (2, 4))
    packer = TR.DevicePacker(x3d6, short_side=176, crop_size=160, spatial_idx=VIEWS, src_layout=layout, yuv=YUV, height=180, **KW)
    logits = packer(clips).clone()
    views = TR.device_scale_crop(clips, 176, 160, VIEWS, src_layout=layout, yuv=YUV, height=180, **KW)
    assert tuple(logits.shape) == (6, 400) and torch.isfinite(logits).all() and torch.equal(logits, x3d6(views).clone())


def test_video_predictor_scores_422_as_the_replicated_444_video(x3d6, videos):
    from pytorchvideo_amd import data as D
    from pytorchvideo_amd.inference import VideoPredictor
    v422, v444 = videos
    sampler = D.UniformClipSampler(0.8)
    args = dict(short_side=176, crop_size=160, spatial_idx=VIEWS, yuv=YUV, **KW)
    got = VideoPredictor(x3d6, sampler, src_layout="I422", **args)(v422, 10).clone()
    want = VideoPredictor(x3d6, sampler, src_layout="I444", **args)(v444, 10).clone()
    swapped = VideoPredictor(x3d6, sampler, src_layout="YV16", **args)(v422, 10).clone()
    assert tuple(got.shape) == (400,) and torch.isfinite(got).all()
    assert torch.equal(got, want) and not torch.equal(got, swapped)
    frames = VideoPredictor(x3d6, sampler, src_layout="I422", **args)(TR.FrameList(list(v422.unbind(0)), "I422"), 10)
    assert torch.equal(frames, want)


def test_stream_predictor_scores_422_frames_as_the_replicated_444_frames(x3d6, videos):
    from fractions import Fraction
    from pytorchvideo_amd.inference import StreamPredictor
    v422, v444 = videos
    dur, stride, fps = Fraction(8, 10), Fraction(3, 10), 10
    args = dict(short_side=176, crop_size=160, spatial_idx=VIEWS, yuv=YUV, **KW)
    got = StreamPredictor(x3d6, dur, stride, fps, src_layout="I422", **args).push([f.clone() for f in v422.unbind(0)])
    want = StreamPredictor(x3d6, dur, stride, fps, src_layout="I444", **args).push([f.clone() for f in v444.unbind(0)])
    assert [k for k, _, _ in got] == list(range(6)) == [k for k, _, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0][2], got[5][2])
