"""`pv_yuv_views` on the MI355X: the ingest reading decoder-native YUV 4:2:0 (NV12 / NV21 / I420 / YV12) itself, and the
`src_layout="NV12"` ... paths of `device_scale_crop`, `DevicePacker` and `inference.VideoPredictor`.

Reference of every kernel case: `transforms.yuv420_to_rgb` -- the host mirror of the tap rule, conversion in fp64 with the
fp32 matrix the device holds, rounded once to fp32 -- followed by `spatial_util.pinned_resample` with the affine map.

Tolerance (derived, every element asserted): `spatial_util.bound(...)`, the bound the RGB kernels are held to, plus
4 * 2^-14 * max_scale: the conversion of a tap is three multiply-adds on magnitudes below 1024, so each rounding is at most
2^-14 raw units, the clamp is 1-Lipschitz, and four roundings are allowed so that the bound holds whether or not the compiler
contracts them; the blend's weights sum to one, so a tap error reaches the output at most once, times the affine scale."""
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
from pytorchvideo_amd.inference import VideoPredictor

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 7.0
MAX_SCALE = 1.0 / (255.0 * min(SU.STD))
TAP = 4 * 2.0 ** -14
M601 = TR.yuv_matrix("bt601", False)
M709F = TR.yuv_matrix("bt709", True)


# ----------------------------------------------------------------------------- kernel
def _destination(form, dtype, n, t, crop):
    if form == "planar":
        return torch.full((n, 3, t, crop, crop), SENTINEL, dtype=dtype, device="cuda"), None
    c_p, ld = {"c4": (4, 4), "cl8": (8, 8), "cl8_ld16": (8, 16)}[form]
    return torch.full((n, t, crop, crop, ld), SENTINEL, dtype=dtype, device="cuda"), (c_p, ld)


def _run(frames, layout, table, size, crop, idxs, form, dtype, matrix, item0=0, n_items=0, extra=1, affine=True, **geom_kw):
    """pv_yuv_views on device frames: (sentinel-filled destination of `extra` more items than the window, items written)."""
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
    dst, cl = _destination(form, dtype, n + extra, t, crop)
    d.dst, d.dst_dtype = dst.data_ptr(), (L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32)
    if cl is None:
        d.dst_layout = L.DST_NCTHW
    else:
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, cl[0], cl[1], t * crop * crop * cl[1]
    call("pv_yuv_views", d)
    return dst, n


def _resampled(rgb, table, size, crop, idxs, affine=True):
    """[N, 3, Hs, Ws] virtual RGB frames -> planar [n_clips * n_views, 3, T, crop, crop] by the pinned formula; table
    entries are clamped into the frames as the kernel clamps them."""
    n, _, hs, ws = rgb.shape
    clips = rgb[table.long().clamp(0, n - 1)].permute(0, 2, 1, 3, 4)               # [n_clips, 3, T, Hs, Ws]
    hn, wn = TR.scaled_size(hs, ws, size)
    scale, shift = SU.affine() if affine else (None, None)
    out = []
    for v in idxs:
        y, x = TR.crop_offsets(hn, wn, crop, v)
        out.append(SU.pinned_resample(clips, hn, wn, y, x, crop, crop, scale, shift))
    return torch.stack(out, dim=1).reshape(table.shape[0] * len(idxs), 3, table.shape[1], crop, crop)


def _reference(frames_cpu, layout, matrix, table, size, crop, idxs, affine=True, **geom_kw):
    rgb = TR.yuv420_to_rgb(frames_cpu, layout, matrix.float().double(), **geom_kw)
    return _resampled(rgb, table, size, crop, idxs, affine)


def _planar_of(dst, form, n):
    """The written items as planar [n, 3, T, crop, crop] fp32 on the CPU, after checking what surrounds them: pad channels
    zero, bytes beyond c_p and items behind the window untouched."""
    assert torch.all(dst[n:] == SENTINEL), "items behind the window were written"
    if form == "planar":
        return dst[:n].float().cpu()
    c_p = 4 if form == "c4" else 8
    assert torch.all(dst[:n, ..., 3:c_p] == 0), "pad channels are zero"
    assert torch.all(dst[:n, ..., c_p:] == SENTINEL), "bytes beyond c_p were written"
    return dst[:n, ..., :3].permute(0, 4, 1, 2, 3).float().cpu()


def _check(got, ref, hs, ws, max_scale, bf16, what, extra=0.0):
    got, ref = got.float().cpu(), ref.float()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    tol = SU.bound(ref, hs, ws, max_scale, bf16) + TAP * max_scale + extra
    worst = err.max().item()
    print("%s: worst |d| %.3e, smallest bound %.3e, |ref| max %.3f" % (what, worst, tol.min().item(), ref.abs().max().item()))
    assert bool((err <= tol).all()), "%s: %d elements over the bound, worst %.3e" % (what, int((err > tol).sum()), worst)


FORMS = [("c4", torch.bfloat16), ("cl8", torch.float32), ("cl8_ld16", torch.bfloat16), ("planar", torch.bfloat16),
         ("planar", torch.float32)]
# 2 rows x 5: a repeated frame, and entries that leave the 10 frames and must clamp
TABLE = torch.tensor([[0, 2, 2, -3, 9], [7, 99, 4, 5, 1]], dtype=torch.int32)


@pytest.fixture(scope="module")
def video10():
    """Planes of a 10-frame 98 x 132 video and, per (packing, matrix), the reference shared by the destination forms."""
    y, u, v = YU.planes(10, 98, 132, 1200)
    cache = {}

    def reference(layout, matrix_name):
        if (layout, matrix_name) not in cache:
            m = {"bt601_limited": M601, "bt709_full": M709F}[matrix_name]
            frames = YU.pack(y, u, v, layout).frames()
            cache[(layout, matrix_name)] = (frames.cuda(), m, _reference(frames, layout, m, TABLE, 64, 56, (0, 1, 2)))
        return cache[(layout, matrix_name)]
    return reference


@pytest.mark.parametrize("form,dtype", FORMS, ids=["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS])
@pytest.mark.parametrize("matrix_name", ["bt601_limited", "bt709_full"])
@pytest.mark.parametrize("layout", ["NV12", "I420"])
def test_yuv_views_forms_and_packings(video10, layout, matrix_name, form, dtype):
    frames, m, want = video10(layout, matrix_name)
    dst, n = _run(frames, layout, TABLE, 64, 56, (0, 1, 2), form, dtype, m, extra=2)
    assert n == 6
    _check(_planar_of(dst, form, n), want, 98, 132, MAX_SCALE, dtype == torch.bfloat16, "%s %s %s %s" % (layout, matrix_name, form, dtype))


@pytest.mark.parametrize("layout", ["NV21", "YV12"])
def test_yuv_views_swapped_chroma_packings(video10, layout):
    """NV21 and YV12 are NV12 and I420 with U and V exchanged: the same reference, bit for bit the same output."""
    y, u, v = YU.planes(10, 98, 132, 1200)
    twin = "NV12" if layout == "NV21" else "I420"
    frames, m, want = video10(twin, "bt601_limited")
    dst, n = _run(YU.pack(y, u, v, layout).frames("cuda"), layout, TABLE, 64, 56, (0, 1, 2), "planar", torch.float32, m)
    ref, _ = _run(frames, twin, TABLE, 64, 56, (0, 1, 2), "planar", torch.float32, m)
    assert torch.equal(dst, ref)
    _check(_planar_of(dst, "planar", n), want, 98, 132, MAX_SCALE, False, layout)


@pytest.mark.parametrize("layout,pitch", [("NV12", 25), ("NV21", 25), ("I420", 26)], ids=["NV12_pitch25", "NV21_pitch25", "I420_pitch26"])
def test_yuv_views_odd_alignment_pitch_coded_height_and_upscaling(layout, pitch):
    """30 x 22 frames with a row pitch of W + 3 (planar chroma rows have half the luma pitch, so I420 takes W + 4), coded
    height 32, the base at an odd address, scaled up to 41 and cropped to 37.  Whatever lies in the pitch padding, in the
    rows between the display and the coded height and in their chroma must not matter: two runs with different garbage
    there are bit-identical."""
    y, u, v = YU.planes(4, 30, 22, 1201)
    table = torch.tensor([[0, 1, 2, 3], [3, 3, 0, 2]], dtype=torch.int32)
    outs = []
    for garbage in (31, 32):
        packed = YU.pack(y, u, v, layout, coded_height=32, pitch=pitch, base=1, garbage=garbage)
        frames = packed.frames("cuda")
        assert frames.data_ptr() % 2 == 1 and frames.stride() == (48 * pitch, pitch, 1)
        for form, dtype in (("planar", torch.float32), ("c4", torch.bfloat16)):
            dst, n = _run(frames, layout, table, 41, 37, (0, 1, 2), form, dtype, M601, height=30, coded_height=32)
            outs.append(dst)
            if garbage == 31:
                want = _reference(packed.frames(), layout, M601, table, 41, 37, (0, 1, 2), height=30, coded_height=32)
                _check(_planar_of(dst, form, n), want, 30, 22, MAX_SCALE, dtype == torch.bfloat16, "%s pitch %d %s" % (layout, pitch, form))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1].view(torch.int16), outs[3].view(torch.int16))


@pytest.mark.parametrize("layout", ["NV12", "I420"])
def test_yuv_views_sparse_staging(layout):
    """256 x 340 -> 64 / 56: a strip's source rows are more than the dense run holds, so every output row stages its own
    two luma rows and their chroma rows."""
    y, u, v = YU.planes(3, 256, 340, 1202)
    table = torch.tensor([[2, 0], [1, 1]], dtype=torch.int32)
    frames = YU.pack(y, u, v, layout).frames()
    want = _reference(frames, layout, M601, table, 64, 56, (0, 1, 2))
    for form, dtype in (("planar", torch.bfloat16), ("cl8", torch.float32)):
        dst, n = _run(frames.cuda(), layout, table, 64, 56, (0, 1, 2), form, dtype, M601)
        _check(_planar_of(dst, form, n), want, 256, 340, MAX_SCALE, dtype == torch.bfloat16, "%s sparse %s" % (layout, form))


@pytest.mark.parametrize("layout", ["NV12", "I420"])
def test_yuv_views_720p_three_views(layout):
    """The geometry people run: 720 x 1280 -> short side 256, three 224 crops, 3 frames."""
    y, u, v = YU.planes(3, 720, 1280, 1203)
    table = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    frames = YU.pack(y, u, v, layout).frames()
    want = _reference(frames, layout, M709F, table, 256, 224, (0, 1, 2))
    dst, n = _run(frames.cuda(), layout, table, 256, 224, (0, 1, 2), "planar", torch.bfloat16, M709F)
    _check(_planar_of(dst, "planar", n), want, 720, 1280, MAX_SCALE, True, "%s 720p" % layout)


@pytest.mark.parametrize("form,dtype", [("planar", torch.float32), ("c4", torch.bfloat16)], ids=["planar_f32", "c4_bf16"])
def test_yuv_views_item_ranges(form, dtype):
    """2 clips x 3 views: every window writes only its range, and the windows together are the whole, bit for bit."""
    y, u, v = YU.planes(6, 50, 68, 1204)
    frames = YU.pack(y, u, v, "NV12").frames("cuda")
    table = torch.tensor([[0, 2, 4], [5, 3, 1]], dtype=torch.int32)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    whole, n = _run(frames, "NV12", table, 32, 28, (0, 1, 2), form, dtype, M601, 0, 6)
    assert n == 6 and torch.all(whole[6:] == SENTINEL) and not torch.any(torch.all(whole[:6].flatten(1) == SENTINEL, dim=1))
    implied, _ = _run(frames, "NV12", table, 32, 28, (0, 1, 2), form, dtype, M601, 0, 0)     # n_items == 0: all
    assert torch.equal(implied.view(bits), whole.view(bits))
    for item0, cnt in ((1, 4), (5, 1)):
        part, n = _run(frames, "NV12", table, 32, 28, (0, 1, 2), form, dtype, M601, item0, cnt, extra=2)
        assert n == cnt and torch.all(part[cnt:] == SENTINEL)
        assert torch.equal(part[:cnt].view(bits), whole[item0:item0 + cnt].view(bits)), (item0, cnt)


def test_yuv_views_ties_to_the_rgb_kernel():
    """The same frames as an RGB copy -- the mirror rounded to the nearest uint8, [N,H,W,3] -- through pv_video_views, the
    kernel the suite pins to the reference: the integer rounding of the copy (at most 0.5 per tap, times the affine scale)
    is the only modelled difference, on top of the two kernels' own bounds."""
    from gpu_util import call
    y, u, v = YU.planes(6, 98, 132, 1205)
    table = torch.tensor([[0, 2, 4], [5, 3, 3]], dtype=torch.int32)
    frames = YU.pack(y, u, v, "NV12").frames()
    mirror = TR.yuv420_to_rgb(frames, "NV12", M601.float().double())
    rgb_u8 = torch.round(mirror).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()      # [N, H, W, 3]
    got, n = _run(frames.cuda(), "NV12", table, 64, 56, (0, 1, 2), "planar", torch.float32, M601)
    tab = table.cuda()
    scale, shift = [x.cuda() for x in SU.affine()]
    hn, wn = TR.scaled_size(98, 132, 64)
    d = L.VideoViewsDesc()
    d.src, d.t_index, d.ch_scale, d.ch_shift = rgb_u8.data_ptr(), tab.data_ptr(), scale.data_ptr(), shift.data_ptr()
    d.n_clips, d.C, d.T, d.N, d.t_stride, d.Hs, d.Ws = 2, 3, 3, 6, 3, 98, 132
    d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NTHWC
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = hn, wn, 56, 56, 3
    for i in range(3):
        d.y_off[i], d.x_off[i] = TR.crop_offsets(hn, wn, 56, i)
    old = torch.full((6, 3, 3, 56, 56), SENTINEL, dtype=torch.float32, device="cuda")
    d.dst, d.dst_layout, d.dst_dtype = old.data_ptr(), L.DST_NCTHW, L.PV_F32
    call("pv_video_views", d)
    got, old = got[:n].cpu(), old.cpu()
    want = _resampled(mirror, table, 64, 56, (0, 1, 2))
    tol = 0.5 * MAX_SCALE + 2 * SU.bound(want, 98, 132, MAX_SCALE) + TAP * MAX_SCALE
    err = (got - old).abs()
    print("yuv vs rgb copy: worst |d| %.3e of %.3e allowed" % (err.max().item(), tol.min().item()))
    assert bool((err <= tol).all()), "%d elements over the bound, worst %.3e" % (int((err > tol).sum()), err.max().item())
    assert err.max().item() > 4 * TAP * MAX_SCALE           # the copy WAS rounded: the two paths are not the same arithmetic


def test_yuv_views_clamps_every_tap_before_the_blend():
    """A frame of (Y, U, V) corners, far out of gamut, equals the CLAMPED mirror -- and neither a clamp behind the blend nor
    no clamp at all would: both alternatives are computed here and lie outside the bound."""
    g = torch.Generator().manual_seed(1206)
    y, u, v = [torch.randint(0, 2, s, generator=g, dtype=torch.uint8) * 255 for s in ((2, 32, 44), (2, 16, 22), (2, 16, 22))]
    table = torch.tensor([[0, 1]], dtype=torch.int32)
    for layout in ("NV12", "I420"):
        frames = YU.pack(y, u, v, layout).frames()
        want = _reference(frames, layout, M601, table, 41, 37, (1,), affine=False)
        dst, n = _run(frames.cuda(), layout, table, 41, 37, (1,), "planar", torch.float32, M601, affine=False)
        _check(dst[:n], want, 32, 44, 1.0, False, "%s corners" % layout)
        assert want.min().item() >= 0.0 and want.max().item() <= 255.0
    m = M601.float().double()
    up = [c.double().repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v)]
    raw = torch.stack([m[c, 0] * y.double() + m[c, 1] * up[0] + m[c, 2] * up[1] + m[c, 3] for c in range(3)], dim=1).float()
    assert raw.min().item() < -100 and raw.max().item() > 400
    unclamped = _resampled(raw, table, 41, 37, (1,), affine=False)
    tol = SU.bound(want, 32, 44, 1.0) + TAP
    assert bool(((unclamped - want).abs() > 100 * tol).any())
    assert bool(((torch.clamp(unclamped, 0, 255) - want).abs() > 100 * tol).any())


# ----------------------------------------------------------------------------- models
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)


def _deploy(m, x, dtype=torch.bfloat16, **kw):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    transmute_model(m, "mi355x")
    xd = [t.cuda().to(dtype) for t in x] if isinstance(x, list) else x.cuda().to(dtype)
    return convert_to_deployable_form(m, xd, dtype=dtype, **kw)


def _x3d(batch, dtype=torch.bfloat16):
    """x3d_xs (4 x 160 x 160, 400 classes) converted for `batch` items."""
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    m = trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()
    return _deploy(m, seeded_input((batch, 3, 4, 160, 160), 6), dtype)


def _nv12_video(n, hs, ws, seed, **kw):
    return YU.pack(*YU.planes(n, hs, ws, seed), "NV12", **kw).frames("cuda")


def _composed(dep, video, table, batch, short_side, crop, views, dtype, frame_ratios=None, **yuv_kw):
    """The composed path: YUV clips materialised by index_select, `device_scale_crop(..., src_layout="NV12")` once per
    pathway, the views fed to the same deploy form `batch` items at a time (the last batch padded with items that are
    never folded), `VideoEnsembler`.  (video scores, clip scores)."""
    n_clips, t = table.shape
    n_views = len(views)
    clips = video.index_select(0, table.reshape(-1).long().to(video.device)).view(n_clips, t, *video.shape[1:])
    ratios = frame_ratios or (1,)
    paths = [TR.device_scale_crop(clips, short_side, crop, views, num_frames=t // r, dtype=dtype, src_layout="NV12", **KW, **yuv_kw)
             for r in ratios]
    total = n_clips * n_views
    ve = ce = None
    for i0 in range(0, total, batch):
        k = min(batch, total - i0)
        x = [torch.cat([p[i0:i0 + k], torch.full((batch - k,) + tuple(p.shape[1:]), 2.0, dtype=p.dtype, device=p.device)])
             for p in paths]
        logits = dep(x if frame_ratios else x[0])[:k].clone()
        if ve is None:
            ve, ce = VideoEnsembler(1, logits.shape[1], "sum"), VideoEnsembler(n_clips, logits.shape[1], "sum")
        ve.update(logits, [0] * k)
        ce.update(logits, [(i0 + i) // n_views for i in range(k)])
    return ve.result()[0].clone(), ce.result().clone()


def _check_predictor(dep, sampler, video, fps, batch, short_side, crop, views, dtype, frame_ratios=None, **yuv_kw):
    pred = VideoPredictor(dep, sampler, short_side=short_side, crop_size=crop, spatial_idx=views, frame_ratios=frame_ratios,
                          src_layout="NV12", **KW, **yuv_kw)
    assert pred.packer.batch == batch
    table, _ = D.clip_frame_table(sampler, video.shape[0], fps, pred.packer.clip_frames)
    scores, clip_scores = pred(video, fps, return_clip_scores=True)
    scores, clip_scores = scores.clone(), clip_scores.clone()
    n_clips, n_views = table.shape[0], len(views)
    assert int(pred.video_ensembler.counts.item()) == n_clips * n_views
    assert (n_clips * n_views) % batch != 0, "the case is meant to end in a ragged chunk"
    want, want_clips = _composed(dep, video, table, batch, short_side, crop, views, dtype, frame_ratios, **yuv_kw)
    assert torch.equal(scores, want), "video scores differ by %.3e" % (scores - want).abs().max().item()
    assert torch.equal(clip_scores, want_clips), "clip scores differ by %.3e" % (clip_scores - want_clips).abs().max().item()
    assert not torch.equal(clip_scores[0], clip_scores[-1])      # the clips are different frames
    return pred


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16_plan", "fp32_plan"])
def test_predictor_x3d_on_an_nv12_video(dtype):
    """x3d_xs, batch 6 = 2 clips x 3 views; a 40-frame 64 x 86 NV12 video (a pitched surface with a coded height of 72) at
    10 fps, 5 clips of 8 frames subsampled to 4: 15 items = 6 + 6 + 3.  Then a batch of materialised clips."""
    dep = _x3d(6, dtype)
    video = _nv12_video(40, 64, 86, 1210, coded_height=72, pitch=96, base=1, garbage=9)
    assert not video.is_contiguous()
    geom = dict(coded_height=72, height=64)
    pred = _check_predictor(dep, D.ConstantClipsPerVideoSampler(Fraction(8, 10), 5), video, 10, 6, 176, 160, (0, 1, 2), dtype, **geom)
    assert bool(pred.packer._planar) == (dtype == torch.bfloat16)
    # [B, T', Hc*3/2, W] clips through DevicePacker.__call__: frames 8..15 of the surface, in place, as 2 clips of 4
    clips = torch.as_strided(video, (2, 4) + tuple(video.shape[1:]), (4 * video.stride(0),) + tuple(video.stride()),
                             video.storage_offset() + 8 * video.stride(0))
    packer = TR.DevicePacker(dep, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), src_layout="NV12", **KW, **geom)
    logits = packer(clips).clone()
    views = TR.device_scale_crop(clips, 176, 160, (0, 1, 2), dtype=dtype, src_layout="NV12", **KW, **geom)
    assert tuple(views.shape) == (6, 3, 4, 160, 160)
    assert torch.equal(logits, dep(views).clone())
    with pytest.raises(RuntimeError):
        packer(clips[:1])                                        # 1 clip x 3 views is not the batch of 6


def test_predictor_slowfast_on_an_nv12_video():
    """slowfast_r50_small (4 + 16 frames at 96 x 96), frame_ratios (4, 1), batch 4 = 2 clips x 2 views: both pathways read the
    NV12 frames through column subsets of one table.  3 clips of 24 frames -> 6 items = 4 + 2."""
    from oracle.weights import deterministic_fill, seeded_input
    from pytorchvideo_amd.models import create_slowfast
    g = torch.load(os.path.join(GOLD, "slowfast_r50_small.pt"), weights_only=False)
    m = deterministic_fill(create_slowfast(**g["cfg"]), g["seed"]).eval()
    fast = seeded_input((4, 3, 16, 96, 96), 7)
    dep = _deploy(m, [TR.uniform_temporal_subsample(fast, 4, 2), fast])
    video = _nv12_video(40, 64, 86, 1211)
    pred = _check_predictor(dep, D.ConstantClipsPerVideoSampler(Fraction(24, 20), 3, 2), video, 20, 4, 100, 96, (0, 2),
                            torch.bfloat16, frame_ratios=(4, 1))
    assert pred.packer.clip_frames == 16


def test_a_detection_model_is_refused_with_the_reason():
    from oracle.weights import detection_fill
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_resnet_with_roi_head
    g = torch.load(os.path.join(GOLD, "resnet_det_r50_small.pt"), weights_only=False)
    m = detection_fill(create_resnet_with_roi_head(**g["cfg"]), g["seed"]).eval()
    transmute_model(m, "mi355x")
    x = SU.normalised(SU.clip((3, 4, 64, 64), 916))[None].repeat(2, 1, 1, 1, 1)
    dm = convert_to_deployable_form(m, (x.cuda().bfloat16(), g["boxes"]), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="detection model's boxes belong to key frames .*NV12"):
        VideoPredictor(dm, D.UniformClipSampler(1), short_side=72, crop_size=64, src_layout="NV12", **KW)
    with pytest.raises(ValueError, match="detection model does not take I420 frames: its boxes"):
        TR.DevicePacker(dm, short_side=72, crop_size=64, src_layout="I420", **KW)
