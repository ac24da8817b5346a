"""A rectangle per frame on the MI355X: `pv_region_views` (include/pv_mi355x.h "a rectangle per frame"),
`transforms.device_resized_crop`, `DevicePacker.video_batch(regions=)` and `inference.TubePredictor`.

Reference, bit for bit (`torch.equal` on the raw bits, no tolerance): the EXISTING `pv_batch_views` on a dense one-frame copy
of every rectangle, given as a source of its own with Hn = Ho, Wn = Wo and offsets 0 -- the header's guarantee -- which the
existing suite already holds against the reference's fixtures.  The host mirror `transforms.resized_crop` and the reference's
own `random_resized_crop` (tests/golden/region_transforms.pt) bound the transform from the other side, within
`spatial_util.bound`.  No test feeds the device a rectangle or a table entry that leaves its video."""
import ctypes as C
import os

import pytest
import torch

import spatial_util as SU
import test_gpu_batch_views as BV
import yuv16_util as Y16
import yuv_util as YU
from make_region_golden import CASES, SHAPE, clip
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import TubePredictor

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = BV.SENTINEL
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)
HO = WO = 16
FORMS = BV.FORMS                                                 # the FORMS of tests/test_gpu_resample.py
FORM_IDS = ["%s_%s" % (f, "bf16" if t == torch.bfloat16 else "f32") for f, t in FORMS]
PLANE_FIELDS = ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch")


# ----------------------------------------------------------------------------- launches
def _fill_batch_desc(d, n_rows, t_stride, t, codes, c_step, matrix, window):
    d.n_rows, d.t_stride, d.C, d.T = n_rows, t_stride, 3, t
    d.src_layout, d.src_dtype = codes
    if matrix is not None:
        d.c_step, d.yuv2rgb = c_step, matrix.data_ptr()
    d.Ho, d.Wo, d.n_views = window[0], window[1], 1


def _records(recs):
    """`recs`: one dict per source -- src (an address), N, Hs, Ws and, for YUV, the plane fields.  The view geometry of a
    record (Hn, Wn, the offsets, sy, sx) is left zero here: pv_region_views does not read it."""
    sources = (L.ViewSource * len(recs))()
    for rec, r in zip(sources, recs):
        for k, v in r.items():
            setattr(rec, k, v)
    return sources


def _region_launch(recs, codes, table, regions, pairs, form, dtype, c_step=0, matrix=None, ptrs=None, extra=2):
    """pv_region_views over the sources `recs` for the items `pairs` = (source, table row) into a sentinel-filled destination
    of `extra` more items than the launch writes.  `table` int32 [rows, T] and `regions` int64 [rows, T, 4] on the host;
    `ptrs`: the int64 pointer table of a frame-list launch (a record's src is then an INDEX into it)."""
    from gpu_util import call
    g = L.RegionViewsDesc()
    d = g.frames.batch
    tab = table.to(torch.int32).contiguous().cuda()
    host = TR.region_records(TR._check_regions(regions, 1 << 20, 1 << 20), (HO, WO))
    dev = host.cuda()
    keep = [tab, host, dev]
    if ptrs is not None:
        ptrs_dev = ptrs.cuda()
        keep.append(ptrs_dev)
        g.frames.frame_ptrs, g.frames.frame_ptrs_dev, g.frames.n_frame_ptrs = ptrs.data_ptr(), ptrs_dev.data_ptr(), ptrs.numel()
        recs = [dict(r, src=ptrs_dev.data_ptr() + 8 * r["src"]) for r in recs]
    sources, items = _records(recs), BV._items([(s, r, 0) for s, r in pairs])
    keep += [BV._upload(sources), BV._upload(items)] + [x.cuda() for x in SU.affine()]
    d.sources, d.sources_dev = C.addressof(sources), keep[-4].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[-3].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.ch_scale, d.ch_shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    d.t_index = tab.data_ptr()
    _fill_batch_desc(d, tab.shape[0], tab.shape[1], tab.shape[1], codes, c_step, matrix, (HO, WO))
    g.regions, g.regions_dev = host.data_ptr(), dev.data_ptr()
    dst, cl = BV._destination(form, dtype, len(items) + extra, 3, tab.shape[1], HO)
    BV._set_destination(d, dst, cl, dtype, tab.shape[1], HO)
    call("pv_region_views", g)
    return dst


def _dense_launch(recs, codes, form, dtype, c_step=0, matrix=None):
    """The oracle: ONE launch of the existing pv_batch_views over dense one-frame sources (`recs`, each with its tensor kept
    alive by the caller), item k = source k, with Hn = Ho, Wn = Wo and offsets 0."""
    from gpu_util import call
    for r in recs:
        r.update(N=1, Hn=HO, Wn=WO, sy=BV._f32(r["Hs"], HO), sx=BV._f32(r["Ws"], WO))
    sources, items = _records(recs), BV._items([(k, 0, 0) for k in range(len(recs))])
    tab = torch.zeros((1, 1), dtype=torch.int32).cuda()
    keep = [BV._upload(sources), BV._upload(items)] + [x.cuda() for x in SU.affine()]
    d = L.BatchViewsDesc()
    d.sources, d.sources_dev = C.addressof(sources), keep[0].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[1].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    d.ch_scale, d.ch_shift = keep[2].data_ptr(), keep[3].data_ptr()
    d.t_index = tab.data_ptr()
    _fill_batch_desc(d, 1, 1, 1, codes, c_step, matrix, (HO, WO))
    dst, cl = BV._destination(form, dtype, len(items), 3, 1, HO)
    BV._set_destination(d, dst, cl, dtype, 1, HO)
    call("pv_batch_views", d)
    return dst


def _frame_of(dst, form, i, t):
    """Destination frame t of item i: [C, Ho, Wo] of a planar destination, [Ho, Wo, ld] of a channels-last one."""
    return dst[i, :, t] if form == "planar" else dst[i, t]


def _check_against_dense(got, want, pairs, table, form, what):
    """`want` holds one item per (item, t) of the launch, in that order."""
    k = 0
    for i in range(len(pairs)):
        for t in range(table.shape[1]):
            assert BV._same_bits(_frame_of(got, form, i, t), _frame_of(want, form, k, 0)), "%s: item %d frame %d" % (what, i, t)
            k += 1
    assert not torch.all(got[:len(pairs)] == SENTINEL), what
    assert torch.all(got[len(pairs):] == SENTINEL), "items behind the launch were written: " + what


# ----------------------------------------------------------------------------- RGB / planar sources
SIZES = [(6, 38, 54), (5, 46, 34), (4, 128, 96)]
# row -> (source, frames, a rectangle per frame): rectangles that move and change size; 1 x 1 (a corner pixel and the
# bottom-right one), the full frame, rectangles that end at the bottom-right pixel, odd widths, the 9 x 5 upscale, the identity
# size 16 x 16, one-pixel rows and columns, and on the 128 x 96 video h / Ho > 2: the strip's source rows are staged in pairs
ROWS = [
    (0, [0, 2, 5, 3], [(0, 0, 1, 1), (0, 0, 38, 54), (30, 41, 8, 13), (5, 7, 16, 16)]),
    (0, [1, 1, 4, 0], [(37, 53, 1, 1), (3, 4, 9, 5), (10, 3, 21, 33), (22, 38, 16, 16)]),
    (1, [4, 0, 2, 2], [(0, 0, 46, 34), (11, 9, 7, 25), (45, 0, 1, 34), (0, 33, 46, 1)]),
    (2, [0, 3, 1, 2], [(4, 3, 120, 90), (0, 0, 128, 96), (100, 60, 28, 36), (8, 6, 40, 35)]),
]
PAIRS = [(0, 0), (2, 3), (1, 2), (0, 1), (2, 3)]                 # sources interleaved, one item twice
TABLE = torch.tensor([r[1] for r in ROWS], dtype=torch.int32)
REGIONS = torch.tensor([r[2] for r in ROWS], dtype=torch.int64)


def _codes(layout, dtype):
    return (L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC, L.PV_U8 if dtype == torch.uint8 else L.PV_F32)


def _rgb_rec(src, layout):
    c, n, hs, ws = TR._video_geometry(src, layout)
    return dict(src=src.data_ptr(), N=n, Hs=hs, Ws=ws)


def _rgb_dense(src, layout, frame, rect):
    top, left, h, w = rect
    if layout == "NTHWC":
        one = src[frame, top:top + h, left:left + w].contiguous()
    else:
        one = src[:, frame:frame + 1, top:top + h, left:left + w].contiguous()
    return dict(src=one.data_ptr(), Hs=h, Ws=w, keep=one)


def _dense_recs(recs):
    return [{k: v for k, v in r.items() if k != "keep"} for r in recs]


@pytest.fixture(scope="module")
def videos():
    return [SU.clip((3, n, h, w), 2100 + i) for i, (n, h, w) in enumerate(SIZES)]


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("layout,src_dtype", BV.SOURCES, ids=["planar_u8", "planar_f32", "interleaved_u8"])
def test_region_views_writes_the_bits_of_batch_views_on_a_dense_copy_of_every_rectangle(videos, layout, src_dtype, form, dtype):
    srcs = [BV._source(v, layout, src_dtype) for v in videos]
    recs = [_rgb_rec(s, layout) for s in srcs]
    got = _region_launch(recs, _codes(layout, src_dtype), TABLE, REGIONS, PAIRS, form, dtype)
    dense = [_rgb_dense(srcs[s], layout, int(TABLE[r, t]), REGIONS[r, t].tolist()) for s, r in PAIRS for t in range(TABLE.shape[1])]
    assert any(d["Hs"] > 2 * HO for d in dense) and any(d["Hs"] < HO for d in dense)      # sparse and dense staging
    want = _dense_launch(_dense_recs(dense), _codes(layout, src_dtype), form, dtype)
    _check_against_dense(got, want, PAIRS, TABLE, form, "%s %s -> %s %s" % (layout, src_dtype, form, dtype))


# ----------------------------------------------------------------------------- YUV sources
YUV_ROWS = [
    (0, [0, 3, 1], [(0, 0, 2, 2), (0, 0, 38, 54), (30, 42, 8, 12)]),
    (0, [2, 2, 0], [(36, 52, 2, 2), (4, 6, 10, 6), (8, 2, 16, 16)]),
    (1, [1, 0, 2], [(2, 4, 124, 90), (0, 0, 128, 96), (100, 60, 28, 36)]),
]
YUV_PAIRS = [(1, 2), (0, 0), (0, 1), (1, 2)]
YUV_TABLE = torch.tensor([r[1] for r in YUV_ROWS], dtype=torch.int32)
YUV_REGIONS = torch.tensor([r[2] for r in YUV_ROWS], dtype=torch.int64)
M601 = TR.yuv_matrix("bt601", False)
M709F_P010 = TR.yuv_matrix("bt709", True, 10, True)


def _yuv_sources(layout):
    """Two videos as decoder surfaces: 38 x 54 pitched with a coded height above the display height (and, for the 8-bit
    interleaved forms, at an odd base address), 128 x 96 tight.  Returns (planes, device frames, geometries, module)."""
    wide = layout in TR.YUV16_LAYOUTS
    mod = Y16 if wide else YU
    pl = [Y16.planes(4, 38, 54, 2301, shift=6), Y16.planes(3, 128, 96, 2302, shift=6)] if wide else \
        [YU.planes(4, 38, 54, 2301), YU.planes(3, 128, 96, 2302)]
    base = 2 if wide or layout == "I420" else 3
    first = mod.pack(*pl[0], layout, coded_height=48, pitch=64, base=base, garbage=9).frames("cuda")
    second = mod.pack(*pl[1], layout).frames("cuda")
    geoms = [TR.yuv_geometry(first, layout, coded_height=48, height=38), TR.yuv_geometry(second, layout)]
    return pl, [first, second], geoms, mod


def _yuv_rec(frames, geom):
    return dict(src=frames.data_ptr(), N=geom["N"], Hs=geom["Hs"], Ws=geom["Ws"], **{k: geom[k] for k in PLANE_FIELDS})


def _yuv_dense(planes, mod, layout, frame, rect):
    """A dense, tight 4:2:0 copy of the rectangle: the Y rows / columns cut, chroma at half."""
    top, left, h, w = rect
    y, u, v = planes
    one = mod.pack(y[frame:frame + 1, top:top + h, left:left + w], u[frame:frame + 1, top // 2:(top + h) // 2, left // 2:(left + w) // 2],
                   v[frame:frame + 1, top // 2:(top + h) // 2, left // 2:(left + w) // 2], layout).frames("cuda")
    geom = TR.yuv_geometry(one, layout)
    assert (geom["Hs"], geom["Ws"]) == (h, w)
    return dict(src=one.data_ptr(), Hs=h, Ws=w, keep=one, **{k: geom[k] for k in PLANE_FIELDS})


@pytest.mark.parametrize("layout", ["NV12", "NV21", "I420", "P010"])
def test_region_views_yuv_writes_the_bits_of_batch_views_on_a_dense_copy(layout):
    planes, frames, geoms, mod = _yuv_sources(layout)
    wide = layout in TR.YUV16_LAYOUTS
    codes = (L.SRC_YUV420, L.PV_U16 if wide else L.PV_U8)
    matrix = (M709F_P010 if wide else M601).float().reshape(12).cuda()
    c_step = geoms[0]["c_step"]
    recs = [_yuv_rec(f, g) for f, g in zip(frames, geoms)]
    dense = [_yuv_dense(planes[s], mod, layout, int(YUV_TABLE[r, t]), YUV_REGIONS[r, t].tolist())
             for s, r in YUV_PAIRS for t in range(YUV_TABLE.shape[1])]
    for form, dtype in (("c4", torch.bfloat16), ("cl8", torch.float32), ("cl16", torch.float32), ("planar", torch.bfloat16),
                        ("planar", torch.float32)):
        got = _region_launch(recs, codes, YUV_TABLE, YUV_REGIONS, YUV_PAIRS, form, dtype, c_step, matrix)
        want = _dense_launch(_dense_recs(dense), codes, form, dtype, c_step, matrix)
        _check_against_dense(got, want, YUV_PAIRS, YUV_TABLE, form, "%s -> %s %s" % (layout, form, dtype))


# ----------------------------------------------------------------------------- frame lists
def _pointer_table(per_video_frames):
    """(int64 table, first index per video) of the frame tensors, video-major."""
    ptrs = torch.tensor([f.data_ptr() for frames in per_video_frames for f in frames], dtype=torch.int64)
    first, k = [], 0
    for frames in per_video_frames:
        first.append(k)
        k += len(frames)
    return ptrs, first


@pytest.mark.parametrize("kind", ["interleaved_u8", "planar_f32", "NV12", "P010"])
def test_a_frame_list_gives_the_bits_of_the_stacked_video(videos, kind):
    """The same items with every frame addressed through the pointer table (`frame_ptrs`) equal the whole-video launch."""
    if kind in ("NV12", "P010"):
        _, frames, geoms, _ = _yuv_sources(kind)
        codes = (L.SRC_YUV420, L.PV_U16 if kind == "P010" else L.PV_U8)
        matrix = (M709F_P010 if kind == "P010" else M601).float().reshape(12).cuda()
        c_step, recs = geoms[0]["c_step"], [_yuv_rec(f, g) for f, g in zip(frames, geoms)]
        lists = [list(f.unbind(0)) for f in frames]              # every surface where it lies
        table, regions, pairs = YUV_TABLE, YUV_REGIONS, YUV_PAIRS
    else:
        layout, src_dtype = ("NTHWC", torch.uint8) if kind == "interleaved_u8" else ("NCTHW", torch.float32)
        srcs = [BV._source(v, layout, src_dtype) for v in videos]
        codes, matrix, c_step, recs = _codes(layout, src_dtype), None, 0, [_rgb_rec(s, layout) for s in srcs]
        # every frame an allocation of its own; a planar frame of a list is a dense [C, Hs, Ws]
        lists = [[f.clone(memory_format=torch.contiguous_format) for f in s.unbind(1 if layout == "NCTHW" else 0)] for s in srcs]
        table, regions, pairs = TABLE, REGIONS, PAIRS
    ptrs, first = _pointer_table(lists)
    listed = [dict(r, src=k) for r, k in zip(recs, first)]
    for form, dtype in (("c4", torch.bfloat16), ("planar", torch.float32)):
        whole = _region_launch(recs, codes, table, regions, pairs, form, dtype, c_step, matrix)
        got = _region_launch(listed, codes, table, regions, pairs, form, dtype, c_step, matrix, ptrs=ptrs)
        assert BV._same_bits(got, whole), (kind, form, dtype)
        assert not torch.all(got[:len(pairs)] == SENTINEL)


# ----------------------------------------------------------------------------- sharing a launch
@pytest.mark.parametrize("layout,src_dtype", [("NTHWC", torch.uint8), ("NCTHW", torch.uint8)], ids=["interleaved_u8", "planar_u8"])
def test_an_item_holds_the_same_bits_whatever_shares_its_launch(videos, layout, src_dtype):
    """Items of different sources and rectangle sizes in one launch -- sized for the widest rectangle of all of them -- equal
    each item launched alone, sized for its own; and a launch writes its n_items and nothing behind them."""
    srcs = [BV._source(v, layout, src_dtype) for v in videos]
    recs = [_rgb_rec(s, layout) for s in srcs]
    for form, dtype in (("cl8", torch.bfloat16), ("planar", torch.bfloat16)):
        got = _region_launch(recs, _codes(layout, src_dtype), TABLE, REGIONS, PAIRS, form, dtype, extra=2)
        assert torch.all(got[len(PAIRS):] == SENTINEL) and got.shape[0] == len(PAIRS) + 2
        for i, pair in enumerate(PAIRS):
            alone = _region_launch(recs, _codes(layout, src_dtype), TABLE, REGIONS, [pair], form, dtype, extra=1)
            assert BV._same_bits(alone[0], got[i]), (layout, form, i)
            assert torch.all(alone[1:] == SENTINEL)


# ----------------------------------------------------------------------------- the host mirror
@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLD, "region_transforms.pt"), weights_only=False)


def _case_regions(rects, t):
    if len(rects) == 1:
        return torch.tensor(rects[0]).expand(t, 4)
    return torch.tensor([[int(v) for v in torch.linspace(a, b, steps=t).tolist()] for a, b in zip(*rects)]).T.contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_device_resized_crop_against_the_host_mirror_and_the_reference(gold, dtype):
    bf16 = dtype == torch.bfloat16
    for case, (rects, size) in enumerate(CASES):
        x = clip(600 + case)
        regions = _case_regions(rects, SHAPE[1])
        got = TR.device_resized_crop(x[None], regions[None], size, dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == (1, 3, SHAPE[1]) + tuple(size) and got.is_cuda
        SU.check(got[0], gold[case], SHAPE[2], SHAPE[3], 1.0, bf16, "device_resized_crop vs the reference, case %d" % case)
        SU.check(got[0], TR.resized_crop(x, regions, size), SHAPE[2], SHAPE[3], 1.0, bf16, "vs resized_crop, case %d" % case)
    # two clips at once, the decoder's layout, Div255 + Normalize fused in: item b is clip b
    clips = torch.stack([clip(650), clip(651)])
    regions = torch.stack([_case_regions(CASES[5][0], SHAPE[1]), _case_regions(CASES[0][0], SHAPE[1])])
    got = TR.device_resized_crop(clips.permute(0, 2, 3, 4, 1).contiguous(), regions, (12, 14), dtype=dtype, src_layout="NTHWC", **KW)
    scale, shift = SU.affine()
    for b in range(2):
        want = TR.resized_crop(clips[b], regions[b], (12, 14)) * scale.view(3, 1, 1, 1) + shift.view(3, 1, 1, 1)
        SU.check(got[b], want, SHAPE[2], SHAPE[3], float(scale.max()), bf16, "normalised, clip %d" % b)


# ----------------------------------------------------------------------------- model level
def _deploy(m, x, dtype=torch.bfloat16, **kw):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    transmute_model(m, "mi355x")
    xd = [t.cuda().to(dtype) for t in x] if isinstance(x, list) else x.cuda().to(dtype)
    return convert_to_deployable_form(m, xd, dtype=dtype, **kw)


@pytest.fixture(scope="module")
def x3d6():
    """x3d_xs (4 x 160 x 160, 400 classes) converted for 6 items: the recipe of tests/test_gpu_batch_views.py."""
    from oracle.weights import seeded_input, trained_like_fill
    from pytorchvideo_amd.models import create_x3d
    m = create_x3d(model_num_class=400, input_clip_length=4, input_crop_size=160)
    m = trained_like_fill(m, seeded_input((4, 3, 4, 160, 160), 5), 0).eval()
    return _deploy(m, seeded_input((6, 3, 4, 160, 160), 6))


def _nthwc_video(n, hs, ws, seed):
    return SU.clip((3, n, hs, ws), seed).permute(1, 2, 3, 0).contiguous().cuda()


def test_tube_predictor_scores_the_rows_of_pre_cropped_tubes(x3d6):
    """Two videos, two time stamps each, two static square boxes with integer corners per time stamp: 8 tubes, a full
    forward and a short one.  The same deploy form walked through the existing video_batch / fill_batch / launch on dense
    pre-cropped copies of the tubes with short_side = crop_size = 160 (Hn = Wn = 160, offsets 0: the same items at the same
    batch positions) must return the same rows, bit for bit."""
    videos = [_nthwc_video(9, 180, 240, 2400), _nthwc_video(7, 200, 170, 2401)]
    stamps = [[0.5, 1.5], [0.5, 1.25]]                           # 4 frames per second, clips of one second: frames 0..3, 4..7 / 0..3, 3..6
    boxes = [[torch.tensor([[20.0, 10.0, 120.0, 110.0], [100.0, 30.0, 240.0, 170.0]]), torch.tensor([[0.0, 0.0, 180.0, 180.0], [61.0, 7.0, 94.0, 40.0]])],
             [torch.tensor([[5.0, 40.0, 165.0, 200.0], [10.0, 10.0, 11.0, 11.0]]), torch.tensor([[30.0, 50.0, 130.0, 150.0], [0.0, 0.0, 170.0, 170.0]])]]
    tubes = TubePredictor(x3d6, 1.0, crop_size=160, context=1.0, square=True, src_layout="NTHWC", **KW)
    got = tubes(videos, 4, stamps, boxes).clone()
    assert tuple(got.shape) == (8, 400) and got.dtype == torch.float32 and tubes.forwards == 2
    # the second forward was short: its tail is zero
    tail = BV._input_items(tubes.packer)
    assert bool((tail[2:] == 0).all()) and not bool((tail[:2] == 0).all())
    packer = TR.DevicePacker(x3d6, short_side=160, crop_size=160, spatial_idx=1, src_layout="NTHWC", **KW)
    from pytorchvideo_amd.data.clip_sampling import keyframe_frame_table
    cropped, tables = [], []
    for video, ts, per_stamp in zip(videos, stamps, boxes):
        table, _ = keyframe_frame_table(ts, 1.0, video.shape[0], 4, 4)
        for k, bs in enumerate(per_stamp):
            for x1, y1, x2, y2 in bs.long().tolist():
                cropped.append(video[:, y1:y2, x1:x2].contiguous())
                tables.append(table[k:k + 1])
    batch = packer.video_batch(cropped, tables)
    assert batch.total == 8 and all((rec.Hn, rec.Wn, rec.y_off[0], rec.x_off[0]) == (160, 160, 0, 0) for rec in batch.sources)
    want = torch.zeros_like(got)
    for i0, n in TR.batch_chunks(batch.total, packer.batch):
        packer.fill_batch(batch, i0, n)
        want[i0:i0 + n] = packer.launch()[:n]
    packer.release_batch()
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got, want)
    # rows differ between tubes: the rectangles are honoured, not one crop for all
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[2], got[3])


def test_tube_predictor_fills_both_pathways_of_slowfast_with_a_moving_tube():
    """slowfast_r50_small (4 + 16 frames at 96 x 96, frame_ratios (4, 1), batch 4): one tube that moves and grows along a
    track.  Each pathway's input holds the host mirror of ITS frames and ITS rectangles -- the column subset `pathway_tables`
    takes -- within `spatial_util.bound`."""
    from oracle.weights import deterministic_fill, seeded_input
    from pytorchvideo_amd.data.clip_sampling import keyframe_frame_table
    from pytorchvideo_amd.models import create_slowfast
    g = torch.load(os.path.join(GOLD, "slowfast_r50_small.pt"), weights_only=False)
    m = deterministic_fill(create_slowfast(**g["cfg"]), g["seed"]).eval()
    fast = seeded_input((4, 3, 16, 96, 96), 7)
    dep = _deploy(m, [TR.uniform_temporal_subsample(fast, 4, 2), fast])
    host = SU.clip((3, 24, 131, 113), 2410)
    video = host.permute(1, 2, 3, 0).contiguous().cuda()
    track = (torch.tensor([0, 10, 23]), torch.tensor([[5.0, 8.0, 45.0, 60.0], [30.5, 40.0, 90.0, 110.0], [50.0, 20.0, 113.0, 131.0]]))
    tubes = TubePredictor(dep, 0.8, crop_size=96, context=1.1, square=False, frame_ratios=(4, 1), src_layout="NTHWC", **KW)
    out = tubes(video, 20, [0.6], None, tracks=[[track]])
    assert tuple(out.shape)[0] == 1 and tubes.forwards == 1 and torch.isfinite(out).all()
    table, _ = keyframe_frame_table([0.6], 0.8, 24, 20, 16)     # frames 4 .. 19
    rects = TR.box_regions(TR.track_boxes_at(track[0], track[1], table[0]), 131, 113, 1.1, False)
    assert len({tuple(r) for r in rects.tolist()}) > 8           # the tube does move
    scale, shift = SU.affine()
    p = tubes.packer
    for i, ref in enumerate(p.refs):
        cols = TR.temporal_indices(16, ref.T)
        frames = host[:, table[0][cols].long()]
        want = TR.resized_crop(frames, rects[cols], 96) * scale.view(3, 1, 1, 1) + shift.view(3, 1, 1, 1)
        held = p._planar[i] if i in p._planar else p.sess.view(ref)
        SU.check(held[0, :3].float(), want, 131, 113, float(scale.max()), True, "pathway %d (%d frames)" % (i, ref.T))
        assert bool((held[1:].float() == 0).all())               # one tube in a batch of four: the rest is zero
