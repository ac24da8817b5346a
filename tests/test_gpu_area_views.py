"""The box-filtered downscale on the MI355X: `pv_area_views` (include/pv_mi355x.h "box-filtered downscale"),
`transforms.device_scale_crop(interpolation="area")`, `DevicePacker(interpolation="area")` and the predictors.

Reference: the float64 box mean of the raw taps over the header's integer windows (tests/area_util.py; for YUV the taps are
converted and clamped first, tests/yuv_util.rgb_of_planes), under the derived bound of `area_util.tolerance`, every element
asserted.  Bit for bit (`torch.equal`): an item against the same item launched alone, a frame list against the stacked video,
the identity geometry against `pv_batch_views`, `device_scale_crop` against the ABI launch, the predictors against the deploy
form run on the area views.  No test feeds the device a window or a table entry that leaves its video."""
import ctypes as C
from fractions import Fraction

import pytest
import torch

import area_util as AU
import spatial_util as SU
import test_gpu_batch_views as BV
import yuv16_util as Y16
import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import KeyframeDetector, VideoBatchPredictor

pytestmark = pytest.mark.gpu
SENTINEL = BV.SENTINEL
KW = dict(mean=SU.MEAN, std=SU.STD, div255=True)
SCALE, SHIFT = SU.affine()
MAX_SCALE = float(SCALE.max())
PLANE_FIELDS = ("frame_stride", "u_offset", "v_offset", "y_pitch", "c_pitch")
N, T = 3, 2
TABLE = torch.tensor([[1, 1], [0, 5]], dtype=torch.int32)       # a repeated frame; 5 is clamped to the last frame, 2
SOURCES = BV.SOURCES
SOURCE_IDS = ["planar_u8", "planar_f32", "interleaved_u8"]
# The widest column tile the kernels choose is 64 output columns (kArTiles, pv_area.hip): the 500-column window of the
# 96 x 1500 geometry spans at least 8 of them, and its 32 rows at least 4 strips of at most 8.
WIDEST_TILE = 64


# ----------------------------------------------------------------------------- launches
def _record(src, n, hs, ws, hn, wn, offsets, **planes):
    return dict(src=src, N=n, Hs=hs, Ws=ws, Hn=hn, Wn=wn, sy=BV._f32(hs, hn), sx=BV._f32(ws, wn), offsets=offsets, **planes)


def _sources(recs):
    sources = (L.ViewSource * len(recs))()
    for rec, r in zip(sources, recs):
        for k, v in r.items():
            if k == "offsets":
                for i, (y, x) in enumerate(v):
                    rec.y_off[i], rec.x_off[i] = y, x
            else:
                setattr(rec, k, v)
    return sources


def _launch(recs, codes, table, triples, window, n_views, form, dtype, c_step=0, matrix=None, ptrs=None, entry="pv_area_views",
            affine=True, channels=3):
    """`entry` over the sources `recs` for the items `triples` = (source, table row, view) into the middle of a sentinel-filled
    destination with one guard item in front and one behind, both checked here.  `table` int32 [rows, T] on the host; `ptrs`:
    the int64 pointer table of a frame-list launch (a record's src is then an INDEX into it).  Returns the items written."""
    from gpu_util import call
    a = L.AreaViewsDesc()
    a.filter = L.PV_FILTER_AREA
    d = a.frames.batch
    tab = table.to(torch.int32).contiguous().cuda()
    keep = [tab]
    if ptrs is not None:
        ptrs_dev = ptrs.cuda()
        keep.append(ptrs_dev)
        a.frames.frame_ptrs, a.frames.frame_ptrs_dev, a.frames.n_frame_ptrs = ptrs.data_ptr(), ptrs_dev.data_ptr(), ptrs.numel()
        recs = [dict(r, src=ptrs_dev.data_ptr() + 8 * r["src"]) for r in recs]
    sources, items = _sources(recs), BV._items(triples)
    keep += [BV._upload(sources), BV._upload(items), SCALE.cuda(), SHIFT.cuda()]
    d.sources, d.sources_dev = C.addressof(sources), keep[-4].data_ptr()
    d.items, d.items_dev = C.addressof(items), keep[-3].data_ptr()
    d.n_sources, d.n_items = len(sources), len(items)
    if affine:
        d.ch_scale, d.ch_shift = keep[-2].data_ptr(), keep[-1].data_ptr()
    d.t_index, d.n_rows, d.t_stride, d.C, d.T = tab.data_ptr(), tab.shape[0], tab.shape[1], channels, tab.shape[1]
    d.src_layout, d.src_dtype = codes
    if matrix is not None:
        d.c_step, d.yuv2rgb = c_step, matrix.data_ptr()
    ho, wo = window
    d.Ho, d.Wo, d.n_views = ho, wo, n_views
    n, t = len(items), tab.shape[1]
    d.dst_dtype = L.PV_BF16 if dtype == torch.bfloat16 else L.PV_F32
    if form == "planar":
        dst = torch.full((n + 2, channels, t, ho, wo), SENTINEL, dtype=dtype, device="cuda")
        d.dst_layout = L.DST_NCTHW
    else:
        c_p, ld = {"c4": (4, 4), "cl8": (8, 8), "cl8_ld16": (8, 16)}[form]
        dst = torch.full((n + 2, t, ho, wo, ld), SENTINEL, dtype=dtype, device="cuda")
        d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, c_p, ld, t * ho * wo * ld
    d.dst = dst[1].data_ptr()
    call(entry, d if entry == "pv_batch_views" else a)
    assert torch.all(dst[0] == SENTINEL) and torch.all(dst[-1] == SENTINEL), "the guard items around dst were written"
    assert not torch.all(dst[1:-1] == SENTINEL)
    return dst[1:-1]


def _codes(layout, dtype):
    return (L.SRC_NCTHW if layout == "NCTHW" else L.SRC_NTHWC, L.PV_U8 if dtype == torch.uint8 else L.PV_F32)


def _rgb_record(src, layout, hn, wn, offsets):
    c, n, hs, ws = TR._video_geometry(src, layout)
    return _record(src.data_ptr(), n, hs, ws, hn, wn, offsets)


def _frames_of(table, row, n):
    return table[row].long().clamp(0, n - 1)


def _planar(item, form):
    """[C, T, Ho, Wo] of one destination item, whatever its form."""
    return item if form == "planar" else item.permute(3, 0, 1, 2)


# ----------------------------------------------------------------------------- RGB / planar sources against the reference
_CASES = {}


def _case(name):
    """The video of a geometry, its views and the float64 reference of every (row, view) item: computed once per run."""
    if name not in _CASES:
        hs, ws, short, crop = AU.GEOMETRIES[name]
        hn, wn, window, offsets = AU.view_geometry(hs, ws, short, crop)
        video = SU.clip((3, N, hs, ws), 3100 + hs)
        triples = [(0, r, v) for r in range(TABLE.shape[0]) for v in range(len(offsets))]
        refs, worst_n = [], 0
        for _, r, v in triples:
            ref, n = AU.reference(video[:, _frames_of(TABLE, r, N)], hn, wn, offsets[v][0], offsets[v][1], window[0], window[1], SCALE, SHIFT)
            refs.append(ref)
            worst_n = max(worst_n, n)
        _CASES[name] = (video, hn, wn, window, offsets, triples, refs, worst_n)
    return _CASES[name]


@pytest.mark.parametrize("layout,src_dtype", SOURCES, ids=SOURCE_IDS)
@pytest.mark.parametrize("name", list(AU.GEOMETRIES))
def test_area_views_against_the_float64_box_mean(name, layout, src_dtype):
    video, hn, wn, window, offsets, triples, refs, n = _case(name)
    if name == "96x1500_to_32":
        assert window == (32, 500) and window[1] >= 2 * WIDEST_TILE and window[0] > 8          # several strips and column tiles
    src = BV._source(video, layout, src_dtype)
    recs = [_rgb_record(src, layout, hn, wn, offsets)]
    for dtype in (torch.bfloat16, torch.float32):
        got = _launch(recs, _codes(layout, src_dtype), TABLE, triples, window, len(offsets), "planar", dtype)
        for i, ref in enumerate(refs):
            AU.check(got[i], ref, n, MAX_SCALE, src_dtype == torch.uint8, dtype == torch.bfloat16,
                     "%s %s %s -> %s item %d" % (name, layout, src_dtype, dtype, i))
        if name == "33x57_to_33":                                # every window is one pixel: the bits of the four-tap launch
            same = _launch(recs, _codes(layout, src_dtype), TABLE, triples, window, len(offsets), "planar", dtype, entry="pv_batch_views")
            assert BV._same_bits(got, same), (layout, src_dtype, dtype)


@pytest.mark.parametrize("form,dtype", [("c4", torch.bfloat16), ("cl8", torch.bfloat16), ("cl8", torch.float32), ("cl8_ld16", torch.float32)],
                         ids=["c4_bf16", "cl8_bf16", "cl8_f32", "cl8_ld16_f32"])
def test_the_channels_last_forms_hold_the_same_values_and_zero_pads(form, dtype):
    name = "45x70_to_16"
    video, hn, wn, window, offsets, triples, refs, n = _case(name)
    c_p = 4 if form == "c4" else 8
    for layout, src_dtype in SOURCES:
        src = BV._source(video, layout, src_dtype)
        recs = [_rgb_record(src, layout, hn, wn, offsets)]
        got = _launch(recs, _codes(layout, src_dtype), TABLE, triples, window, len(offsets), form, dtype)
        planar = _launch(recs, _codes(layout, src_dtype), TABLE, triples, window, len(offsets), "planar", dtype)
        for i, ref in enumerate(refs):
            item = _planar(got[i], form)
            AU.check(item[:3], ref, n, MAX_SCALE, src_dtype == torch.uint8, dtype == torch.bfloat16, "%s %s item %d" % (form, layout, i))
            assert BV._same_bits(item[:3].contiguous(), planar[i].contiguous()), (form, layout, i)   # one rounding, every form
            assert bool((item[3:c_p] == 0).all()), "pad channels are zero"
            assert bool((item[c_p:] == SENTINEL).all()), "the bytes between c_p and ld are not written"


# ----------------------------------------------------------------------------- YUV 4:2:0
M601 = TR.yuv_matrix("bt601", False)
YUV_LAYOUTS = {
    # layout: (module, planes kwargs, pack kwargs per (pitch, coded height), matrix)
    "NV12": (YU, {}, dict(base=3, garbage=9), M601),
    "I420": (YU, {}, dict(base=2, garbage=7), M601),
    "P010": (Y16, dict(shift=6), dict(base=1, garbage=5), TR.yuv_matrix("bt709", True, 10, True)),
    "I010": (Y16, {}, {}, TR.yuv_matrix("bt709", False, 10, False)),
}


def _yuv_case(layout, hs, ws, pitched=True):
    """A video as decoder surfaces -- pitch above the width and a coded height above the height (NV12: at an odd base
    address), except I010, which is tight -- its records' plane fields, and the float64 converted-then-clamped RGB frames."""
    mod, pkw, packkw, matrix = YUV_LAYOUTS[layout]
    planes = mod.planes(N, hs, ws, 3300 + hs, **pkw)
    kw, geo_kw = dict(packkw), {}
    if packkw and pitched:
        kw.update(coded_height=hs + 10, pitch=(ws + 15) // 16 * 16 + 16)
        geo_kw = dict(coded_height=hs + 10, height=hs)
    frames = mod.pack(*planes, layout, **kw).frames("cuda")
    geom = TR.yuv_geometry(frames, layout, **geo_kw)
    assert (geom["N"], geom["Hs"], geom["Ws"]) == (N, hs, ws)
    rgb = mod.rgb_of_planes(*planes, matrix.float()).permute(1, 0, 2, 3)                     # [3, N, Hs, Ws] float64
    wide = layout in TR.YUV16_LAYOUTS
    return frames, geom, rgb, (L.SRC_YUV420, L.PV_U16 if wide else L.PV_U8), matrix.float().reshape(12).cuda()


@pytest.mark.parametrize("hs,ws", [(46, 70), (136, 240)], ids=["46x70", "136x240"])
@pytest.mark.parametrize("layout", list(YUV_LAYOUTS))
def test_area_views_yuv_converts_and_clamps_every_tap_then_averages(layout, hs, ws):
    frames, geom, rgb, codes, matrix = _yuv_case(layout, hs, ws)
    if layout == "NV12":
        assert geom["y_pitch"] > ws and geom["u_offset"] > hs * geom["y_pitch"] and frames.data_ptr() % 2 == 1
    hn, wn, window, offsets = AU.view_geometry(hs, ws, 16, 16)
    rec = _record(frames.data_ptr(), N, hs, ws, hn, wn, offsets, **{k: geom[k] for k in PLANE_FIELDS})
    triples = [(0, r, v) for r in range(TABLE.shape[0]) for v in range(3)]
    refs = [AU.reference(rgb[:, _frames_of(TABLE, r, N)], hn, wn, offsets[v][0], offsets[v][1], 16, 16, SCALE, SHIFT) for _, r, v in triples]
    n = max(k for _, k in refs)
    for form, dtype in (("planar", torch.float32), ("planar", torch.bfloat16), ("c4", torch.bfloat16)):
        got = _launch([rec], codes, TABLE, triples, window, 3, form, dtype, geom["c_step"], matrix)
        for i, (ref, _) in enumerate(refs):
            AU.check(_planar(got[i], form)[:3], ref, n, MAX_SCALE, False, dtype == torch.bfloat16,
                     "%s %dx%d -> %s %s item %d" % (layout, hs, ws, form, dtype, i))


# ----------------------------------------------------------------------------- nothing beyond `end` is read
@pytest.mark.parametrize("name", ["45x70_to_16", "135x240_to_16", "20x30_to_32"])
def test_nothing_outside_the_footprint_of_a_view_enters_it(name):
    """An fp32 planar source that is NaN everywhere outside the source footprint of the view being written -- rows
    [start_y(first), end_y(last)) x columns likewise: the output is finite and within the bound."""
    video, hn, wn, window, offsets, _, _, _ = _case(name)
    hs, ws = video.shape[-2:]
    for v, (y0, x0) in enumerate(offsets):
        sy, ey = AU.windows(hs, hn, y0, window[0])
        sx, ex = AU.windows(ws, wn, x0, window[1])
        inside = torch.zeros((hs, ws), dtype=torch.bool)
        inside[int(sy[0]):int(ey[-1]), int(sx[0]):int(ex[-1])] = True
        assert not bool(inside.all())                            # there is something outside to poison
        src = torch.where(inside, video.float(), torch.tensor(float("nan"))).cuda()
        recs = [_rgb_record(src, "NCTHW", hn, wn, offsets)]
        triples = [(0, r, v) for r in range(TABLE.shape[0])]
        got = _launch(recs, _codes("NCTHW", torch.float32), TABLE, triples, window, len(offsets), "planar", torch.float32)
        for i, (_, r, _) in enumerate(triples):
            ref, n = AU.reference(video[:, _frames_of(TABLE, r, N)], hn, wn, y0, x0, window[0], window[1], SCALE, SHIFT)
            AU.check(got[i], ref, n, MAX_SCALE, False, False, "%s view %d row %d, NaN outside the footprint" % (name, v, r))


# ----------------------------------------------------------------------------- sharing a launch
def _mixed(layout, src_dtype):
    """The 45 x 70, 135 x 240 and 96 x 1500 videos as three sources of one launch with a 16 x 16 window (short side 16, 16 and
    32, three views each): the staged rows and the LDS pitch follow the 8.4x record, the strip height differs from the one each
    video gets alone."""
    recs, keep = [], []
    for name, short in (("45x70_to_16", 16), ("135x240_to_16", 16), ("96x1500_to_32", 32)):
        video = _case(name)[0]
        hn, wn, _, offsets = AU.view_geometry(video.shape[-2], video.shape[-1], short, 16)
        src = BV._source(video, layout, src_dtype)
        keep.append(src)
        recs.append(_rgb_record(src, layout, hn, wn, offsets))
    triples = [(2, 1, 0), (0, 0, 2), (1, 1, 1), (0, 1, 0), (2, 0, 2), (1, 0, 0), (0, 0, 2), (2, 1, 1), (1, 1, 2)]   # (0, 0, 2) twice
    return recs, keep, triples


@pytest.mark.parametrize("layout,src_dtype", SOURCES, ids=SOURCE_IDS)
def test_an_item_holds_the_same_bits_whatever_shares_its_launch(layout, src_dtype):
    recs, keep, triples = _mixed(layout, src_dtype)
    for form, dtype in (("planar", torch.bfloat16), ("cl8", torch.float32)):
        got = _launch(recs, _codes(layout, src_dtype), TABLE, triples, (16, 16), 3, form, dtype)
        assert BV._same_bits(got[1], got[6])                     # the repeated item
        for i, triple in enumerate(triples):
            alone = _launch(recs, _codes(layout, src_dtype), TABLE, [triple], (16, 16), 3, form, dtype)
            assert BV._same_bits(alone[0], got[i]), (layout, src_dtype, form, i, triple)


# ----------------------------------------------------------------------------- frame lists
def _pointer_table(per_video_frames):
    ptrs = torch.tensor([f.data_ptr() for frames in per_video_frames for f in frames], dtype=torch.int64)
    first, k = [], 0
    for frames in per_video_frames:
        first.append(k)
        k += len(frames)
    return ptrs, first


@pytest.mark.parametrize("kind", ["interleaved_u8", "planar_f32", "NV12"])
def test_a_frame_list_gives_the_bits_of_the_stacked_video(kind):
    """The same items with every frame a separate allocation, addressed through the pointer table, equal the whole-video launch."""
    if kind == "NV12":
        cases = [_yuv_case("NV12", 46, 70), _yuv_case("NV12", 136, 240)]
        recs, lists = [], []
        for frames, geom, _, codes, matrix in cases:
            hn, wn, _, offsets = AU.view_geometry(geom["Hs"], geom["Ws"], 16, 16)
            recs.append(_record(frames.data_ptr(), N, geom["Hs"], geom["Ws"], hn, wn, offsets, **{k: geom[k] for k in PLANE_FIELDS}))
            lists.append(list(frames.unbind(0)))                 # every surface where it lies
        c_step = cases[0][1]["c_step"]
        triples = [(1, 1, 0), (0, 0, 2), (1, 0, 1), (0, 1, 1)]
    else:
        layout, src_dtype = ("NTHWC", torch.uint8) if kind == "interleaved_u8" else ("NCTHW", torch.float32)
        recs, keep, triples = _mixed(layout, src_dtype)
        codes, matrix, c_step = _codes(layout, src_dtype), None, 0
        # every frame an allocation of its own; a planar frame of a list is a dense [C, Hs, Ws]
        lists = [[f.clone(memory_format=torch.contiguous_format) for f in s.unbind(1 if layout == "NCTHW" else 0)] for s in keep]
    ptrs, first = _pointer_table(lists)
    listed = [dict(r, src=k) for r, k in zip(recs, first)]
    for form, dtype in (("c4", torch.bfloat16), ("planar", torch.float32)):
        whole = _launch(recs, codes, TABLE, triples, (16, 16), 3, form, dtype, c_step, matrix)
        got = _launch(listed, codes, TABLE, triples, (16, 16), 3, form, dtype, c_step, matrix, ptrs=ptrs)
        assert BV._same_bits(got, whole), (kind, form, dtype)


# ----------------------------------------------------------------------------- the index limit
def test_the_index_limit_is_2_to_the_24_inclusive():
    """Hs * Hn == 2^24 runs (the identity on a 4096 x 8 one-channel frame returns the pixels); 4098 * 4098 is refused."""
    g = torch.Generator().manual_seed(3500)
    for hs, ok in ((4096, True), (4098, False)):
        video = torch.randint(0, 256, (1, 1, hs, 8), generator=g, dtype=torch.uint8)
        src = video.cuda()
        rec = _record(src.data_ptr(), 1, hs, 8, hs, 8, [(hs - 8, 0)])
        args = ([rec], _codes("NCTHW", torch.uint8), torch.zeros((1, 1), dtype=torch.int32), [(0, 0, 0)], (8, 8), 1, "planar", torch.float32)
        if ok:
            got = _launch(*args, affine=False, channels=1)
            assert torch.equal(got[0, 0, 0].cpu(), video[0, 0, hs - 8:].float())
        else:
            with pytest.raises(L.PvError, match="unsupported"):
                _launch(*args, affine=False, channels=1)


# ----------------------------------------------------------------------------- device_scale_crop
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_device_scale_crop_area_is_the_abi_launch_and_the_host_mirror(dtype):
    video, hn, wn, window, offsets, _, _, _ = _case("45x70_to_16")
    other = SU.clip((3, N, 45, 70), 3600)
    clips = torch.stack([video, other])                          # [2, 3, N, 45, 70]
    got = TR.device_scale_crop(clips, 16, 16, (0, 1, 2), dtype=dtype, interpolation="area", **KW)
    assert got.dtype == dtype and tuple(got.shape) == (6, 3, N, 16, 16) and got.is_cuda
    srcs = [c.cuda() for c in clips]
    recs = [_rgb_record(s, "NCTHW", hn, wn, offsets) for s in srcs]
    table = torch.arange(N, dtype=torch.int32)[None].repeat(2, 1)
    triples = [(b, b, v) for b in range(2) for v in range(3)]
    abi = _launch(recs, _codes("NCTHW", torch.uint8), table, triples, (16, 16), 3, "planar", dtype)
    assert BV._same_bits(got, abi.contiguous())
    norm = TR.Normalize(SU.MEAN, SU.STD)
    for b in range(2):
        scaled = TR.short_side_scale(clips[b].float(), 16, "area")
        n = AU.reference(clips[b], hn, wn, 0, 0, hn, wn)[1]
        for v in range(3):
            want = norm(TR.div_255(TR.uniform_crop(scaled, 16, v)))
            AU.check(got[b * 3 + v], want, n, MAX_SCALE, False, dtype == torch.bfloat16, "clip %d view %d vs the host mirror" % (b, v))
    # the decoder's layout with a frame subsample, and NV12 surfaces: the same route, against the reference
    idx = TR.temporal_indices(N, 2)
    nthwc = TR.device_scale_crop(clips.permute(0, 2, 3, 4, 1).contiguous(), 16, 16, 1, num_frames=2, dtype=dtype, src_layout="NTHWC",
                                 interpolation="area", **KW)
    assert tuple(nthwc.shape) == (2, 3, 2, 16, 16)
    for b in range(2):
        ref, n = AU.reference(clips[b][:, idx], hn, wn, offsets[1][0], offsets[1][1], 16, 16, SCALE, SHIFT)
        AU.check(nthwc[b], ref, n, MAX_SCALE, True, dtype == torch.bfloat16, "NTHWC clip %d" % b)
    frames, geom, rgb, _, _ = _yuv_case("NV12", 46, 70)
    hn2, wn2, _, off2 = AU.view_geometry(46, 70, 16, 16)
    nv12 = TR.device_scale_crop(frames, 16, 16, (0, 2), dtype=dtype, src_layout="NV12", yuv=("bt601", False), coded_height=56, height=46,
                                interpolation="area", **KW)
    assert tuple(nv12.shape) == (2, 3, N, 16, 16)
    for k, v in enumerate((0, 2)):
        ref, n = AU.reference(rgb, hn2, wn2, off2[v][0], off2[v][1], 16, 16, SCALE, SHIFT)
        AU.check(nv12[k], ref, n, MAX_SCALE, False, dtype == torch.bfloat16, "NV12 view %d" % v)


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def x3d6():
    return BV._x3d(6)


def _checkerboard(n, hs, ws):
    """A one-pixel checkerboard of 0 / 255, uint8 [n, hs, ws, 3] on the device: point sampling sees black or white, a box grey."""
    board = ((torch.arange(hs)[:, None] + torch.arange(ws)[None]) % 2 * 255).to(torch.uint8)
    return board[None, :, :, None].expand(n, hs, ws, 3).contiguous().cuda()


def test_batch_predictor_area_scores_the_area_views(x3d6):
    """x3d_xs at batch 6, two videos of different sizes, clips of 8 frames subsampled to 4, three views: the scores equal the
    fold of the deploy form's logits on the `device_scale_crop(interpolation="area")` views of every clip, bit for bit; and on
    a one-pixel checkerboard they differ from the bilinear predictor's."""
    videos = [BV._nthwc_video(17, 360, 480, 3700), BV._nthwc_video(9, 400, 380, 3701)]
    sampler = D.UniformClipSampler(Fraction(8, 10))
    pred = VideoBatchPredictor(x3d6, sampler, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), interpolation="area", **KW)
    assert pred.packer.area
    scores = pred(videos, 10).clone()
    views, video_of = [], []
    for j, video in enumerate(videos):
        table, _ = D.clip_frame_table(sampler, video.shape[0], 10, pred.packer.clip_frames)
        for row in table:
            clip = video[row.long().cuda()][None]                 # [1, T, H, W, 3]
            views.append(TR.device_scale_crop(clip, 176, 160, (0, 1, 2), src_layout="NTHWC", interpolation="area", **KW))
            video_of += [j] * 3
    views = torch.cat(views)
    video_of = torch.tensor(video_of, dtype=torch.int32, device="cuda")
    ve = VideoEnsembler(2, scores.shape[1], "sum")
    for i0 in range(0, views.shape[0], 6):
        n = min(6, views.shape[0] - i0)
        x = torch.zeros((6,) + tuple(views.shape[1:]), dtype=torch.bfloat16, device="cuda")
        x[:n] = views[i0:i0 + n]
        ve.update(x3d6(x)[:n], video_of[i0:i0 + n])
    want = ve.result()
    assert views.shape[0] == 9 and pred.forwards == 2
    assert torch.equal(scores, want), "scores differ by %.3e" % (scores - want).abs().max().item()
    assert not torch.equal(scores[0], scores[1])
    board = [_checkerboard(8, 360, 480)]
    area = pred(board, 10).clone()
    plain = VideoBatchPredictor(x3d6, sampler, short_side=176, crop_size=160, spatial_idx=(0, 1, 2), **KW)(board, 10)
    assert torch.isfinite(area).all() and not torch.equal(area, plain)


def test_keyframe_detector_area_fills_the_area_views_and_the_same_boxes():
    """resnet_det_r50_small at 48 x 72, no-crop mode, one 60 x 90 video, two key frames in one forward: the input items are the
    area views of the key-frame clips, and the box buffer is the bilinear detector's (boxes depend on the geometry only)."""
    import test_gpu_keyframe_detection as KD
    dm = KD._form("resnet_det_r50_small", torch.bfloat16, 48, 72)[0]
    video = KD._video(40, 60, 90, 4500).cuda()
    stamps, box_list = KD.STAMPS[:2], KD._split(KD.box_set(60, 90), [2, 3])

    def run(**kw):
        det = KeyframeDetector(dm, KD.DURATION, short_side=48, **KW, **kw)
        out = det(video, KD.FPS, stamps, box_list).clone()
        p = det.packer
        ref = p.refs[0]
        held = (p._planar[0] if 0 in p._planar else p.sess.view(ref))[:, :3].clone()
        cap = p.box_capacity
        ptr = p.model._pv_box_ptr
        boxes = p.sess.weights_t[ptr.off: ptr.off + cap * 20].view(torch.float32).view(cap, 5).clone()
        assert det.forwards == 1
        return out, held, boxes

    out_a, held_a, boxes_a = run(interpolation="area")
    out_b, held_b, boxes_b = run()
    assert torch.equal(boxes_a, boxes_b) and bool((boxes_a[:, 0] >= 0).all())
    assert not torch.equal(held_a, held_b) and torch.isfinite(out_a).all() and tuple(out_a.shape) == tuple(out_b.shape)
    table, _ = D.keyframe_frame_table(stamps, KD.DURATION, 40, KD.FPS, 4)
    for k in range(2):
        clip = video[table[k].long().cuda()][None]
        # no crop: the window is the whole scaled frame, 48 x 72, which device_scale_crop's square crop cannot say: the ABI launch
        src = clip[0].contiguous()
        rec = _rgb_record(src, "NTHWC", 48, 72, [(0, 0)])
        want = _launch([rec], _codes("NTHWC", torch.uint8), torch.arange(4, dtype=torch.int32)[None], [(0, 0, 0)], (48, 72), 1, "planar",
                       torch.bfloat16)
        assert BV._same_bits(held_a[k].contiguous(), want[0].contiguous()), k
