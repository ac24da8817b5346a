"""A rectangle per frame (`pv_region_views`, include/pv_mi355x.h "a rectangle per frame"), without a GPU: the host mirror
`transforms.resized_crop` against the reference's own `random_resized_crop` (tests/golden/region_transforms.pt, recorded by
tests/golden/make_region_golden.py), `box_regions` / `track_boxes_at` on hand-computed cases, the entry point -- exported,
mirrored by ctypes, validated before any launch --, the code-object metadata of its kernels, and the host logic and the
refusals of `DevicePacker.video_batch(regions=)`."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

import spatial_util as SU
import test_batch_views as TB
import test_frame_views as TF
from make_region_golden import CASES, SHAPE, clip
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
W = TB.W


def _shift_rectangles(first, last, t):
    """The per-frame rectangles of the reference's `shift=True`: every member `torch.linspace` over the clip, cut by int()."""
    cols = [[int(v) for v in torch.linspace(a, b, steps=t).tolist()] for a, b in zip(first, last)]
    return torch.tensor(cols).T.contiguous()


def _regions_of(rects, t):
    return torch.tensor(rects[0]) if len(rects) == 1 else _shift_rectangles(rects[0], rects[1], t)


# ----------------------------------------------------------------------------- the host mirror
@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(SU.GOLD_DIR, "region_transforms.pt"), weights_only=False)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_resized_crop_against_the_reference(gold, case):
    rects, (ho, wo) = CASES[case]
    x = clip(600 + case)
    got = TR.resized_crop(x, _regions_of(rects, SHAPE[1]), (ho, wo))
    assert got.dtype == torch.float32 and tuple(got.shape) == (SHAPE[0], SHAPE[1], ho, wo)
    SU.check(got, gold[case], SHAPE[2], SHAPE[3], 1.0, what="resized_crop case %d" % case)
    # and the pinned formula of the header, on the rectangle alone, agrees with the reference inside the same bound
    regions = _regions_of(rects, SHAPE[1])
    regions = regions.expand(SHAPE[1], 4) if regions.dim() == 1 else regions
    for k, (top, left, h, w) in enumerate(regions.tolist()):
        pinned = SU.pinned_resample(x[:, k:k + 1, top:top + h, left:left + w], ho, wo, 0, 0, ho, wo)
        SU.check(pinned, gold[case][:, k:k + 1], SHAPE[2], SHAPE[3], 1.0, what="pinned case %d frame %d" % (case, k))


def test_the_rectangles_of_shift_are_linspace_cut_by_int():
    got = _shift_rectangles((3, 5, 20, 9), (10, 30, 11, 21), 5)
    assert got.tolist() == [[3, 5, 20, 9], [4, 11, 17, 12], [6, 17, 15, 15], [8, 23, 13, 18], [10, 30, 11, 21]]
    # one rectangle for the clip is the same rectangle on every frame
    x = clip(777)
    one = TR.resized_crop(x, (3, 5, 20, 9), 16)
    assert torch.equal(one, TR.resized_crop(x, torch.tensor([[3, 5, 20, 9]] * SHAPE[1]), (16, 16)))
    # the identity size returns the pixels
    assert torch.equal(TR.resized_crop(x, (10, 11, 13, 17), (13, 17)), x[:, :, 10:23, 11:28].float())


def test_resized_crop_refuses_bad_arguments():
    x = clip(778)
    for bad in ((0, 0, 38, 53), (0, 0, 37, 54), (-1, 0, 4, 4), (0, -1, 4, 4), (36, 52, 2, 1), (3, 3, 0, 4), (3, 3, 4, 0)):
        with pytest.raises(ValueError):
            TR.resized_crop(x, bad, 8)
    with pytest.raises(ValueError):
        TR.resized_crop(x, torch.tensor([[0, 0, 4, 4]] * 4), 8)                  # four rectangles for five frames
    with pytest.raises(ValueError):
        TR.resized_crop(x, torch.tensor([0.0, 0.0, 4.0, 4.0]), 8)                # float rectangles
    with pytest.raises(ValueError):
        TR.resized_crop(x, (0, 0, 4, 4), (8, 0))
    with pytest.raises(ValueError):
        TR.resized_crop(x[0], (0, 0, 4, 4), 8)


# ----------------------------------------------------------------------------- boxes to rectangles
def test_box_regions_on_hand_computed_cases():
    f = TR.box_regions
    # floor / ceil: every pixel the box touches
    assert f(torch.tensor([10.2, 5.5, 20.1, 30.0]), 37, 53).tolist() == [5, 10, 25, 11]
    assert f(torch.tensor([10.0, 5.0, 20.0, 30.0]), 37, 53).tolist() == [5, 10, 25, 10]           # integer corners: exact
    # clipped at each edge of a 37 x 53 frame
    assert f(torch.tensor([-5.0, 4.0, 3.5, 9.0]), 37, 53).tolist() == [4, 0, 5, 4]                 # left
    assert f(torch.tensor([4.0, -7.5, 9.0, 3.0]), 37, 53).tolist() == [0, 4, 3, 5]                 # top
    assert f(torch.tensor([48.5, 4.0, 60.0, 9.0]), 37, 53).tolist() == [4, 48, 5, 5]               # right
    assert f(torch.tensor([4.0, 30.2, 9.0, 44.0]), 37, 53).tolist() == [30, 4, 7, 5]               # bottom
    # context enlarges about the centre; square takes the longer side
    assert f(torch.tensor([20.0, 10.0, 30.0, 20.0]), 37, 53, context=1.5).tolist() == [7, 17, 16, 16]   # 12.5..27.5 x 17.5..32.5
    assert f(torch.tensor([20.0, 10.0, 24.0, 20.0]), 37, 53, square=True).tolist() == [10, 17, 10, 10]
    assert f(torch.tensor([20.0, 10.0, 24.0, 20.0]), 37, 53, context=2.0, square=True).tolist() == [5, 12, 20, 20]
    # a square that does not fit is clipped, and is then no square
    assert f(torch.tensor([0.0, 10.0, 4.0, 30.0]), 37, 53, square=True).tolist() == [10, 0, 20, 12]
    # degenerate boxes: a point, an inverted box, a box outside the frame -- one pixel, the nearest
    assert f(torch.tensor([7.0, 9.0, 7.0, 9.0]), 37, 53).tolist() == [9, 7, 1, 1]
    assert f(torch.tensor([50.0, 60.0, 40.0, 50.0]), 37, 53).tolist() == [36, 45, 1, 1]
    assert f(torch.tensor([100.0, 100.0, 120.0, 130.0]), 37, 53).tolist() == [36, 52, 1, 1]
    assert f(torch.tensor([-9.0, -9.0, -3.0, -1.0]), 37, 53).tolist() == [0, 0, 1, 1]
    # even: outward to even members, inside the frame, at least 2 x 2
    assert f(torch.tensor([11.2, 5.5, 20.1, 30.0]), 36, 52, even=True).tolist() == [4, 10, 26, 12]
    assert f(torch.tensor([11.2, 5.5, 20.1, 30.0]), 36, 52, context=1.2, square=True, even=True).tolist() == [2, 0, 32, 32]
    assert f(torch.tensor([51.5, 35.5, 51.5, 35.5]), 36, 52, even=True).tolist() == [34, 50, 2, 2]
    assert f(torch.tensor([0.0, 0.0, 52.0, 36.0]), 36, 52, even=True).tolist() == [0, 0, 36, 52]
    # shapes: [..., 4] in, [..., 4] int64 out
    many = f(torch.zeros(2, 3, 4), 8, 8)
    assert many.dtype == torch.int64 and tuple(many.shape) == (2, 3, 4)
    for bad in (dict(boxes=torch.tensor([0.0, 0.0, float("nan"), 1.0]), height=8, width=8),
                dict(boxes=torch.tensor([0.0, 0.0, float("inf"), 1.0]), height=8, width=8),
                dict(boxes=torch.zeros(3), height=8, width=8), dict(boxes=torch.zeros(4), height=0, width=8),
                dict(boxes=torch.zeros(4), height=8, width=8, context=0.0),
                dict(boxes=torch.zeros(4), height=7, width=8, even=True)):
        with pytest.raises(ValueError):
            f(**bad)
    # whatever comes out is a legal rectangle for resized_crop
    g = torch.Generator().manual_seed(5)
    boxes = (torch.rand(200, 4, generator=g) - 0.25) * 80.0
    for even in (False, True):
        TR._check_regions(f(boxes, 36, 52, 1.3, True, even), 36, 52, even)


def test_track_boxes_at_on_hand_computed_cases():
    track = torch.tensor([[0.0, 0.0, 10.0, 10.0], [2.0, 2.0, 12.0, 12.0], [10.0, 10.0, 20.0, 20.0]])
    got = TR.track_boxes_at([2, 4, 8], track, [0, 2, 3, 4, 6, 7, 8, 9])
    want = [[0, 0, 10, 10], [0, 0, 10, 10], [1, 1, 11, 11], [2, 2, 12, 12], [6, 6, 16, 16], [8, 8, 18, 18], [10, 10, 20, 20],
            [10, 10, 20, 20]]
    assert got.dtype == torch.float64 and got.tolist() == [[float(v) for v in row] for row in want]
    assert TR.track_boxes_at([5], track[:1], [0, 5, 9]).tolist() == [[0.0, 0.0, 10.0, 10.0]] * 3   # one point: held
    with pytest.raises(ValueError):
        TR.track_boxes_at([2, 2, 8], track, [3])
    with pytest.raises(ValueError):
        TR.track_boxes_at([2, 4], track, [3])
    with pytest.raises(ValueError):
        TR.track_boxes_at([], track[:0], [3])


# ----------------------------------------------------------------------------- the entry point
def test_region_views_is_exported_and_mirrored(pv_lib, tmp_path):
    assert "pv_region_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_region_views")
    assert pv_lib.pv_version() == L.ABI_VERSION                  # additive: no existing descriptor changed
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "int pv_region_views(const pv_region_views_desc* d, pv_stream_t stream);" in header
    assert C.sizeof(L.RegionViewsDesc) == C.sizeof(L.FrameViewsDesc) + 16 and C.sizeof(L.ViewRegion) == 32
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16                # what they were
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    text = ('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_region_views_desc) == sizeof(pv_frame_views_desc) + 16, "size");\n'
            '_Static_assert(sizeof(pv_region_views_desc) == %d, "size");\n_Static_assert(sizeof(pv_view_region) == %d, "size");\n'
            '_Static_assert(sizeof(pv_frame_views_desc) == %d, "size");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    sizes = [C.sizeof(L.RegionViewsDesc), C.sizeof(L.ViewRegion), C.sizeof(L.FrameViewsDesc)]
    src.write_text(text % tuple(sizes))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i in range(2):                                           # the assertions do fire
        off = list(sizes)
        off[i] += 8
        src.write_text(text % tuple(off))
        assert subprocess.run(cmd, capture_output=True).returncode != 0, i


def _f32(a, b):
    return C.c_float(a / b).value


def _set_region(reg, top, left, h, w, ho, wo):
    reg.top, reg.left, reg.h, reg.w = top, left, h, w
    reg.sy, reg.sx = _f32(h, ho), _f32(w, wo)


def _region_desc(keep, frames, yuv=False):
    """The base descriptors of tests/test_batch_views.py / tests/test_frame_views.py -- two sources, 2 x W and 6 x W with
    W = 40000, a table of 3 rows of one frame, 4 items writing 1 x W, one view -- wrapped, with a rectangle of 2 x W (the top
    two rows, legal in both sources and of even members) for every row.  It passes EVERY check but the last, the LDS limit of
    a staged strip, so it returns PV_ERR_UNSUPPORTED -- the positive control of every PV_ERR_INVALID case below -- and
    nothing here is ever launched, on a machine with a GPU or without."""
    if frames:
        f, sources, items, ptrs = TF._desc(keep, yuv)
    else:
        d, sources, items = TB._desc(keep, yuv)
        f, ptrs = L.FrameViewsDesc(), None
        C.memmove(C.byref(f.batch), C.byref(d), C.sizeof(d))
    regions = (L.ViewRegion * 3)()
    keep.append(regions)
    for reg in regions:
        _set_region(reg, 0, 0, 2, W, 1, W)
    r = L.RegionViewsDesc()
    C.memmove(C.byref(r.frames), C.byref(f), C.sizeof(f))
    r.regions = r.regions_dev = C.addressof(regions)
    return r, sources, items, regions, ptrs


def _status(r):
    return L.lib().pv_region_views(C.byref(r), None)


FORMS = [(False, False), (False, True), (True, False), (True, True)]
FORM_IDS = ["videos-planar", "videos-nv12", "frames-planar", "frames-nv12"]


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_region_views_is_validated_before_any_launch(pv_lib, frames, yuv):
    keep = []
    assert pv_lib.pv_region_views(None, None) == INV
    assert _status(L.RegionViewsDesc()) == INV
    r, _, _, _, _ = _region_desc(keep, frames, yuv)
    assert _status(r) == UNS                                     # the positive control: only the LDS limit is left
    # this entry point's own pointers
    for field in ("regions", "regions_dev"):
        r, _, _, _, _ = _region_desc(keep, frames, yuv)
        setattr(r, field, None)
        assert _status(r) == INV, field
    r, _, _, _, _ = _region_desc(keep, frames, yuv)
    r.regions_dev += 2                                           # the kernel reads it with dword loads
    assert _status(r) == INV
    # a pointer table only half given, or a length without a table
    full, _, _, _, _ = _region_desc(keep, True, yuv)
    for field in ("frame_ptrs", "frame_ptrs_dev"):
        r, _, _, _, _ = _region_desc(keep, frames, yuv)
        r.frames.frame_ptrs, r.frames.frame_ptrs_dev, r.frames.n_frame_ptrs = full.frames.frame_ptrs, full.frames.frame_ptrs_dev, 6
        setattr(r.frames, field, None)
        assert _status(r) == INV, field
    if not frames:
        r, _, _, _, _ = _region_desc(keep, False, yuv)
        r.frames.n_frame_ptrs = 6
        assert _status(r) == INV
    else:
        for n in (0, -1, 4):                                     # the wrapped entry point's table checks (4: a slice leaves it)
            r, _, _, _, _ = _region_desc(keep, True, yuv)
            r.frames.n_frame_ptrs = n
            assert _status(r) == INV, n
    # one view, and every item names it
    for nv in (0, 2, 3, -1):
        r, _, _, _, _ = _region_desc(keep, frames, yuv)
        r.frames.batch.n_views = nv
        assert _status(r) == INV, nv
    for view in (1, -1):
        for index in (0, 3):
            r, _, items, _, _ = _region_desc(keep, frames, yuv)
            items[index].view = view
            assert _status(r) == INV, (view, index)
    # what the wrapped entry point rejects: the launch fields, the items, the stored frames of a record
    for field in ("sources", "sources_dev", "items", "items_dev", "t_index", "dst") + (("yuv2rgb",) if yuv else ()):
        r, _, _, _, _ = _region_desc(keep, frames, yuv)
        setattr(r.frames.batch, field, None)
        assert _status(r) == INV, field
    for field in ("n_sources", "n_items", "n_rows", "T", "Ho", "Wo", "C"):
        r, _, _, _, _ = _region_desc(keep, frames, yuv)
        setattr(r.frames.batch, field, 0)
        assert _status(r) == INV, field
    for field, bad in (("source", 2), ("source", -1), ("row", 3), ("row", -1)):
        r, _, items, _, _ = _region_desc(keep, frames, yuv)
        setattr(items[3], field, bad)
        assert _status(r) == INV, (field, bad)
    for index in (0, 1):
        for field in ("src", "N", "Hs", "Ws"):
            r, sources, _, _, _ = _region_desc(keep, frames, yuv)
            setattr(sources[index], field, None if field == "src" else 0)
            assert _status(r) == INV, (index, field)
        for orient in (8, -1):
            r, sources, _, _, _ = _region_desc(keep, frames, yuv)
            sources[index].orient = orient
            assert _status(r) == INV, (index, orient)
        if yuv:
            for field in ("frame_stride", "c_pitch"):
                r, sources, _, _, _ = _region_desc(keep, frames, yuv)
                setattr(sources[index], field, 1)
                assert _status(r) == INV, (index, field)
    r, _, _, _, _ = _region_desc(keep, frames, yuv)
    r.frames.batch.dst_dtype = L.PV_U8
    assert _status(r) == UNS
    r, _, _, _, _ = _region_desc(keep, frames, yuv)
    r.frames.batch.src_dtype = L.PV_BF16
    assert _status(r) == UNS


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_the_view_geometry_of_a_record_is_not_read(pv_lib, frames, yuv):
    """Hn, Wn, y_off, x_off, sy and sx of a record belong to pv_batch_views' geometry: here the geometry is the rectangle's,
    and values that the wrapped entry point refuses change nothing."""
    keep = []
    r, sources, _, _, _ = _region_desc(keep, frames, yuv)
    for rec in sources:
        rec.Hn, rec.Wn, rec.sy, rec.sx = 0, -7, 0.0, float("nan")
        rec.y_off[0], rec.x_off[0] = 99, -99
    assert _status(r) == UNS


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_region_views_rejects_invalid_rectangles(pv_lib, frames, yuv):
    """Rows 0 (source 0: 2 x W, items 1 and 3), 1 and 2 (source 1: 6 x W): every rectangle of every row an item names is
    checked against THAT item's source."""
    keep = []
    step = 2 if yuv else 1

    def status(row, top, left, h, w, **fields):
        r, _, _, regions, _ = _region_desc(keep, frames, yuv)
        _set_region(regions[row], top, left, h, w, 1, W)
        for k, v in fields.items():
            setattr(regions[row], k, v)
        return _status(r)

    for row in (0, 1, 2):
        assert status(row, 0, 0, 0, W) == INV and status(row, 0, 0, 2, 0) == INV and status(row, 0, 0, -2, W) == INV
        assert status(row, -step, 0, 2, W) == INV and status(row, 0, -step, 2, W - step) == INV
        assert status(row, 0, step, 2, W) == INV                 # one column past the right edge
        assert status(row, 0, step, 2, W - step) == UNS          # the last column inside
        hs = 2 if row == 0 else 6
        assert status(row, hs - 2 + step, 0, 2, W) == INV        # past the bottom of ITS source
        assert status(row, hs - 2, 0, 2, W) == UNS
        # sy / sx are the library's own division, bit for bit: one ulp off is refused
        for field, good in (("sy", _f32(2, 1)), ("sx", _f32(W, W))):
            bits = C.c_uint32.from_buffer_copy(C.c_float(good)).value
            for off in (1, -1):
                assert status(row, 0, 0, 2, W, **{field: C.c_float.from_buffer_copy(C.c_uint32(bits + off)).value}) == INV
        for k in (0, 1):
            r, _, _, regions, _ = _region_desc(keep, frames, yuv)
            regions[row].reserved[k] = 1
            assert _status(r) == INV, (row, k)
    assert status(0, 0, 0, 4, W) == INV                          # 4 rows: legal in source 1, not in source 0
    assert status(1, 0, 0, 4, W) == UNS
    # YUV 4:2:0: an odd member splits a chroma sample; the RGB / planar forms take any rectangle
    for top, left, h, w in ((1, 0, 2, W), (0, 1, 2, W - 2), (0, 0, 3, W), (0, 0, 2, W - 1)):
        assert status(2, top, left, h, w) == (INV if yuv else UNS), (top, left, h, w)
    assert status(2, 1, 1, 1, 1) == (INV if yuv else UNS)
    # a row no item names is not read: the table has three rows, and with the items all on row 0 the others may hold anything
    r, _, items, regions, _ = _region_desc(keep, frames, yuv)
    for it in items:
        it.source, it.row = 0, 0
    _set_region(regions[1], -5, -5, 0, 0, 1, W)
    assert _status(r) == UNS


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_oriented_records_are_out_of_scope(pv_lib, frames, yuv):
    """A record with orient != 0 named by an item is PV_ERR_UNSUPPORTED; the code is read (a code outside 0..7 is invalid,
    above), an invalid rectangle still wins, and a record no item names may be oriented."""
    keep = []
    for orient in (1, 2, 4, 7):
        r, sources, _, _, _ = _region_desc(keep, frames, yuv)
        sources[1].orient = orient
        assert _status(r) == UNS, orient
    r, sources, _, regions, _ = _region_desc(keep, frames, yuv)
    sources[1].orient = 1
    regions[1].h = 0
    assert _status(r) == INV


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_region(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_region") / "pv_region.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_region.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_region_kernel_is_free_of_scratch_and_spills(asm_region):
    """3 RGB / planar source forms and 2 chroma arrangements x 2 sample widths, x 5 destination forms: no private segment and
    no spilled register.  The register counts are printed (profiles/r21/resource_usage.md records them); they are not gated."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_region, re.S)
    names = [k for k, _ in kernels]
    assert len([n for n in names if "region_views_kernel" in n]) == 15 and len([n for n in names if "region_yuv_kernel" in n]) == 20
    assert len(kernels) == 35, names
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


# ----------------------------------------------------------------------------- host logic of video_batch(regions=)
def _fake_deployed(batch, size, frames=(4,), detection=False):
    refs = [types.SimpleNamespace(B=batch, C=3, T=t, H=size[0], W=size[1], src_slot=None, c4_readers=0) for t in frames]
    dep = types.SimpleNamespace(_pv_inputs=refs if len(refs) > 1 else refs[0], _pv_session=types.SimpleNamespace(device="cpu"))
    if detection:
        dep._pv_load_boxes = lambda b: None
    return dep


def test_video_batch_builds_the_region_records_on_the_host():
    """Two videos of different sizes, a SlowFast-like pair of pathways (2 and 8 frames of an 8-frame clip): the rectangle
    table of a pathway is the column subset `pathway_tables` takes of the frame table, the records hold the rectangle, the
    bits of the fp32 quotients and zeros, and the rows of the videos follow one another like the rows of the frame tables."""
    packer = TR.DevicePacker(_fake_deployed(4, (24, 32), frames=(2, 8)), frame_ratios=(4, 1), crop_size=(24, 32), src_layout="NTHWC",
                             regions=True)
    assert packer.window == (24, 32) and packer.views == (1,) and packer.clip_frames == 8
    videos = [torch.zeros((20, 40, 60, 3), dtype=torch.uint8), torch.zeros((9, 30, 30, 3), dtype=torch.uint8)]
    tables = [torch.arange(8)[None] + torch.tensor([[0], [12]]), torch.arange(8)[None] + 1]
    g = torch.Generator().manual_seed(11)
    regions = [TR.box_regions(torch.rand(2, 8, 4, generator=g) * 50.0, 40, 60), TR.box_regions(torch.rand(1, 8, 4, generator=g) * 30.0, 30, 30)]
    b = packer.video_batch(videos, tables, regions=regions)
    assert b.total == 3 and b.n_views == 1 and b.item_rows.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [1, 2, 0, 0]]
    assert [tuple(r.shape) for r in b.regions] == [(3, 2, 8), (3, 8, 8)] and all(r.dtype == torch.int32 and r.is_contiguous() for r in b.regions)
    whole = torch.cat(regions)
    for tab, rec, tp in zip(b.tables, b.regions, (2, 8)):
        cols = TR.temporal_indices(8, tp)
        assert torch.equal(tab, torch.cat(tables)[:, cols].to(torch.int32))
        assert torch.equal(rec[..., :4].long(), whole[:, cols]) and int(rec[..., 6:].abs().max()) == 0
        for row in range(3):
            for t in range(tp):
                top, left, h, w = whole[row, cols[t]].tolist()
                reg = L.ViewRegion.from_buffer_copy(rec[row, t].numpy().tobytes())
                assert (reg.top, reg.left, reg.h, reg.w) == (top, left, h, w)
                assert (reg.sy, reg.sx) == (_f32(h, 24), _f32(w, 32)) and tuple(reg.reserved) == (0, 0)
    assert (b.sources[0].Hs, b.sources[0].Ws, b.sources[1].Hs, b.sources[1].Ws) == (40, 60, 30, 30)
    assert all(rec.orient == 0 for rec in b.sources)


def test_video_batch_refuses_regions_it_cannot_honour():
    dep = _fake_deployed(4, (32, 32))
    video, table = torch.zeros((6, 40, 60, 3), dtype=torch.uint8), torch.arange(4)[None]
    ok = torch.tensor([0, 0, 40, 60]).expand(1, 4, 4)
    packer = TR.DevicePacker(dep, crop_size=32, src_layout="NTHWC", regions=True)
    assert packer.video_batch([video], [table], regions=[ok]).total == 1
    # three views: a rectangle is resized whole
    with pytest.raises(ValueError, match="one view"):
        TR.DevicePacker(_fake_deployed(3, (32, 32)), crop_size=32, spatial_idx=(0, 1, 2), src_layout="NTHWC", regions=True)
    three = TR.DevicePacker(_fake_deployed(3, (32, 32)), short_side=36, crop_size=32, spatial_idx=(0, 1, 2), src_layout="NTHWC")
    with pytest.raises(ValueError, match="short_side"):
        three.video_batch([video], [table], regions=[ok])
    with pytest.raises(ValueError, match="one view"):
        TR.build_video_batch([video], [table], "NTHWC", None, (32, 32), (0, 1, 2), [4], 3, torch.device("cpu"), lambda t: t, regions=[ok])
    # a short-side geometry contradicts them, on either side
    with pytest.raises(ValueError, match="short_side"):
        TR.DevicePacker(dep, short_side=36, crop_size=32, src_layout="NTHWC", regions=True)
    one = TR.DevicePacker(dep, short_side=36, crop_size=32, src_layout="NTHWC")
    with pytest.raises(ValueError, match="short_side"):
        one.video_batch([video], [table], regions=[ok])
    with pytest.raises(ValueError, match="regions="):
        packer.video_batch([video], [table])                     # and a regions packer takes nothing else
    with pytest.raises(RuntimeError, match="video_batch"):
        packer(torch.zeros((4, 3, 4, 40, 60), dtype=torch.uint8))
    with pytest.raises(ValueError, match="crop_size"):
        TR.DevicePacker(dep, src_layout="NTHWC", regions=True)
    with pytest.raises(ValueError, match="converted for"):
        TR.DevicePacker(dep, crop_size=(32, 24), src_layout="NTHWC", regions=True)
    # orientation and hdr are out of scope
    for orientation in (1, [4]):
        with pytest.raises(ValueError, match="orientation"):
            packer.video_batch([video], [table], orientation=orientation, regions=[ok])
    with pytest.raises(ValueError, match="hdr"):
        TR.DevicePacker(dep, crop_size=32, src_layout="P010", hdr="pq", regions=True)
    # a wrong table shape, rectangles outside the frame, float rectangles, odd members for a YUV layout
    for bad in (ok[:, :3], ok[0], ok.expand(2, 4, 4), torch.tensor([0, 0, 41, 60]).expand(1, 4, 4),
                torch.tensor([0, 1, 40, 60]).expand(1, 4, 4), torch.tensor([0, 0, 0, 60]).expand(1, 4, 4), ok.float()):
        with pytest.raises(ValueError):
            packer.video_batch([video], [table], regions=[bad])
    with pytest.raises(ValueError, match="region tables"):
        packer.video_batch([video], [table], regions=[ok, ok])
    nv12 = TR.DevicePacker(dep, crop_size=32, src_layout="NV12", regions=True)
    frames = torch.zeros((6, 60, 60), dtype=torch.uint8)                                # 40 x 60 luma over 20 rows of chroma
    assert nv12.video_batch([frames], [table], regions=[ok]).total == 1
    with pytest.raises(ValueError, match="even"):
        nv12.video_batch([frames], [table], regions=[torch.tensor([1, 0, 38, 60]).expand(1, 4, 4)])
    with pytest.raises(ValueError, match="KeyframeDetector"):
        TR.DevicePacker(_fake_deployed(4, (32, 32), detection=True), crop_size=32, src_layout="NTHWC", regions=True)
    with pytest.raises(ValueError, match="KeyframeDetector"):
        INF.TubePredictor(_fake_deployed(4, (32, 32), detection=True), 1.0, None, None, False, 32)


def test_device_resized_crop_refuses_bad_arguments_before_any_launch():
    clip5 = torch.zeros((2, 3, 4, 20, 30), dtype=torch.uint8)
    with pytest.raises(ValueError, match="src_layout"):
        TR.device_resized_crop(clip5, torch.zeros((2, 4, 4), dtype=torch.int64), 8, src_layout="RGB")
    with pytest.raises(ValueError, match="dtype"):
        TR.device_resized_crop(clip5, torch.zeros((2, 4, 4), dtype=torch.int64), 8, dtype=torch.float16)
    with pytest.raises(ValueError):
        TR.device_resized_crop(clip5, torch.zeros((2, 4, 4), dtype=torch.int64), (8, -1))
    import inspect
    assert "hdr" not in inspect.signature(TR.device_resized_crop).parameters
