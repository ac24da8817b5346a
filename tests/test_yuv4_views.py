"""YUV 4:2:2 and 4:4:4 (include/pv_mi355x.h "YUV 4:2:2 and 4:4:4": PV_SRC_YUV422, PV_SRC_YUV444), without a GPU: the layouts in
the C ABI of `pv_batch_views`, `pv_frame_views`, `pv_region_views` and `pv_area_views` -- validated before any launch, in the
positive-control style of tests/test_packed_views.py: nothing is launched, a valid descriptor is PV_ERR_UNSUPPORTED for an LDS
or index-limit reason, which shows that validation was passed --, the code-object metadata of the kernels of pv_yuv4.hip, and
the Python side: the strings, `yuv_geometry`, the host mirror `yuv_to_rgb` and the constructors."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import test_area_views as TA
import test_batch_views as TB
import test_clip_sampling as TCS
import test_frame_views as TF
import test_hdr_ingest as TH
import test_region_views as TRV
import test_transforms_spatial as TTS
import test_yuv16_ingest as TY16
import test_yuv_ingest as TY
import yuv4_util as Y4
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
W = TB.W
SIZES = ((2, W), (6, W))                                         # the two sources of the base descriptors
SUBS = {10: (0, 1), 11: (0, 0)}                                  # layout code -> (csy, csx)

# (entry point, frame list?)
ENTRIES = [("batch", False), ("frames", True), ("region", False), ("region", True), ("area", False), ("area", True)]
ENTRY_IDS = ["%s-%s" % (e, "frames" if f else "videos") for e, f in ENTRIES]
# every new layout x c_step x sample width
SOURCE_FORMS = [(code, c_step, sb) for code in (10, 11) for c_step in (1, 2) for sb in (1, 2)]


def _planes(rec, hs, ws, code, c_step, sb):
    """The dense planes of an hs x ws frame in a record: luma, then U and V (c_step 2: interleaved, U first)."""
    csy, csx = SUBS[code]
    hc, wc = (hs + csy) >> csy, (ws + csx) >> csx
    rec.y_pitch, rec.c_pitch = ws * sb, wc * c_step * sb
    rec.u_offset = hs * rec.y_pitch
    rec.v_offset = rec.u_offset + (sb if c_step == 2 else hc * rec.c_pitch)
    rec.frame_stride = hs * rec.y_pitch + hc * rec.c_pitch * (1 if c_step == 2 else 2)


def _yuv4_desc(keep, entry, frames, code=10, c_step=1, sb=1):
    """The NV12 base descriptor of the entry point's own test file (two sources of 2 x W and 6 x W, W = 40000, beyond the LDS
    limit of a staged strip and the index limit of the box filter) as a 4:2:2 / 4:4:4 launch.  Returns (status(), batch
    descriptor, records, pointer table or None, rectangles or None)."""
    regions = None
    if entry == "batch":
        outer, sources, _ = TB._desc(keep, True)
        d, ptrs, fn = outer, None, "pv_batch_views"
    elif entry == "frames":
        outer, sources, _, ptrs = TF._desc(keep, True)
        d, fn = outer.batch, "pv_frame_views"
    elif entry == "region":
        outer, sources, _, regions, ptrs = TRV._region_desc(keep, frames, True)
        d, fn = outer.frames.batch, "pv_region_views"
    else:
        outer, sources, _, ptrs = TA._area_desc(keep, frames, True)
        d, fn = outer.frames.batch, "pv_area_views"
    if code == 2:                                                # the NV12 base itself
        return (lambda: getattr(L.lib(), fn)(C.byref(outer), None)), d, sources, ptrs, regions
    d.src_layout, d.c_step, d.src_dtype = code, c_step, (L.PV_U16 if sb == 2 else L.PV_U8)
    for rec, (hs, ws) in zip(sources, SIZES):
        _planes(rec, hs, ws, code, c_step, sb)
    if sb == 2:                                                  # the bases stand at odd addresses: two-byte samples at even ones
        if ptrs is not None:
            for i in range(6):
                ptrs[i] -= 1
        else:
            sources[0].src -= sources[0].src % 2
    return (lambda: getattr(L.lib(), fn)(C.byref(outer), None)), d, sources, ptrs, regions


# ----------------------------------------------------------------------------- the ABI
def test_the_layout_values_are_the_headers(pv_lib):
    assert (L.SRC_YUV420, L.SRC_YUV422, L.SRC_YUV444) == (2, 10, 11)
    assert pv_lib.pv_version() == L.ABI_VERSION == 36
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "enum { PV_SRC_YUV422 = 10, PV_SRC_YUV444 = 11 };" in header
    assert "enum { PV_SRC_YUV420 = 2 };" in header
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16     # no struct gained or lost a byte


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_yuv4_descriptors_are_validated_before_any_launch(pv_lib, entry, frames):
    keep = []
    for code, c_step, sb in SOURCE_FORMS:                        # the positive control: every source form passes validation
        status, _, _, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
        assert status() == UNS, (code, c_step, sb)
    status, d, _, _, _ = _yuv4_desc(keep, entry, frames)
    d.src_layout = 9                                             # no layout
    assert status() == INV
    status, d, _, _, _ = _yuv4_desc(keep, entry, frames)
    d.src_layout = 12
    assert status() == INV
    for code, c_step, sb in SOURCE_FORMS:
        what = (code, c_step, sb)
        for index in (0, 1):
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            sources[index].y_pitch -= sb                         # pitches that do not hold a row
            assert status() == INV, what
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            sources[index].c_pitch -= sb * c_step
            assert status() == INV, what
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            sources[index].frame_stride -= sb                    # the last chroma row ends outside the frame
            assert status() == INV, what
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            sources[index].u_offset = -2 * sb
            assert status() == INV, what
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            sources[index].v_offset += 2 * sb                    # V leaves the frame; c_step 2: no interleaved pair either
            assert status() == INV, what
        if c_step == 2:                                          # |v_offset - u_offset| is one sample
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            for rec in sources:
                rec.frame_stride += 8
                rec.v_offset = rec.u_offset + 2 * sb
            assert status() == INV, what
            status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
            for rec in sources:                                  # V first: legal
                rec.u_offset, rec.v_offset = rec.v_offset, rec.u_offset
            assert status() == UNS, what
        status, d, _, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
        d.C = 4
        assert status() == INV, what
        status, d, _, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
        d.yuv2rgb = None
        assert status() == INV, what
        status, d, _, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
        d.c_step = 3
        assert status() == INV, what
        # an invalid field wins over the unsupported size
        status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, sb)
        sources[1].N = 0
        assert status() == INV, what
    status, d, _, _, _ = _yuv4_desc(keep, entry, frames)
    d.src_dtype = L.PV_F32
    assert status() in (INV, UNS) and status() != L.PV_OK


def _narrowed(keep, entry, frames, code, c_step, sb, ws):
    """The base launch with both sources `ws` wide and a window (and rectangles) that fit them."""
    status, d, sources, _, regions = _yuv4_desc(keep, entry, frames, code, c_step, sb)
    wo = ws - ws % 2
    d.Wo = wo
    for rec, (hs, _) in zip(sources, SIZES):
        rec.Ws, rec.Wn = ws, ws
        rec.sx = TB._f32(ws, ws)
        _planes(rec, hs, ws, code, c_step, sb)
    for reg in regions if regions is not None else ():
        TRV._set_region(reg, 0, 0, 2, wo, 1, wo)
    return status


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_the_sizes_a_layout_halves_are_even_and_no_others(pv_lib, entry, frames):
    keep = []
    for c_step in (1, 2):
        for sb in (1, 2):
            # 4:2:2: an odd Ws is invalid; 4:4:4 takes it (and says so by reaching the size limit)
            assert _narrowed(keep, entry, frames, 10, c_step, sb, W - 1)() == INV
            assert _narrowed(keep, entry, frames, 11, c_step, sb, W - 1)() == UNS
            assert _narrowed(keep, entry, frames, 10, c_step, sb, W - 2)() == UNS
    # an odd Hs: both take it (4:2:0 does not) -- source 1 is 5 x W, scaled to 3 x W as before
    for code, want in ((10, UNS), (11, UNS), (2, INV)):
        status, d, sources, _, _ = _yuv4_desc(keep, entry, frames, code)
        assert status() == UNS, code
        sources[1].Hs = 5
        sources[1].sy = TB._f32(5, 3)
        if code != 2:
            _planes(sources[1], 5, W, code, 1, 1)
        assert status() == want, code


@pytest.mark.parametrize("frames", [False, True], ids=["videos", "frames"])
def test_a_rectangle_is_even_only_where_the_subsampling_halves(pv_lib, frames):
    keep = []

    def with_region(code, top, left, h, w):
        status, _, _, _, regions = _yuv4_desc(keep, "region", frames, code)
        for reg in regions:
            TRV._set_region(reg, top, left, h, w, 1, W)
        return status()

    assert with_region(10, 0, 0, 2, W) == with_region(11, 0, 0, 2, W) == UNS
    assert with_region(10, 1, 0, 1, W) == UNS                    # 4:2:2: top and h may be odd
    assert with_region(10, 0, 1, 2, W - 2) == INV                # left may not
    assert with_region(10, 0, 0, 2, W - 1) == INV                # nor w
    assert with_region(10, 0, 2, 1, W - 2) == UNS
    assert with_region(11, 1, 1, 1, W - 1) == UNS                # 4:4:4: nothing is halved
    assert with_region(11, 0, 3, 2, W - 3) == UNS
    assert with_region(11, 0, 3, 2, W - 2) == INV                # still inside the frame


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_two_byte_samples_lie_at_even_bytes(pv_lib, entry, frames):
    keep = []
    for code in (10, 11):
        for c_step in (1, 2):
            for field in ("y_pitch", "c_pitch", "frame_stride", "u_offset", "v_offset"):
                status, _, sources, _, _ = _yuv4_desc(keep, entry, frames, code, c_step, 2)
                for rec in sources:
                    rec.frame_stride += 64                       # room for what grows
                setattr(sources[1], field, getattr(sources[1], field) + 1)
                assert status() == INV, (code, c_step, field)
            status, _, sources, ptrs, _ = _yuv4_desc(keep, entry, frames, code, c_step, 2)
            if ptrs is not None:
                ptrs[3] += 1                                     # a frame of source 1's slice
            else:
                sources[1].src += 1
            assert status() == INV, (code, c_step)


def test_the_other_entry_points_refuse_the_new_layouts(pv_lib):
    keep = []
    for code in (10, 11):
        for frames in (False, True):                             # pv_hdr_views: 16-bit 4:2:0 only
            h, _, _ = TH._hdr_desc(keep, frames)
            assert TH._status(h) == UNS                          # the base: valid, too large
            h.frames.batch.src_layout = code
            assert TH._status(h) == UNS, code
            h, _, _ = TH._hdr_desc(keep, frames)
            h.frames.batch.src_layout, h.frames.batch.src_dtype = code, L.PV_U8
            assert TH._status(h) == UNS, code
        d = TTS._desc(keep)                                      # pv_resample_crop
        d.src_layout, d.src_dtype, d.C = code, L.PV_U8, 3
        assert TTS._status(d) == INV, code
        d = TCS._desc(keep)                                      # pv_video_views
        d.src_layout, d.src_dtype, d.C = code, L.PV_U8, 3
        assert TCS._status(d) == INV, code
    # pv_yuv_views / pv_yuv16_views have no field for a layout: their descriptors are what they were
    assert not hasattr(TY._desc(keep), "src_layout") and not hasattr(TY16._desc(keep), "src_layout")
    assert C.sizeof(L.YuvViewsDesc) == C.sizeof(type(TY._desc(keep)))


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_yuv4(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_yuv4") / "pv_yuv4.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_yuv4.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_yuv4_kernel_is_free_of_scratch_and_spills(asm_yuv4):
    """4 bodies x 2 chroma arrangements x 2 sample widths x 5 destination forms -- the subsampling is a kernel argument, not a
    kernel --: 80 kernels, no private segment and no spilled register.  The register counts are printed
    (profiles/r27/resource_usage.md records them)."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_yuv4, re.S)
    names = [k for k, _ in kernels]
    for body in ("yuv4_views_kernel", "yuv4_orient_kernel", "yuv4_region_kernel", "yuv4_area_kernel"):
        for c_step in (1, 2):
            for smp in ("h", "t"):                               # unsigned char / unsigned short
                assert len([n for n in names if "%sILi%dE%s" % (body, c_step, smp) in n]) == 5, (body, c_step, smp)
    assert len(kernels) == 80, names
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


def test_the_new_unit_is_built_into_the_library():
    from pytorchvideo_amd.csrc import build as B
    assert "pv_yuv4.hip" in B.SOURCES and os.path.exists(os.path.join(B.HERE, "pv_yuv4.hip"))


# ----------------------------------------------------------------------------- Python: the strings and the geometry
def test_the_layout_tuples():
    assert TR.YUV422_LAYOUTS == ("I422", "YV16", "NV16", "NV61", "P210", "P212", "P216", "I210", "I212", "I216")
    assert TR.YUV444_LAYOUTS == ("I444", "YV24", "I410", "I412", "I416")
    assert TR.YUV_LAYOUTS == ("NV12", "NV21", "I420", "YV12")                      # the 4:2:0 tuples are what they were
    assert TR.YUV16_LAYOUTS == ("P010", "P012", "P016", "I010", "I012", "I016")
    assert set(Y4.LAYOUT) >= set(TR.YUV422_LAYOUTS + TR.YUV444_LAYOUTS)
    for layout in TR.YUV422_LAYOUTS + TR.YUV444_LAYOUTS:
        sub, _, _, sb, _, _ = Y4.LAYOUT[layout]
        assert TR._src_codes(layout, None) == (Y4.CODE[sub], L.PV_U16 if sb == 2 else L.PV_U8), layout
        assert TR.region_evenness(layout) == ("width" if sub == (0, 1) else False)
    assert TR.region_evenness("NV12") is True and TR.region_evenness("P010") is True
    assert TR.region_evenness("NTHWC") is False and TR.region_evenness("BGRA") is False
    assert "NV24" not in TR._SRC_LAYOUTS                         # reachable through the C ABI only


def _contiguous(layout, n, hc, w):
    sub, _, _, sb, _, _ = Y4.LAYOUT[layout]
    rows = hc * (2 if sub == (0, 1) else 3)
    return torch.zeros((n, rows, w), dtype=torch.uint8 if sb == 1 else torch.int16)


@pytest.mark.parametrize("layout", TR.YUV422_LAYOUTS + TR.YUV444_LAYOUTS)
def test_yuv_geometry_of_contiguous_frames(layout):
    sub, c_step, v_first, sb, _, _ = Y4.LAYOUT[layout]
    hc, w = 5, (12 if sub[1] else 11)                            # odd heights; 4:4:4: an odd width
    g = TR.yuv_geometry(_contiguous(layout, 3, hc, w), layout)
    first = hc * w
    if c_step == 2:
        a, b, c_pitch = first, first + 1, w
    else:
        c_pitch = w >> sub[1]
        a, b = first, first + hc * c_pitch
    u, v = (b, a) if v_first else (a, b)
    rows = hc * (2 if sub[1] else 3)
    assert g == dict(N=3, Hs=hc, Ws=w, Hc=hc, frame_stride=rows * w * sb, y_pitch=w * sb, c_pitch=c_pitch * sb, c_step=c_step,
                     u_offset=u * sb, v_offset=v * sb, csy=0, csx=sub[1])
    if sb == 2:                                                  # uint16 and int16 are the same frames
        assert TR.yuv_geometry(_contiguous(layout, 3, hc, w).view(torch.uint16), layout) == g
    # clips [B, T, rows, W] are one sequence of frames
    assert TR.yuv_geometry(_contiguous(layout, 6, hc, w).reshape(2, 3, rows, w), layout)["N"] == 6
    # the 4:2:0 results carry no new key
    assert "csy" not in TR.yuv_geometry(torch.zeros((2, 18, 12), dtype=torch.uint8), "NV12")


@pytest.mark.parametrize("layout", ["I422", "NV16", "NV61", "I210", "P210", "I444", "YV24", "I410"])
def test_yuv_geometry_of_pitched_frames_with_a_coded_height(layout):
    """The test surfaces: pitched, an offset base, a coded height above the display height -- yuv_geometry reads the very
    fields the surface was built with."""
    sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT[layout]
    h, w = (7, 10) if sub[1] else (7, 9)
    s = Y4.surface_of(layout, *Y4.planes(3, h, w, sub, 5, sb, bits, msb))
    assert not s.view.is_contiguous()
    g = TR.yuv_geometry(s.view, layout, height=h)
    assert {k: g[k] for k in s.geom} == s.geom and (g["csy"], g["csx"]) == sub
    assert TR.yuv_geometry(s.view, layout, coded_height=s.hc, height=h) == g
    assert TR.yuv_geometry(s.view, layout)["Hs"] == s.hc         # the default display height is the coded one
    with pytest.raises(RuntimeError, match="coded_height"):
        TR.yuv_geometry(s.view, layout, coded_height=s.hc + 1)
    with pytest.raises(RuntimeError, match="display height"):
        TR.yuv_geometry(s.view, layout, height=s.hc + 1)
    one = TR.FrameList(list(s.view.unbind(0)), layout).geometry(layout, None, h)
    assert one[:3] == (3, h, w) and one[3]["y_pitch"] == g["y_pitch"] and one[3]["u_offset"] == g["u_offset"]


def test_yuv_geometry_errors():
    with pytest.raises(RuntimeError, match="even width"):        # 4:2:2: an odd W
        TR.yuv_geometry(torch.zeros((2, 10, 11), dtype=torch.uint8), "I422")
    assert TR.yuv_geometry(torch.zeros((2, 15, 11), dtype=torch.uint8), "I444")["Ws"] == 11
    with pytest.raises(RuntimeError, match="rows"):              # wrong row counts
        TR.yuv_geometry(torch.zeros((2, 11, 12), dtype=torch.uint8), "NV16")
    with pytest.raises(RuntimeError, match="rows"):
        TR.yuv_geometry(torch.zeros((2, 10, 12), dtype=torch.uint8), "I444")
    for layout, dtype in (("I422", torch.int16), ("I210", torch.uint8), ("I444", torch.float32), ("I410", torch.uint8),
                          ("P210", torch.int32)):
        with pytest.raises(RuntimeError, match="frames are"):    # wrong dtypes
            TR.yuv_geometry(torch.zeros((2, 12, 12), dtype=dtype), layout)
    with pytest.raises(RuntimeError, match="pitch"):             # planar 4:2:2: chroma rows at half an odd pitch
        TR.yuv_geometry(torch.zeros((2, 10, 13), dtype=torch.uint8)[:, :, :12], "I422")
    assert TR.yuv_geometry(torch.zeros((2, 10, 13), dtype=torch.uint8)[:, :, :12], "NV16")["c_pitch"] == 13
    with pytest.raises(ValueError, match="YUV layout"):
        TR.yuv_geometry(torch.zeros((2, 12, 12), dtype=torch.uint8), "NV24")


# ----------------------------------------------------------------------------- Python: the host mirror
def test_yuv_to_rgb_is_yuv420_to_rgb_on_420_input():
    m = TR.yuv_matrix("bt601", False)
    for layout in ("NV12", "NV21", "I420", "YV12", "P010", "I010"):
        sub, c_step, v_first, sb, bits, msb = Y4.LAYOUT.get(layout, (Y4.SUB420, 2 if layout == "NV21" else 1,
                                                                     layout in ("NV21", "YV12"), 1, 8, False))
        s = Y4.Surface(*Y4.planes(2, 8, 12, Y4.SUB420, 11, sb, bits, msb), Y4.SUB420, c_step, v_first, sb, seed=3)
        mm = TR._yuv_matrix_of(("bt601", False), layout)
        a = TR.yuv_to_rgb(s.view, layout, mm, height=8)
        b = TR.yuv420_to_rgb(s.view, layout, mm, height=8)
        assert a.shape == (2, 3, 8, 12) and torch.equal(a, b), layout
    with pytest.raises(ValueError, match="4:2:0"):
        TR.yuv420_to_rgb(torch.zeros((2, 10, 12), dtype=torch.uint8), "I422", m)


def test_yuv_to_rgb_of_i444_with_a_selecting_matrix_is_the_planes():
    y, u, v = Y4.planes(2, 7, 9, Y4.SUB444, 21)
    pick = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], dtype=torch.float64)   # R = Y, G = U, B = V
    for layout, order in (("I444", (y, u, v)), ("YV24", (y, u, v))):
        s = Y4.surface_of(layout, y, u, v, seed=4)
        got = TR.yuv_to_rgb(s.view, layout, pick, height=7)
        assert got.dtype == torch.float32 and torch.equal(got, torch.stack(order, 1).float()), layout
    # 4:2:2: the chroma columns are replicated, the rows are not
    y, u, v = Y4.planes(2, 7, 10, Y4.SUB422, 22)
    for layout in ("I422", "NV16", "NV61", "YV16"):
        got = TR.yuv_to_rgb(Y4.surface_of(layout, y, u, v, seed=5).view, layout, pick, height=7)
        assert torch.equal(got, torch.stack([y, u.repeat_interleave(2, 2), v.repeat_interleave(2, 2)], 1).float()), layout
    # 16-bit codes are read unsigned, whichever of uint16 / int16 the tensor is
    y, u, v = Y4.planes(2, 5, 6, Y4.SUB444, 23, sb=2, bits=16)
    s = Y4.surface_of("I416", y, u, v, seed=6)
    assert int(y.max()) > 40000
    pick16 = pick * (255.0 / 65535.0)
    want = torch.stack([y, u, v], 1).double() * (255.0 / 65535.0)
    for view in (s.view, s.view.view(torch.uint16)):
        assert torch.equal(TR.yuv_to_rgb(view, "I416", pick16, height=5), want.float())
    # depth and alignment go into the matrix: P210's is I210's scaled by 2^-6, exactly
    assert torch.equal(TR._yuv_matrix_of(("bt709", False), "P210")[:, :3] * 64.0, TR._yuv_matrix_of(("bt709", False), "I210")[:, :3])
    assert torch.equal(TR._yuv_matrix_of(("bt709", False), "I410"), TR.yuv_matrix("bt709", False, 10, False))
    assert torch.equal(TR._yuv_matrix_of(("bt709", True), "I444"), TR.yuv_matrix("bt709", True))


# ----------------------------------------------------------------------------- Python: the constructors
def _dep(batch=4, size=(32, 32), detection=False):
    return TRV._fake_deployed(batch, size, detection=detection)


def _det():
    dep = _dep(2, (36, 54), detection=True)
    dep._pv_box_capacity, dep._pv_box_ptr = 5, None
    return dep


@pytest.mark.parametrize("layout", TR.YUV422_LAYOUTS + TR.YUV444_LAYOUTS)
def test_every_constructor_takes_the_new_strings(layout):
    sampler = D.UniformClipSampler(1)
    sub, _, _, sb, _, _ = Y4.LAYOUT[layout]
    p = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout)
    assert p.is_yuv and p.is_yuv4 and p.item_only and p.in_place and not p.is_packed and p.is_yuv16 == (sb == 2)
    assert p.yuv_matrix is not None and p.region_even == ("width" if sub == (0, 1) else False)
    assert TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, interpolation="area").area
    assert TR.DevicePacker(_dep(), crop_size=32, src_layout=layout, regions=True).region_mode
    assert TR.DevicePacker(_dep(2, (36, 54), detection=True), short_side=36, src_layout=layout, keyframes=True).no_crop
    frame = _contiguous(layout, 1, 40, 60)[0]
    assert TR.FrameList([frame] * 3, layout).geometry(layout)[:3] == (3, 40, 60)
    assert INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.VideoBatchPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.StreamPredictor(_dep(), 1.0, 1.0, 4, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.KeyframeDetector(_det(), 1.0, None, None, False, 36, src_layout=layout).packer.is_yuv4
    assert INF.TubePredictor(_dep(), 1.0, None, None, False, 32, src_layout=layout).packer.is_yuv4
    # hdr= is a ValueError that says so
    clip = _contiguous(layout, 2, 40, 60)[None]
    for make in (lambda: TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, hdr="pq"),
                 lambda: INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout, hdr="hlg"),
                 lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout, hdr="pq")):
        with pytest.raises(ValueError, match="hdr.*4:2:2 / 4:4:4"):
            make()
    # the functions take the string: what stops them on a machine without a GPU is the device, never the layout
    for call in (lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout),
                 lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout, interpolation="area"),
                 lambda: TR.device_resized_crop(clip, torch.tensor([[[1, 2, 21, 20]] * 2]), 32, src_layout=layout)):
        try:
            call()
        except ValueError as e:                                  # pragma: no cover - the failure this test is for
            pytest.fail("%s refused: %s" % (layout, e))
        except (RuntimeError, AssertionError):
            assert not torch.cuda.is_available()


def test_the_records_of_a_video_batch_carry_the_planes():
    table = torch.arange(4)[None] % 3
    for layout in ("I422", "NV16", "I210", "I444", "I410"):
        sub, _, _, sb, bits, msb = Y4.LAYOUT[layout]
        s = Y4.surface_of(layout, *Y4.planes(3, 40, 60, sub, 31, sb, bits, msb))
        for packer in (TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, height=40),
                       TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, height=40, interpolation="area")):
            batch = packer.video_batch([s.view], [table])
            rec = batch.sources[0]
            assert rec.src == s.view.data_ptr() and batch.videos[0] is s.view
            assert {k: getattr(rec, k) for k in TR._YUV_PLANE_FIELDS} == {k: s.geom[k] for k in TR._YUV_PLANE_FIELDS}
            assert (rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (3, 40, 60, 36, 54)
            assert batch.src_dtype == (L.PV_U16 if sb == 2 else L.PV_U8)
        frames = TR.FrameList([s.view[i] for i in (2, 0, 1)], layout)
        batch = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, height=40).video_batch([frames], [table])
        assert batch.frame_ptrs.tolist() == [f.data_ptr() for f in frames.frames] and batch.sources[0].N == 3


def test_tube_rectangles_are_even_where_the_layout_needs_it():
    boxes = torch.tensor([[3.2, 5.1, 20.7, 30.3], [7.0, 1.0, 9.0, 2.0]])
    r422 = TR.box_regions(boxes, 41, 60, even="width")
    top, left, h, w = r422.unbind(-1)
    assert bool((left % 2 == 0).all()) and bool((w % 2 == 0).all()) and top.tolist() == [5, 1] and h.tolist() == [26, 1]
    assert torch.equal(TR.box_regions(boxes, 41, 61, even=False), TR.box_regions(boxes, 41, 61))
    with pytest.raises(ValueError, match="width is even"):
        TR.box_regions(boxes, 41, 61, even="width")
    assert torch.equal(TR.box_regions(boxes, 40, 60, even=True) % 2, torch.zeros((2, 4), dtype=torch.int64))
    tubes = TR.DevicePacker(_dep(), crop_size=32, src_layout="I422", regions=True)
    video = _contiguous("I422", 4, 41, 60)
    table = torch.arange(4)[None]
    ok = tubes.video_batch([video], [table], regions=[r422[:1, None].expand(1, 4, 4)])
    assert ok.regions is not None
    with pytest.raises(ValueError, match="even left and w"):
        tubes.video_batch([video], [table], regions=[torch.tensor([[[5, 3, 26, 18]] * 4])])
    tubes = TR.DevicePacker(_dep(), crop_size=32, src_layout="I444", regions=True)
    assert tubes.video_batch([_contiguous("I444", 4, 41, 61)], [table], regions=[torch.tensor([[[5, 3, 25, 17]] * 4])]).regions is not None
