"""Packed YUV 4:2:2 (include/pv_mi355x.h "packed YUV 4:2:2": PV_SRC_YUYV422), without a GPU: the layout in the C ABI of
`pv_batch_views`, `pv_frame_views`, `pv_region_views` and `pv_area_views` -- validated before any launch, in the
positive-control style of tests/test_yuv4_views.py: nothing is launched, a valid descriptor is PV_ERR_UNSUPPORTED for an LDS or
index-limit reason, which shows that validation was passed --, the code-object metadata of the kernels of pv_yuyv.hip, and the
Python side: the strings, `yuyv_geometry`, the host mirrors `yuyv_to_planar` / `yuv_to_rgb` and the constructors."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import test_clip_sampling as TCS
import test_hdr_ingest as TH
import test_region_views as TRV
import test_transforms_spatial as TTS
import test_yuv4_views as T4
import yuyv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR

ROOT, HIPCC = T4.ROOT, T4.HIPCC
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
W, SIZES = T4.W, T4.SIZES
ENTRIES, ENTRY_IDS = T4.ENTRIES, T4.ENTRY_IDS
SOURCE_FORMS = [(sb, order) for sb in (1, 2) for order in YU.ORDERS]


def _packed(rec, hs, ws, sb, order="YUY2"):
    """The tight one-plane frame of hs x ws in a record."""
    us, vs = YU.ORDERS[order]
    rec.y_pitch, rec.c_pitch = 2 * ws * sb, 0
    rec.u_offset, rec.v_offset = us * sb, vs * sb
    rec.frame_stride = hs * rec.y_pitch


def _desc(keep, entry, frames, sb=1, order="YUY2"):
    """The base descriptor of tests/test_yuv4_views.py (two sources of 2 x W and 6 x W, W = 40000: beyond the LDS limit of a
    staged strip and the index limit of the box filter) as a packed 4:2:2 launch."""
    status, d, sources, ptrs, regions = T4._yuv4_desc(keep, entry, frames, 10, 1, sb)
    d.src_layout, d.c_step = 13, 4
    for rec, (hs, ws) in zip(sources, SIZES):
        _packed(rec, hs, ws, sb, order)
    return status, d, sources, ptrs, regions


# ----------------------------------------------------------------------------- the ABI
def test_the_layout_value_is_the_headers(pv_lib):
    assert L.SRC_YUYV422 == 13
    assert pv_lib.pv_version() == L.ABI_VERSION == 36
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "enum { PV_SRC_YUYV422 = 13 };" in header and "The value 12 is no layout" in header
    assert "/* ---- packed YUV 4:2:2" in header
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16     # no struct gained or lost a byte


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_packed_422_descriptors_are_validated_before_any_launch(pv_lib, entry, frames):
    keep = []
    for sb, order in SOURCE_FORMS:                               # the positive control: every sample order passes validation
        status, _, _, _, _ = _desc(keep, entry, frames, sb, order)
        assert status() == UNS, (sb, order)
    status, d, _, _, _ = _desc(keep, entry, frames)
    d.src_layout = 12                                            # still no layout
    assert status() == INV
    for sb in (1, 2):
        valid = set(YU.ORDERS.values())
        pairs = [(u, v) for u in range(-1, 6) for v in range(-1, 6) if (u, v) not in valid]
        # among them (0, SB) and (SB, 2 SB), equal offsets, offsets of 4 SB and beyond, negative ones
        assert all(p in pairs for p in ((0, 1), (1, 2), (0, 0), (1, 1), (3, 3), (4, 2), (1, 4), (5, 3), (2, 4), (-1, 1)))
        for u, v in pairs:                                       # every other pair of sample positions
            status, _, sources, _, _ = _desc(keep, entry, frames, sb)
            sources[1].u_offset, sources[1].v_offset = u * sb, v * sb
            assert status() == INV, (sb, u, v)
        for c_step in (1, 2, 3, 0, 8):
            status, d, _, _, _ = _desc(keep, entry, frames, sb)
            d.c_step = c_step
            assert status() == INV, (sb, c_step)
        for index in (0, 1):
            status, _, sources, _, _ = _desc(keep, entry, frames, sb)
            sources[index].c_pitch = 2 * sb
            assert status() == INV, sb
            status, _, sources, _, _ = _desc(keep, entry, frames, sb)
            sources[index].y_pitch -= sb                         # a pitch that does not hold a row
            assert status() == INV, sb
            status, _, sources, _, _ = _desc(keep, entry, frames, sb)
            sources[index].frame_stride -= sb                    # the last row ends outside the frame
            assert status() == INV, sb
        status, _, sources, _, _ = _desc(keep, entry, frames, sb)
        for rec in sources:                                      # a pitched surface with room behind every frame: legal
            rec.y_pitch += 6 * sb
            rec.frame_stride = rec.Hs * rec.y_pitch + 2 * sb
        assert status() == UNS, sb
        status, d, _, _, _ = _desc(keep, entry, frames, sb)
        d.C = 4
        assert status() == INV, sb
        status, d, _, _, _ = _desc(keep, entry, frames, sb)
        d.yuv2rgb = None
        assert status() == INV, sb
        status, _, sources, _, _ = _desc(keep, entry, frames, sb)     # an invalid field wins over the unsupported size
        sources[1].N = 0
        assert status() == INV, sb
    status, d, _, _, _ = _desc(keep, entry, frames)              # c_step 4 is this layout's alone
    d.src_layout, d.c_step = 10, 4
    assert status() == INV
    status, d, _, _, _ = _desc(keep, entry, frames)
    d.src_dtype = L.PV_F32
    assert status() in (INV, UNS) and status() != L.PV_OK


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_the_width_is_even_and_the_height_is_any(pv_lib, entry, frames):
    keep = []

    def narrowed(sb, ws):
        status, d, sources, _, regions = _desc(keep, entry, frames, sb)
        wo = ws - ws % 2
        d.Wo = wo
        for rec, (hs, _) in zip(sources, SIZES):
            rec.Ws, rec.Wn = ws, ws
            rec.sx = T4.TB._f32(ws, ws)
            _packed(rec, hs, ws, sb)
        for reg in regions if regions is not None else ():
            TRV._set_region(reg, 0, 0, 2, wo, 1, wo)
        return status

    for sb in (1, 2):
        assert narrowed(sb, W - 1)() == INV
        assert narrowed(sb, W - 2)() == UNS
        status, _, sources, _, _ = _desc(keep, entry, frames, sb)
        sources[1].Hs = 5                                        # an odd Hs, scaled to 3 x W as before
        sources[1].sy = T4.TB._f32(5, 3)
        _packed(sources[1], 5, W, sb)
        assert status() == UNS, sb


@pytest.mark.parametrize("frames", [False, True], ids=["videos", "frames"])
def test_a_rectangle_has_an_even_left_and_w(pv_lib, frames):
    keep = []

    def with_region(sb, top, left, h, w):
        status, _, _, _, regions = _desc(keep, "region", frames, sb)
        for reg in regions:
            TRV._set_region(reg, top, left, h, w, 1, W)
        return status()

    for sb in (1, 2):
        assert with_region(sb, 0, 0, 2, W) == UNS
        assert with_region(sb, 1, 0, 1, W) == UNS                # top and h may be odd
        assert with_region(sb, 0, 2, 1, W - 2) == UNS
        assert with_region(sb, 0, 1, 2, W - 2) == INV            # left may not
        assert with_region(sb, 0, 0, 2, W - 1) == INV            # nor w
        assert with_region(sb, 0, 2, 2, W) == INV                # and the rectangle stays inside the frame


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_two_byte_samples_lie_at_even_bytes(pv_lib, entry, frames):
    keep = []
    for field in ("y_pitch", "frame_stride", "u_offset", "v_offset"):
        status, _, sources, _, _ = _desc(keep, entry, frames, 2)
        for rec in sources:
            rec.frame_stride += 64                               # room for what grows
        setattr(sources[1], field, getattr(sources[1], field) + 1)
        assert status() == INV, field
    status, _, sources, ptrs, _ = _desc(keep, entry, frames, 2)
    if ptrs is not None:
        ptrs[3] += 1                                             # a frame of source 1's slice
    else:
        sources[1].src += 1
    assert status() == INV
    # one-byte samples start at any byte: the base descriptors stand at odd addresses already; an odd pitch is legal too
    status, _, sources, ptrs, _ = _desc(keep, entry, frames, 1)
    assert ((ptrs[3] if ptrs is not None else sources[0].src) & 1) == 1
    for rec in sources:
        rec.y_pitch += 1
        rec.frame_stride = rec.Hs * rec.y_pitch + 1
    assert status() == UNS


def test_the_other_entry_points_refuse_the_new_layout(pv_lib):
    keep = []
    for frames in (False, True):                                 # pv_hdr_views: 16-bit 4:2:0 only
        h, _, _ = TH._hdr_desc(keep, frames)
        assert TH._status(h) == UNS                              # the base: valid, too large
        h.frames.batch.src_layout, h.frames.batch.c_step = 13, 4
        assert TH._status(h) == UNS
        h, _, _ = TH._hdr_desc(keep, frames)
        h.frames.batch.src_layout, h.frames.batch.c_step, h.frames.batch.src_dtype = 13, 4, L.PV_U8
        assert TH._status(h) == UNS
    d = TTS._desc(keep)                                          # pv_resample_crop
    d.src_layout, d.src_dtype, d.C = 13, L.PV_U8, 3
    assert TTS._status(d) == INV
    d = TCS._desc(keep)                                          # pv_video_views
    d.src_layout, d.src_dtype, d.C = 13, L.PV_U8, 3
    assert TCS._status(d) == INV
    d = T4.TY._desc(keep)                                        # pv_yuv_views / pv_yuv16_views: no layout field, and no c_step 4
    d.c_step = 4
    assert T4.TY._status(d) == INV
    d = T4.TY16._desc(keep)
    d.c_step = 4
    assert T4.TY16._status(d) == INV


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_yuyv(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_yuyv") / "pv_yuyv.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_yuyv.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_yuyv_kernel_is_free_of_scratch_and_spills(asm_yuyv):
    """4 bodies x 2 sample widths x 5 destination forms -- the sample order is read from the record, not a kernel --: 40
    kernels, no private segment and no spilled register.  The register counts are printed
    (profiles/r28/yuyv_resource_usage.md records them)."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_yuyv, re.S)
    names = [k for k, _ in kernels]
    for body in ("yuyv_views_kernel", "yuyv_orient_kernel", "yuyv_region_kernel", "yuyv_area_kernel"):
        for smp in ("h", "t"):                                   # unsigned char / unsigned short
            assert len([n for n in names if "%sI%sLi" % (body, smp) in n]) == 5, (body, smp)
    assert len(kernels) == 40, names
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


def test_the_new_unit_is_built_into_the_library():
    from pytorchvideo_amd.csrc import build as B
    assert "pv_yuyv.hip" in B.SOURCES and os.path.exists(os.path.join(B.HERE, "pv_yuyv.hip"))


# ----------------------------------------------------------------------------- Python: the strings and the geometry
def test_the_layout_tuples():
    assert TR.YUYV_LAYOUTS == ("YUY2", "YVYU", "UYVY", "Y210", "Y212", "Y216")
    assert TR.YUV422_LAYOUTS == ("I422", "YV16", "NV16", "NV61", "P210", "P212", "P216", "I210", "I212", "I216")   # as they were
    assert TR.YUV444_LAYOUTS == ("I444", "YV24", "I410", "I412", "I416")
    assert TR.YUV_LAYOUTS == ("NV12", "NV21", "I420", "YV12") and TR.YUV16_LAYOUTS == ("P010", "P012", "P016", "I010", "I012", "I016")
    assert TR.PACKED_LAYOUTS == ("BGR", "RGBA", "BGRA", "ARGB", "ABGR")
    assert set(YU.LAYOUT) == set(TR.YUYV_LAYOUTS)
    for layout in TR.YUYV_LAYOUTS + ("YUYV",):
        sb = YU.LAYOUT.get(layout, YU.LAYOUT["YUY2"])[1]
        assert TR._src_codes(layout, None) == (13, L.PV_U16 if sb == 2 else L.PV_U8), layout
        assert TR.region_evenness(layout) == "width" and layout in TR._SRC_LAYOUTS
        assert TR._yuv_c_step(layout) == 4
    assert "VYUY" not in TR._SRC_LAYOUTS                         # reachable through the C ABI only
    assert str(TR.YUYV_LAYOUTS) in TR._LAYOUT_ERROR
    with pytest.raises(ValueError, match="YUY2"):
        TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout="VYUY")
    # Y21x: the value in the high bits, composed into the matrix like P21x
    for layout, twin in (("Y210", "P210"), ("Y212", "P212"), ("Y216", "P216")):
        assert torch.equal(TR._yuv_matrix_of(("bt709", False), layout), TR._yuv_matrix_of(("bt709", False), twin))
    assert torch.equal(TR._yuv_matrix_of(("bt601", True), "UYVY"), TR.yuv_matrix("bt601", True))


def _tight(layout, n, h, w):
    sb = YU.LAYOUT[layout][1]
    return torch.zeros((n, h, w, 2), dtype=torch.uint8 if sb == 1 else torch.int16)


@pytest.mark.parametrize("layout", TR.YUYV_LAYOUTS)
def test_yuyv_geometry(layout):
    order, sb, bits, msb = YU.LAYOUT[layout]
    us, vs = YU.ORDERS[order]
    base = dict(N=3, Hs=5, Ws=12, Hc=5, c_pitch=0, c_step=4, u_offset=us * sb, v_offset=vs * sb, csy=0, csx=1)
    g = TR.yuyv_geometry(_tight(layout, 3, 5, 12), layout)
    assert g == dict(base, frame_stride=5 * 24 * sb, y_pitch=24 * sb)
    assert TR.yuv_geometry(_tight(layout, 3, 5, 12), layout) == g and TR.yuv_geometry(_tight(layout, 3, 5, 12), layout, 5, 5) == g
    if layout == "YUY2":
        assert TR.yuyv_geometry(_tight(layout, 3, 5, 12), "YUYV") == g
    if sb == 2:                                                  # uint16 and int16 are the same frames
        assert TR.yuyv_geometry(_tight(layout, 3, 5, 12).view(torch.uint16), layout) == g
    # a pitched surface, and a column slice of it that starts at an even column: read in place
    wide = _tight(layout, 3, 5, 20)
    assert TR.yuyv_geometry(wide[:, :, :12], layout) == dict(base, frame_stride=5 * 40 * sb, y_pitch=40 * sb)
    sliced = wide[:, :, 4:16]
    assert TR.yuyv_geometry(sliced, layout) == dict(base, frame_stride=5 * 40 * sb, y_pitch=40 * sb)
    assert sliced.data_ptr() == wide.data_ptr() + 8 * sb
    # one frame: its extent is the frame stride; rows [1, 4) of a frame
    one = TR.yuyv_geometry(wide[1, :, :12], layout)
    assert one == dict(base, N=1, frame_stride=(4 * 40 + 24) * sb, y_pitch=40 * sb)
    assert TR.yuyv_geometry(wide[:, 1:4, :12], layout)["Hs"] == 3
    # the test surfaces: yuyv_geometry reads the very fields the surface was built with
    s = YU.packed_of(layout, *YU.planes(3, 7, 10, 5, sb, bits, msb))
    assert not s.view.is_contiguous()
    got = TR.yuyv_geometry(s.view, layout)
    assert {k: got[k] for k in s.geom} == s.geom
    # clips [B, T, H, W, 2] are one sequence of frames
    assert TR.yuv_geometry(_tight(layout, 6, 5, 12).reshape(2, 3, 5, 12, 2), layout)["N"] == 6
    lst = TR.FrameList(list(s.view.unbind(0)), layout).geometry(layout)
    assert lst[:3] == (3, 7, 10) and lst[3]["y_pitch"] == got["y_pitch"] and lst[3]["u_offset"] == got["u_offset"]


def test_yuyv_geometry_refuses_every_other_stride():
    x = torch.zeros((3, 6, 12, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"stride\(-1\) is 2"):
        TR.yuyv_geometry(torch.zeros((3, 6, 12, 4), dtype=torch.uint8)[..., ::2], "YUY2")
    with pytest.raises(ValueError, match=r"stride\(-2\) is 4"):
        TR.yuyv_geometry(torch.zeros((3, 6, 24, 2), dtype=torch.uint8)[:, :, ::2], "YUY2")
    with pytest.raises(ValueError, match=r"stride\(-2\) is 12"):     # a transposed frame
        TR.yuyv_geometry(torch.zeros((3, 12, 6, 2), dtype=torch.uint8).transpose(1, 2), "UYVY")
    with pytest.raises(ValueError, match="row stride"):          # overlapping rows
        TR.yuyv_geometry(x.as_strided((3, 6, 12, 2), (144, 20, 2, 1)), "YUY2")
    with pytest.raises(ValueError, match="frame stride"):        # overlapping frames
        TR.yuyv_geometry(x.as_strided((3, 6, 12, 2), (100, 24, 2, 1)), "YUY2")
    with pytest.raises(ValueError, match="W is even"):           # half a macropixel
        TR.yuyv_geometry(torch.zeros((3, 6, 11, 2), dtype=torch.uint8), "YUY2")
    with pytest.raises(ValueError, match="W is even"):           # a column slice of an odd width
        TR.yuyv_geometry(x[:, :, 2:9], "YUY2")
    for layout, dtype in (("YUY2", torch.int16), ("Y210", torch.uint8), ("UYVY", torch.float32), ("Y216", torch.int32)):
        with pytest.raises(ValueError, match="frames are"):      # wrong dtypes
            TR.yuyv_geometry(torch.zeros((2, 4, 8, 2), dtype=dtype), layout)
    for shape in ((2, 4, 8, 3), (4, 8), (2, 2, 2, 4, 8, 2)):
        with pytest.raises(ValueError, match="frames are"):
            TR.yuyv_geometry(torch.zeros(shape, dtype=torch.uint8), "YUY2")
    with pytest.raises(ValueError, match="packed YUV 4:2:2 layout"):
        TR.yuyv_geometry(x, "VYUY")
    with pytest.raises(ValueError, match="packed YUV 4:2:2 layout"):
        TR.yuyv_to_planar(x, "I422")
    with pytest.raises(RuntimeError, match="height"):            # there is no coded height beside the shape's
        TR.yuv_geometry(x, "YUY2", height=4)


# ----------------------------------------------------------------------------- Python: the host mirrors
def test_yuyv_to_planar_of_a_hand_written_frame():
    #        macropixel 0      macropixel 1
    rows = [[10, 11, 12, 13, 14, 15, 16, 17], [20, 21, 22, 23, 24, 25, 26, 27]]
    frame = torch.tensor(rows, dtype=torch.uint8).reshape(2, 4, 2)
    want = {"YUY2": [[10, 12, 14, 16], [20, 22, 24, 26], [11, 15, 21, 25], [13, 17, 23, 27]],     # Y0 U Y1 V
            "YVYU": [[10, 12, 14, 16], [20, 22, 24, 26], [13, 17, 23, 27], [11, 15, 21, 25]],     # Y0 V Y1 U
            "UYVY": [[11, 13, 15, 17], [21, 23, 25, 27], [10, 14, 20, 24], [12, 16, 22, 26]]}     # U Y0 V Y1
    for layout, planar in want.items():
        got = TR.yuyv_to_planar(frame, layout)
        assert got.dtype == torch.uint8 and got.tolist() == planar, layout
        assert TR.yuyv_to_planar(frame[None].repeat(3, 1, 1, 1), layout).tolist() == [planar] * 3
    assert TR.yuyv_to_planar(frame, "YUYV").tolist() == want["YUY2"]
    wide = (torch.tensor(rows, dtype=torch.int32) * 1000 + 30000).to(torch.int16).reshape(2, 4, 2)   # codes above 32767 too
    for layout in ("Y210", "Y212", "Y216"):
        for view in (wide, wide.view(torch.uint16)):
            got = TR.yuyv_to_planar(view, layout)
            assert got.dtype == view.dtype and got.shape == (4, 4)
            assert got.view(torch.int16).tolist() == [[(c * 1000 + 30000 + 32768) % 65536 - 32768 for c in r] for r in want["YUY2"]]
    # an odd height: H rows of W / 2 chroma samples still make up whole tensor rows of the [2H, W] copy
    assert TR.yuyv_to_planar(torch.zeros((2, 3, 4, 2), dtype=torch.uint8), "UYVY").shape == (2, 6, 4)


@pytest.mark.parametrize("layout", TR.YUYV_LAYOUTS)
def test_yuv_to_rgb_is_yuv_to_rgb_of_the_planar_copy(layout):
    order, sb, bits, msb = YU.LAYOUT[layout]
    y, u, v = YU.planes(2, 7, 10, 40 + sb, sb, bits, msb)
    s = YU.packed_of(layout, y, u, v, seed=3)
    m = TR._yuv_matrix_of(("bt601", False), layout)              # explicit: the planar twin's string would compose another depth
    twin = "I216" if sb == 2 else "I422"
    got = TR.yuv_to_rgb(s.view, layout, m)
    assert got.shape == (2, 3, 7, 10) and got.dtype == torch.float32
    assert torch.equal(got, TR.yuv_to_rgb(TR.yuyv_to_planar(s.view, layout), twin, m))
    # and the planar copy is the planes the surface was built from
    k = 1.0 if sb == 1 else 255.0 / 65535.0                      # 16-bit codes, kept below the clamp
    pick = torch.tensor([[k, 0, 0, 0], [0, k, 0, 0], [0, 0, k, 0]], dtype=torch.float64)         # R = Y, G = U, B = V
    want = (torch.stack([y, u.repeat_interleave(2, 2), v.repeat_interleave(2, 2)], 1).double() * k).float()
    assert torch.equal(TR.yuv_to_rgb(s.view, layout, pick), want)
    if sb == 2:                                                  # read unsigned, whichever of uint16 / int16 the tensor is
        assert torch.equal(TR.yuv_to_rgb(s.view.view(torch.uint16), layout, pick), want)
    assert torch.equal(TR.yuv_to_rgb(s.view[0], layout, pick), want[0])          # one frame
    with pytest.raises(ValueError, match="4:2:0"):
        TR.yuv420_to_rgb(s.view, layout, m)


# ----------------------------------------------------------------------------- Python: the constructors
@pytest.mark.parametrize("layout", TR.YUYV_LAYOUTS + ("YUYV",))
def test_every_constructor_takes_the_new_strings(layout):
    sampler = D.UniformClipSampler(1)
    sb = YU.LAYOUT.get(layout, YU.LAYOUT["YUY2"])[1]
    name = "YUY2" if layout == "YUYV" else layout
    p = TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout)
    assert p.is_yuv and p.is_yuv4 and p.item_only and p.in_place and not p.is_packed and p.is_yuv16 == (sb == 2)
    assert p.yuv_matrix is not None and p.region_even == "width" and p.video_dims == 4
    assert TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout, interpolation="area").area
    assert TR.DevicePacker(T4._dep(), crop_size=32, src_layout=layout, regions=True).region_mode
    assert TR.DevicePacker(T4._dep(2, (36, 54), detection=True), short_side=36, src_layout=layout, keyframes=True).no_crop
    frame = _tight(name, 1, 40, 60)[0]
    assert TR.FrameList([frame] * 3, layout).geometry(layout)[:3] == (3, 40, 60)
    with pytest.raises(RuntimeError, match=r"\[H, W, 2\]"):
        TR.FrameList([frame[..., 0]] * 3, layout)
    assert INF.VideoPredictor(T4._dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.VideoBatchPredictor(T4._dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.StreamPredictor(T4._dep(), 1.0, 1.0, 4, None, None, False, 36, 32, src_layout=layout).packer.is_yuv4
    assert INF.KeyframeDetector(T4._det(), 1.0, None, None, False, 36, src_layout=layout).packer.is_yuv4
    assert INF.TubePredictor(T4._dep(), 1.0, None, None, False, 32, src_layout=layout).packer.is_yuv4
    # hdr= is a ValueError that says so
    clip = _tight(name, 2, 40, 60)[None]
    for make in (lambda: TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout, hdr="pq"),
                 lambda: INF.VideoPredictor(T4._dep(), sampler, None, None, False, 36, 32, src_layout=layout, hdr="hlg"),
                 lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout, hdr="pq")):
        with pytest.raises(ValueError, match="hdr.*does not read packed YUV 4:2:2"):
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
    # a stride that is not legal is named, and nothing is copied
    with pytest.raises(ValueError, match=r"stride\(-2\)"):
        TR.device_scale_crop(_tight(name, 2, 40, 120)[None][:, :, :, ::2], 36, 32, src_layout=layout)


def test_the_records_of_a_video_batch_carry_the_plane():
    table = torch.arange(4)[None] % 3
    for layout in TR.YUYV_LAYOUTS:
        order, sb, bits, msb = YU.LAYOUT[layout]
        s = YU.packed_of(layout, *YU.planes(3, 40, 60, 31, sb, bits, msb))
        for packer in (TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout),
                       TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout, interpolation="area")):
            batch = packer.video_batch([s.view], [table])
            rec = batch.sources[0]
            assert rec.src == s.view.data_ptr() and batch.videos[0] is s.view
            assert {k: getattr(rec, k) for k in TR._YUV_PLANE_FIELDS} == {k: s.geom[k] for k in TR._YUV_PLANE_FIELDS}
            assert (rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (3, 40, 60, 36, 54)
            assert batch.src_dtype == (L.PV_U16 if sb == 2 else L.PV_U8)
        turned = TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout).video_batch([s.view], [table], orientation=1)
        assert turned.sources[0].orient == 1 and (turned.sources[0].Hn, turned.sources[0].Wn) == (54, 36)
        frames = TR.FrameList([s.view[i] for i in (2, 0, 1)], layout)
        batch = TR.DevicePacker(T4._dep(), short_side=36, crop_size=32, src_layout=layout).video_batch([frames], [table])
        assert batch.frame_ptrs.tolist() == [f.data_ptr() for f in frames.frames] and batch.sources[0].N == 3
        with pytest.raises(RuntimeError, match="4-d"):
            packer.video_batch([s.view[0]], [table])


def test_tube_rectangles_have_an_even_left_and_w():
    boxes = torch.tensor([[3.2, 5.1, 20.7, 30.3], [7.0, 1.0, 9.0, 2.0]])
    r = TR.box_regions(boxes, 41, 60, even=TR.region_evenness("YUY2"))
    top, left, h, w = r.unbind(-1)
    assert bool((left % 2 == 0).all()) and bool((w % 2 == 0).all()) and top.tolist() == [5, 1] and h.tolist() == [26, 1]
    tubes = TR.DevicePacker(T4._dep(), crop_size=32, src_layout="UYVY", regions=True)
    video = _tight("UYVY", 4, 41, 60)
    table = torch.arange(4)[None]
    assert tubes.video_batch([video], [table], regions=[r[:1, None].expand(1, 4, 4)]).regions is not None
    with pytest.raises(ValueError, match="even left and w"):
        tubes.video_batch([video], [table], regions=[torch.tensor([[[5, 3, 26, 18]] * 4])])
