"""Packed pixels (include/pv_mi355x.h "packed pixels": PV_SRC_BGR, PV_SRC_RGBA, PV_SRC_BGRA, PV_SRC_ARGB, PV_SRC_ABGR), without a
GPU: the layouts in the C ABI of `pv_batch_views`, `pv_frame_views`, `pv_region_views` and `pv_area_views` -- validated before
any launch, in the positive-control style of tests/test_area_views.py: nothing is launched, a valid descriptor is
PV_ERR_UNSUPPORTED for an LDS or index-limit reason, which shows that validation was passed --, the code-object metadata of
the kernels of pv_packed.hip, and the Python side: the strings, the stride rules, the records and the host mirror."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import packed_util as PU
import test_area_views as TA
import test_batch_views as TB
import test_clip_sampling as TCS
import test_frame_views as TF
import test_hdr_ingest as TH
import test_region_views as TRV
import test_transforms_spatial as TTS
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
W = TB.W
CODES = {"BGR": 4, "RGBA": 5, "BGRA": 6, "ARGB": 7, "ABGR": 8}

# (entry point, frame list?)
ENTRIES = [("batch", False), ("frames", True), ("region", False), ("region", True), ("area", False), ("area", True)]
ENTRY_IDS = ["%s-%s" % (e, "frames" if f else "videos") for e, f in ENTRIES]


def _packed_desc(keep, entry, frames, layout="BGRA"):
    """The base descriptor of the entry point's own test file (two sources of 2 x W and 6 x W, W = 40000, beyond the LDS limit
    of a staged strip and the index limit of the box filter) as a packed launch: the layout, and per record a dense row pitch
    and frame stride.  Returns (status(), batch descriptor, records, pointer table or None)."""
    if entry == "batch":
        outer, sources, _ = TB._desc(keep)
        d, ptrs, fn = outer, None, "pv_batch_views"
    elif entry == "frames":
        outer, sources, _, ptrs = TF._desc(keep)
        d, fn = outer.batch, "pv_frame_views"
    elif entry == "region":
        outer, sources, _, _, ptrs = TRV._region_desc(keep, frames)
        d, fn = outer.frames.batch, "pv_region_views"
    else:
        outer, sources, _, ptrs = TA._area_desc(keep, frames)
        d, fn = outer.frames.batch, "pv_area_views"
    pb = PU.layout_bytes(layout)
    d.src_layout = CODES[layout]
    for rec, (hs, ws) in zip(sources, ((2, W), (6, W))):
        rec.y_pitch, rec.frame_stride = ws * pb, hs * ws * pb
    return (lambda: getattr(L.lib(), fn)(C.byref(outer), None)), d, sources, ptrs


# ----------------------------------------------------------------------------- the ABI
def test_the_layout_values_are_the_headers(pv_lib):
    assert (L.SRC_BGR, L.SRC_RGBA, L.SRC_BGRA, L.SRC_ARGB, L.SRC_ABGR) == (4, 5, 6, 7, 8)
    assert pv_lib.pv_version() == L.ABI_VERSION == 36
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "enum { PV_SRC_BGR = 4, PV_SRC_RGBA = 5, PV_SRC_BGRA = 6, PV_SRC_ARGB = 7, PV_SRC_ABGR = 8 };" in header
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16     # no struct gained or lost a byte
    assert TR.PACKED_LAYOUTS == tuple(CODES) and all(getattr(L, "SRC_" + k) == v for k, v in CODES.items())


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_packed_descriptors_are_validated_before_any_launch(pv_lib, entry, frames):
    keep = []
    for layout in CODES:                                         # the positive control: every layout passes validation
        status, _, _, _ = _packed_desc(keep, entry, frames, layout)
        assert status() == UNS, layout
    status, d, _, _ = _packed_desc(keep, entry, frames)
    d.src_layout = 3                                             # no layout
    assert status() == INV
    status, d, _, _ = _packed_desc(keep, entry, frames)
    d.src_layout = 9
    assert status() == INV
    for index in (0, 1):
        hs, ws = ((2, W), (6, W))[index]
        for layout in ("BGRA", "BGR"):
            pb = PU.layout_bytes(layout)
            status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
            sources[index].y_pitch = ws * pb - pb                # a pitch that does not hold a row
            assert status() == INV, (index, layout)
            status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
            sources[index].frame_stride = (hs - 1) * ws * pb + ws * pb - pb      # a stride that does not hold a frame
            assert status() == INV, (index, layout)
            status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
            sources[index].frame_stride = (hs - 1) * ws * pb + ws * pb           # exactly the frame: legal
            assert status() == UNS, (index, layout)
            for field in ("u_offset", "v_offset", "c_pitch"):
                status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
                setattr(sources[index], field, 4)
                assert status() == INV, (index, layout, field)
    status, d, _, _ = _packed_desc(keep, entry, frames)
    d.src_dtype = L.PV_F32
    assert status() == INV
    status, d, _, _ = _packed_desc(keep, entry, frames)
    d.C = 4
    assert status() == INV
    # an invalid field wins over the unsupported size
    status, d, sources, _ = _packed_desc(keep, entry, frames)
    sources[1].N = 0
    assert status() == INV


@pytest.mark.parametrize("entry,frames", ENTRIES, ids=ENTRY_IDS)
def test_a_four_byte_pixel_is_an_aligned_dword_and_a_three_byte_pixel_lies_anywhere(pv_lib, entry, frames):
    keep = []
    for layout in ("RGBA", "BGRA", "ARGB", "ABGR"):
        for index in (0, 1):
            for off in (1, 2, 3):
                status, _, sources, ptrs = _packed_desc(keep, entry, frames, layout)
                if frames:
                    ptrs[3 if index else 0] += off               # a frame of a slice an item names (source 0: 0..1, source 1: 2..4)
                else:
                    sources[index].src += off
                assert status() == INV, (layout, index, off)
            for off in (1, 2, 3):
                status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
                sources[index].y_pitch += off
                sources[index].frame_stride += 4 * 8             # room for the longer rows
                assert status() == INV, (layout, index, off)
                status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
                sources[index].frame_stride += off
                assert status() == INV, (layout, index, off)
        status, _, sources, _ = _packed_desc(keep, entry, frames, layout)
        for rec in sources:                                      # multiples of 4 beyond the dense ones: a pitched surface
            rec.y_pitch += 12
            rec.frame_stride += 12 * 6 + 20
        assert status() == UNS, layout
    for off in (1, 2, 3):                                        # BGR: odd bases, odd pitches, odd strides
        status, _, sources, ptrs = _packed_desc(keep, entry, frames, "BGR")
        for i in range(6 if frames else 0):
            ptrs[i] += off
        for rec in sources:
            if not frames:
                rec.src += off
            rec.y_pitch += off + 4
            rec.frame_stride += (off + 4) * 6 + off
        assert status() == UNS, off


def test_the_other_entry_points_refuse_the_packed_layouts(pv_lib):
    keep = []
    for code in CODES.values():
        for frames in (False, True):                             # pv_hdr_views: 16-bit YUV only
            h, _, _ = TH._hdr_desc(keep, frames)
            h.frames.batch.src_layout, h.frames.batch.src_dtype = code, L.PV_U8
            assert TH._status(h) in (INV, UNS) and TH._status(h) != L.PV_OK, code
            h, _, _ = TH._hdr_desc(keep, frames)
            h.frames.batch.src_layout = code                     # with the 16-bit samples it does take
            assert TH._status(h) in (INV, UNS), code
        d = TTS._desc(keep)                                      # pv_resample_crop
        d.src_layout, d.src_dtype, d.C = code, L.PV_U8, 3
        assert TTS._status(d) == INV, code
        d = TCS._desc(keep)                                      # pv_video_views
        d.src_layout, d.src_dtype, d.C = code, L.PV_U8, 3
        assert TCS._status(d) == INV, code


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_packed(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_packed") / "pv_packed.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_packed.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_packed_kernel_is_free_of_scratch_and_spills(asm_packed):
    """4 bodies x 2 pixel sizes x 5 destination forms -- the channel order is a kernel argument, not a kernel --: no private
    segment and no spilled register.  The register counts are printed (profiles/r26/resource_usage.md records them)."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_packed, re.S)
    names = [k for k, _ in kernels]
    for body in ("packed_views_kernel", "packed_orient_kernel", "packed_region_kernel", "packed_area_kernel"):
        for pb in (3, 4):
            assert len([n for n in names if "%sILi%dE" % (body, pb) in n]) == 5, (body, pb)
    assert len(kernels) == 40, names
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


def test_a_four_byte_tap_is_one_dword_lds_read(asm_packed):
    """PB == 4 reads a tap as one dword from LDS and takes the channels out of the register; PB == 3 keeps byte reads."""
    for m in re.finditer(r"^(_Z\w*packed_\w+_kernelILi(\d)E\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm_packed, re.S | re.M):
        name, pb, body = m.group(1), int(m.group(2)), m.group(3)
        dwords, bytes_ = len(re.findall(r"\bds_read2?_b32\b", body)), len(re.findall(r"\bds_read_u8", body))
        if pb == 4:
            assert dwords > 0 and bytes_ == 0, (name, dwords, bytes_)
        else:
            assert bytes_ > 0, (name, dwords, bytes_)


# ----------------------------------------------------------------------------- Python: the strings
def _dep(batch=4, size=(32, 32), detection=False):
    return TRV._fake_deployed(batch, size, detection=detection)


def _det():
    dep = _dep(2, (36, 54), detection=True)
    dep._pv_box_capacity, dep._pv_box_ptr = 5, None
    return dep


STRINGS = list(TR.PACKED_LAYOUTS) + ["RGBX", "BGRX", "XRGB", "XBGR"]


@pytest.mark.parametrize("layout", STRINGS)
def test_every_constructor_takes_the_packed_strings(layout):
    sampler = D.UniformClipSampler(1)
    pb = TR._packed_bytes(layout)
    assert pb == (3 if layout == "BGR" else 4)
    p = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout)
    assert p.is_packed and p.in_place and not p.is_yuv
    assert TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, interpolation="area").area
    assert TR.DevicePacker(_dep(), crop_size=32, src_layout=layout, regions=True).region_mode
    assert TR.DevicePacker(_dep(2, (36, 54), detection=True), short_side=36, src_layout=layout, keyframes=True).no_crop
    assert TR.FrameList([torch.zeros((40, 60, pb), dtype=torch.uint8)] * 3, layout).geometry(layout)[:3] == (3, 40, 60)
    assert INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_packed
    assert INF.VideoBatchPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout).packer.is_packed
    assert INF.StreamPredictor(_dep(), 1.0, 1.0, 4, None, None, False, 36, 32, src_layout=layout).packer.is_packed
    assert INF.KeyframeDetector(_det(), 1.0, None, None, False, 36, src_layout=layout).packer.is_packed
    assert INF.TubePredictor(_dep(), 1.0, None, None, False, 32, src_layout=layout).packer.is_packed
    assert TR._src_codes(layout, torch.uint8) == (CODES[TR._packed_name(layout)], L.PV_U8)
    # hdr= stays the ValueError it is for every layout without 16-bit samples
    with pytest.raises(ValueError, match="hdr"):
        TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, hdr="pq")
    with pytest.raises(ValueError, match="hdr"):
        INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout=layout, hdr="hlg")
    with pytest.raises(ValueError, match="hdr"):
        TR.device_scale_crop(torch.zeros((1, 2, 40, 60, pb), dtype=torch.uint8), 36, 32, src_layout=layout, hdr="pq")
    # the functions take the string: what stops them on a machine without a GPU is the device, never the layout
    clip = torch.zeros((1, 2, 40, 60, pb), dtype=torch.uint8)
    for call in (lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout),
                 lambda: TR.device_scale_crop(clip, 36, 32, src_layout=layout, interpolation="area"),
                 lambda: TR.device_resized_crop(clip, torch.tensor([[[0, 0, 20, 20]] * 2]), 32, src_layout=layout)):
        try:
            call()
        except ValueError as e:                                  # pragma: no cover - the failure this test is for
            pytest.fail("%s refused: %s" % (layout, e))
        except (RuntimeError, AssertionError):
            assert not torch.cuda.is_available()


def test_rgb_is_still_no_layout():
    for make in (lambda: TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="RGB"),
                 lambda: TR.device_scale_crop(torch.zeros((1, 2, 40, 60, 3), dtype=torch.uint8), 36, 32, src_layout="RGB"),
                 lambda: TR.device_resized_crop(torch.zeros((1, 2, 40, 60, 3), dtype=torch.uint8), torch.zeros((1, 2, 4)), 32, src_layout="RGB"),
                 lambda: TR.FrameList([torch.zeros((40, 60, 3), dtype=torch.uint8)], "RGB")):
        with pytest.raises(ValueError, match="src_layout"):
            make()
    with pytest.raises(ValueError, match="packed layout"):
        TR.packed_to_rgb(torch.zeros((2, 2, 3), dtype=torch.uint8), "RGB")


# ----------------------------------------------------------------------------- Python: the stride rules and the records
def _bad_views(pb):
    """(what the message names, a [N,H,W,PB] tensor that breaks one stride rule)."""
    wide = torch.zeros((3, 40, 60, 2 * pb), dtype=torch.uint8)
    yield "stride\\(-1\\)", torch.zeros((3 * 40 * 60 * pb * 2,), dtype=torch.uint8).as_strided((3, 40, 60, pb), (40 * 60 * pb * 2, 60 * pb * 2, pb * 2, 2))
    yield "stride\\(-2\\)", wide[..., :pb]                       # every other pixel of a wider surface
    yield "stride\\(-2\\)", torch.zeros((3, 40, 120, pb), dtype=torch.uint8)[:, :, ::2]
    yield "row stride", torch.zeros((3 * 40 * 60 * pb,), dtype=torch.uint8).as_strided((3, 40, 60, pb), (40 * 60 * pb, 30 * pb, pb, 1))
    yield "frame stride", torch.zeros((3 * 40 * 60 * pb,), dtype=torch.uint8).as_strided((3, 40, 60, pb), (20 * 60 * pb, 60 * pb, pb, 1))


@pytest.mark.parametrize("layout", ["BGR", "BGRA", "ARGB"])
def test_the_stride_rules_raise_and_name_the_stride(layout):
    pb = PU.layout_bytes(layout)
    packer = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout)
    table = torch.arange(4)[None] % 3
    for what, video in _bad_views(pb):
        assert video.shape == (3, 40, 60, pb)
        with pytest.raises(ValueError, match=what):
            TR.packed_geometry(video, layout)
        with pytest.raises(ValueError, match=what):
            packer.video_batch([video], [table])
        with pytest.raises(ValueError, match=what):
            TR.device_scale_crop(video[None], 36, 32, src_layout=layout)
        with pytest.raises(ValueError, match=what):
            TR.device_resized_crop(video[None], torch.tensor([[[0, 0, 20, 20]] * 3]), 32, src_layout=layout)
        if "frame" not in what:
            with pytest.raises(ValueError, match=what):
                TR.FrameList(list(video.unbind(0)), layout)
    with pytest.raises(ValueError, match="uint8"):
        TR.packed_geometry(torch.zeros((3, 40, 60, pb), dtype=torch.float32), layout)
    with pytest.raises(ValueError, match="uint8"):
        TR.packed_geometry(torch.zeros((3, 40, 60, pb + 1), dtype=torch.uint8), layout)
    if pb == 4:                                                  # a pixel is one aligned dword
        buf = torch.zeros((3 * 40 * 64 * 4 + 16,), dtype=torch.uint8)
        for start, pitch in ((2, 64 * 4), (0, 64 * 4 - 2)):
            video = buf.as_strided((3, 40, 60, 4), (40 * 64 * 4, pitch, 4, 1), start + (-buf.data_ptr()) % 4)
            with pytest.raises(ValueError, match="multiples of 4"):
                packer.video_batch([video], [table])
    else:                                                        # BGR lies anywhere
        buf = torch.zeros((3 * 40 * 187 + 16,), dtype=torch.uint8)
        video = buf.as_strided((3, 40, 60, 3), (40 * 187, 187, 3, 1), 5)
        assert packer.video_batch([video], [table]).sources[0].y_pitch == 187


@pytest.mark.parametrize("layout", ["BGRA", "BGR"])
def test_the_records_of_a_pitched_sliced_view_carry_its_strides(layout):
    """A column slice of a wider, pitched surface: never copied -- the record points at the slice's first pixel and carries the
    surface's row and frame strides as y_pitch / frame_stride."""
    pb = PU.layout_bytes(layout)
    surface = torch.zeros((6, 44, 80, pb), dtype=torch.uint8)
    video = surface[:, 2:42, 8:68]                               # 40 x 60 of 44 x 80
    assert not video.is_contiguous()
    table = torch.arange(4)[None]
    for packer in (TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout),
                   TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout, interpolation="area")):
        batch = packer.video_batch([video], [table])
        rec = batch.sources[0]
        assert rec.src == video.data_ptr() == surface.data_ptr() + (2 * 80 + 8) * pb
        assert (rec.y_pitch, rec.frame_stride, rec.u_offset, rec.v_offset, rec.c_pitch) == (80 * pb, 44 * 80 * pb, 0, 0, 0)
        assert (rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (6, 40, 60, 36, 54) and batch.videos[0] is video
        assert batch.src_dtype == L.PV_U8
    # frame lists: every frame where it lies, the extent of one frame as frame_stride
    frames = TR.FrameList([surface[i, 2:42, 8:68] for i in (3, 0, 5)], layout)
    batch = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout=layout).video_batch([frames], [table % 3])
    rec = batch.sources[0]
    assert (rec.y_pitch, rec.frame_stride, rec.N) == (80 * pb, 39 * 80 * pb + 60 * pb, 3)
    assert batch.frame_ptrs.tolist() == [f.data_ptr() for f in frames.frames]
    # regions
    tubes = TR.DevicePacker(_dep(), crop_size=32, src_layout=layout, regions=True)
    batch = tubes.video_batch([video], [table], regions=[torch.tensor([[[1, 3, 21, 33]] * 4])])
    assert (batch.sources[0].y_pitch, batch.sources[0].frame_stride) == (80 * pb, 44 * 80 * pb) and batch.regions is not None
    # the dense forms keep the zeros they had
    dense = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC").video_batch([torch.zeros((6, 40, 60, 3), dtype=torch.uint8)], [table])
    assert (dense.sources[0].y_pitch, dense.sources[0].frame_stride) == (0, 0)


# ----------------------------------------------------------------------------- Python: the host mirror
def test_packed_to_rgb_is_the_hand_written_permutation():
    by_hand = {"BGR": lambda x: torch.stack([x[..., 2], x[..., 1], x[..., 0]], -1),
               "RGBA": lambda x: torch.stack([x[..., 0], x[..., 1], x[..., 2]], -1),
               "BGRA": lambda x: torch.stack([x[..., 2], x[..., 1], x[..., 0]], -1),
               "ARGB": lambda x: torch.stack([x[..., 1], x[..., 2], x[..., 3]], -1),
               "ABGR": lambda x: torch.stack([x[..., 3], x[..., 2], x[..., 1]], -1)}
    assert set(by_hand) == set(TR.PACKED_LAYOUTS)
    for layout, hand in by_hand.items():
        pb = PU.layout_bytes(layout)
        _, view = PU.surface(layout, 3, 7, 9, 40 + pb)
        got = TR.packed_to_rgb(view, layout)
        assert got.shape == (3, 7, 9, 3) and got.dtype == torch.uint8 and torch.equal(got, hand(view))
        # the round trip: R, G, B written at the layout's bytes come back
        rgb = torch.randint(0, 256, (2, 5, 6, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(pb))
        px = torch.full((2, 5, 6, pb), 77, dtype=torch.uint8)
        for c, at in enumerate(TR._PACKED_RGB[layout]):
            px[..., at] = rgb[..., c]
        assert torch.equal(TR.packed_to_rgb(px, layout), rgb)
        with pytest.raises(ValueError, match="bytes"):
            TR.packed_to_rgb(torch.zeros((2, 2, pb + 1), dtype=torch.uint8), layout)
    for alias, name in (("RGBX", "RGBA"), ("BGRX", "BGRA"), ("XRGB", "ARGB"), ("XBGR", "ABGR")):
        x = torch.randint(0, 256, (4, 4, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
        assert torch.equal(TR.packed_to_rgb(x, alias), TR.packed_to_rgb(x, name))
