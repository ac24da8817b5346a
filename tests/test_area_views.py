"""The box-filtered downscale (`pv_area_views`, include/pv_mi355x.h "box-filtered downscale"), without a GPU: the pinned integer
windows against `F.interpolate(mode="area")` in float64, the entry point -- exported, mirrored by ctypes, validated before any
launch --, the code-object metadata of its kernels, and the refusals of `device_scale_crop`, `DevicePacker` and the predictors
with `interpolation="area"`."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import area_util as AU
import test_batch_views as TB
import test_frame_views as TF
import test_region_views as TRV
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED
W = TB.W


# ----------------------------------------------------------------------------- the windows
@pytest.mark.parametrize("name", list(AU.GEOMETRIES))
def test_the_windows_are_those_of_interpolate_area(name):
    """The header's integer windows, as the float64 reference builds on them, against torch's own adaptive average pooling on
    the whole scaled frame, and the same values through the host mirror `short_side_scale(x, size, "area")`."""
    hs, ws, short, _ = AU.GEOMETRIES[name]
    hn, wn = TR.scaled_size(hs, ws, short)
    x = torch.randint(0, 256, (3, 2, hs, ws), generator=torch.Generator().manual_seed(hs * ws)).double()
    got, n = AU.reference(x, hn, wn, 0, 0, hn, wn)
    want = torch.nn.functional.interpolate(x, size=(hn, wn), mode="area")
    worst = (got - want).abs().max().item()
    print("%s: %d x %d -> %d x %d, largest window %d taps, worst difference %.3e" % (name, hs, ws, hn, wn, n, worst))
    assert worst <= 1e-12
    assert torch.equal(TR.short_side_scale(x.float(), short, "area"), torch.nn.functional.interpolate(x.float(), size=(hn, wn), mode="area"))
    # a window of a view is the same window of the whole frame
    part, _ = AU.reference(x, hn, wn, 1, 2, hn - 1, wn - 2)
    assert torch.equal(part, got[..., 1:, 2:])
    sy, ey = AU.windows(hs, hn, 0, hn)
    assert int(sy[0]) == 0 and int(ey[-1]) == hs and bool((ey[:-1] >= sy[1:]).all())          # no source row is skipped
    if name == "64x96_to_16":
        assert bool((ey - sy == 4).all()) and bool((ey[:-1] == sy[1:]).all())                  # integer ratio: no overlap
    if name == "135x240_to_16":
        assert n >= 90 and bool((ey[:-1] > sy[1:]).any())                                      # neighbours overlap by one row
    if name in ("20x30_to_32", "33x57_to_33"):
        assert int((ey - sy).max()) == (2 if name == "20x30_to_32" else 1)


# ----------------------------------------------------------------------------- the entry point
def test_area_views_is_exported_and_mirrored(pv_lib, tmp_path):
    assert "pv_area_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_area_views")
    assert pv_lib.pv_version() == L.ABI_VERSION                  # additive: no existing descriptor changed
    assert L.PV_FILTER_AREA == 1
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "int pv_area_views(const pv_area_views_desc* d, pv_stream_t stream);" in header
    assert C.sizeof(L.AreaViewsDesc) == C.sizeof(L.FrameViewsDesc) + 16
    assert L.AreaViewsDesc.filter.offset == C.sizeof(L.FrameViewsDesc) and L.AreaViewsDesc.reserved.offset == C.sizeof(L.FrameViewsDesc) + 4
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16                # what they were
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    text = ('#include <stddef.h>\n#include "pv_mi355x.h"\n'
            '_Static_assert(sizeof(pv_area_views_desc) == sizeof(pv_frame_views_desc) + 16, "size");\n'
            '_Static_assert(sizeof(pv_area_views_desc) == %d, "size");\n_Static_assert(sizeof(pv_frame_views_desc) == %d, "size");\n'
            '_Static_assert(offsetof(pv_area_views_desc, filter) == %d, "offset");\n_Static_assert(PV_FILTER_AREA == 1, "value");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    sizes = [C.sizeof(L.AreaViewsDesc), C.sizeof(L.FrameViewsDesc), L.AreaViewsDesc.filter.offset]
    src.write_text(text % tuple(sizes))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i in range(3):                                           # the assertions do fire
        off = list(sizes)
        off[i] += 8
        src.write_text(text % tuple(off))
        assert subprocess.run(cmd, capture_output=True).returncode != 0, i


def _area_desc(keep, frames, yuv=False):
    """The base descriptors of tests/test_batch_views.py / tests/test_frame_views.py -- two sources, 2 x W and 6 x W scaled to
    3 x W with W = 40000, a table of 3 rows of one frame, 4 items writing 1 x W, one view -- wrapped.  It passes EVERY check of
    PV_ERR_INVALID, and Ws * Wn = 1.6e9 is beyond the index limit of 2^24, which is checked behind all of them: it returns
    PV_ERR_UNSUPPORTED -- the positive control of every PV_ERR_INVALID case below -- and nothing here is ever launched, on a
    machine with a GPU or without."""
    if frames:
        f, sources, items, ptrs = TF._desc(keep, yuv)
    else:
        d, sources, items = TB._desc(keep, yuv)
        f, ptrs = L.FrameViewsDesc(), None
        C.memmove(C.byref(f.batch), C.byref(d), C.sizeof(d))
    a = L.AreaViewsDesc()
    C.memmove(C.byref(a.frames), C.byref(f), C.sizeof(f))
    a.filter = L.PV_FILTER_AREA
    return a, sources, items, ptrs


def _status(a):
    return L.lib().pv_area_views(C.byref(a), None)


FORMS, FORM_IDS = TRV.FORMS, TRV.FORM_IDS


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_area_views_is_validated_before_any_launch(pv_lib, frames, yuv):
    keep = []
    assert pv_lib.pv_area_views(None, None) == INV
    assert _status(L.AreaViewsDesc()) == INV
    a, _, _, _ = _area_desc(keep, frames, yuv)
    assert _status(a) == UNS                                     # the positive control: only the index limit is left
    # this entry point's own fields
    for flt in (0, 2, -1):
        a, _, _, _ = _area_desc(keep, frames, yuv)
        a.filter = flt
        assert _status(a) == INV, flt
    for k in range(3):
        a, _, _, _ = _area_desc(keep, frames, yuv)
        a.reserved[k] = 1
        assert _status(a) == INV, k
    # a pointer table only half given, or a length without a table
    full, _, _, _ = _area_desc(keep, True, yuv)
    for field in ("frame_ptrs", "frame_ptrs_dev"):
        a, _, _, _ = _area_desc(keep, frames, yuv)
        a.frames.frame_ptrs, a.frames.frame_ptrs_dev, a.frames.n_frame_ptrs = full.frames.frame_ptrs, full.frames.frame_ptrs_dev, 6
        setattr(a.frames, field, None)
        assert _status(a) == INV, field
    if not frames:
        a, _, _, _ = _area_desc(keep, False, yuv)
        a.frames.n_frame_ptrs = 6
        assert _status(a) == INV
    else:
        for n in (0, -1, 4):                                     # the wrapped entry point's table checks (4: a slice leaves it)
            a, _, _, _ = _area_desc(keep, True, yuv)
            a.frames.n_frame_ptrs = n
            assert _status(a) == INV, n
        a, _, _, ptrs = _area_desc(keep, True, yuv)
        ptrs[3] = 0                                              # a null frame inside a slice an item names
        assert _status(a) == INV
    # what the wrapped entry point rejects: the launch fields, the items, the records
    for field in ("sources", "sources_dev", "items", "items_dev", "t_index", "dst") + (("yuv2rgb",) if yuv else ()):
        a, _, _, _ = _area_desc(keep, frames, yuv)
        setattr(a.frames.batch, field, None)
        assert _status(a) == INV, field
    for field in ("n_sources", "n_items", "n_rows", "T", "Ho", "Wo", "C", "n_views"):
        a, _, _, _ = _area_desc(keep, frames, yuv)
        setattr(a.frames.batch, field, 0)
        assert _status(a) == INV, field
    a, _, _, _ = _area_desc(keep, frames, yuv)
    a.frames.batch.n_views = 4
    assert _status(a) == INV
    a, _, _, _ = _area_desc(keep, frames, yuv)
    a.frames.batch.t_stride = 0
    assert _status(a) == INV
    for field, bad in (("source", 2), ("source", -1), ("row", 3), ("row", -1), ("view", 1), ("view", -1)):
        a, _, items, _ = _area_desc(keep, frames, yuv)
        setattr(items[3], field, bad)
        assert _status(a) == INV, (field, bad)
    for index in (0, 1):
        for field in ("src", "N", "Hs", "Ws", "Hn", "Wn"):
            a, sources, _, _ = _area_desc(keep, frames, yuv)
            setattr(sources[index], field, None if field == "src" else 0)
            assert _status(a) == INV, (index, field)
        for orient in (8, -1):
            a, sources, _, _ = _area_desc(keep, frames, yuv)
            sources[index].orient = orient
            assert _status(a) == INV, (index, orient)
        # a window that leaves the scaled frame; sy / sx are validated as there (one ulp off is refused), though not used
        a, sources, _, _ = _area_desc(keep, frames, yuv)
        sources[index].x_off[0] = 1
        assert _status(a) == INV, index
        a, sources, _, _ = _area_desc(keep, frames, yuv)
        sources[index].y_off[0] = sources[index].Hn
        assert _status(a) == INV, index
        for field in ("sy", "sx"):
            a, sources, _, _ = _area_desc(keep, frames, yuv)
            bits = C.c_uint32.from_buffer_copy(C.c_float(getattr(sources[index], field))).value
            setattr(sources[index], field, C.c_float.from_buffer_copy(C.c_uint32(bits + 1)).value)
            assert _status(a) == INV, (index, field)
        if yuv:
            for field in ("frame_stride", "c_pitch"):
                a, sources, _, _ = _area_desc(keep, frames, yuv)
                setattr(sources[index], field, 1)
                assert _status(a) == INV, (index, field)
    # the dtype / layout matrix of the wrapped entry point
    a, _, _, _ = _area_desc(keep, frames, yuv)
    a.frames.batch.dst_dtype = L.PV_U8
    assert _status(a) == UNS
    a, _, _, _ = _area_desc(keep, frames, yuv)
    a.frames.batch.src_dtype = L.PV_BF16
    assert _status(a) == UNS
    if not yuv:
        a, _, _, _ = _area_desc(keep, frames, yuv)
        a.frames.batch.src_dtype = L.PV_U16                      # 16-bit samples are a YUV 4:2:0 source only
        assert _status(a) == UNS


@pytest.mark.parametrize("frames,yuv", FORMS, ids=FORM_IDS)
def test_oriented_records_and_the_index_limit_are_unsupported(pv_lib, frames, yuv):
    """A record with orient != 0 named by an item is PV_ERR_UNSUPPORTED -- the code is read (a code outside 0..7 is invalid,
    above), an invalid field still wins, and a record no item names may be oriented or anything else.  The index limit: either
    axis beyond 2^24 alone is refused.  (Both limits are PV_ERR_UNSUPPORTED and nothing may be launched here, so what a launch
    inside the limit does is left to the GPU suite.)"""
    keep = []
    for orient in (2, 4, 6):                                     # codes that keep the displayed size: sy / sx stay valid
        a, sources, _, _ = _area_desc(keep, frames, yuv)
        sources[1].orient = orient
        assert _status(a) == UNS, orient
    a, sources, items, _ = _area_desc(keep, frames, yuv)
    sources[1].orient = 2
    items[0].row = 7
    assert _status(a) == INV
    a, sources, items, _ = _area_desc(keep, frames, yuv)          # items on source 0 only: record 1 is not read
    for it in items:
        it.source, it.row = 0, 0
    sources[1].orient, sources[1].Hn = 3, -5
    assert _status(a) == UNS
    # either axis alone beyond the limit, on source 0 alone (the items moved to it)
    for hs, ws in ((2, W), (4098, 2)):                            # W * W columns with 2 * 2 rows; 4098 * 4098 rows with 2 * W columns
        a, sources, items, _ = _area_desc(keep, frames, yuv)
        for it in items:
            it.source, it.row = 0, 0
        rec = sources[0]
        rec.Hs, rec.Hn, rec.Ws, rec.Wn = hs, hs, ws, W
        rec.sy, rec.sx = 1.0, C.c_float(ws / W).value
        if yuv:
            rec.y_pitch = rec.c_pitch = ws
            rec.u_offset, rec.v_offset, rec.frame_stride = hs * ws, hs * ws + 1, hs * ws * 3 // 2
        assert max(hs * hs, ws * W) > 1 << 24 and min(hs * hs, ws * W) <= 1 << 24
        assert _status(a) == UNS, (hs, ws)
        rec.sx = C.c_float(ws / W * 2).value                     # and an invalid field of that record still wins
        assert _status(a) == INV, (hs, ws)


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_area(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_area") / "pv_area.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_area.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_area_kernel_is_free_of_scratch_and_spills(asm_area):
    """3 RGB / planar source forms and 2 chroma arrangements x 2 sample widths, x 5 destination forms: no private segment and
    no spilled register.  The register counts are printed (profiles/r23/resource_usage.md records them); they are not gated."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_area, re.S)
    names = [k for k, _ in kernels]
    assert len([n for n in names if "area_views_kernel" in n]) == 15 and len([n for n in names if "area_yuv_kernel" in n]) == 20
    assert len(kernels) == 35, names
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


# ----------------------------------------------------------------------------- Python refusals, before any launch
def _dep(batch=4, size=(32, 32), detection=False):
    return TRV._fake_deployed(batch, size, detection=detection)


def test_every_new_argument_defaults_to_bilinear():
    for fn in (TR.device_scale_crop, TR.DevicePacker.__init__, INF.VideoPredictor.__init__, INF.VideoBatchPredictor.__init__,
               INF.KeyframeDetector.__init__, INF.StreamPredictor.__init__):
        assert inspect.signature(fn).parameters["interpolation"].default == "bilinear", fn
    assert "interpolation" not in inspect.signature(INF.TubePredictor.__init__).parameters
    assert "interpolation" not in inspect.signature(TR.device_resized_crop).parameters
    assert TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC").area is False
    assert TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC", interpolation="area").area is True


def test_device_scale_crop_refuses_before_any_launch():
    clip = torch.zeros((2, 3, 4, 40, 60), dtype=torch.uint8)
    for mode in ("bicubic", "nearest", "AREA", None):
        with pytest.raises(ValueError, match="'bilinear' or 'area'"):
            TR.device_scale_crop(clip, 36, 32, interpolation=mode)
    for orientation in (1, 4, 7):
        with pytest.raises(ValueError, match="orientation"):
            TR.device_scale_crop(clip, 36, 32, interpolation="area", orientation=orientation)
    p010 = torch.zeros((2, 4, 60, 60), dtype=torch.int16)
    with pytest.raises(ValueError, match="hdr"):
        TR.device_scale_crop(p010, 36, 32, interpolation="area", src_layout="P010", hdr="pq")
    with pytest.raises(ValueError, match="src_layout"):
        TR.device_scale_crop(clip, 36, 32, interpolation="area", src_layout="RGB")
    with pytest.raises(ValueError, match="dtype"):
        TR.device_scale_crop(clip, 36, 32, interpolation="area", dtype=torch.float16)


def test_the_packer_refuses_what_area_does_not_carry():
    video, table = torch.zeros((6, 40, 60, 3), dtype=torch.uint8), torch.arange(4)[None]
    for mode in ("bicubic", "nearest", ""):
        with pytest.raises(ValueError, match="'bilinear' or 'area'"):
            TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC", interpolation=mode)
    with pytest.raises(ValueError, match="regions"):
        TR.DevicePacker(_dep(), crop_size=32, src_layout="NTHWC", regions=True, interpolation="area")
    with pytest.raises(ValueError, match="hdr"):
        TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="P010", hdr="pq", interpolation="area")
    with pytest.raises(ValueError, match="short_side"):
        TR.DevicePacker(_dep(), interpolation="area")
    packer = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC", interpolation="area")
    batch = packer.video_batch([video], [table])                 # whole videos: the records of the bilinear packer
    plain = TR.DevicePacker(_dep(), short_side=36, crop_size=32, src_layout="NTHWC").video_batch([video], [table])
    assert batch.total == plain.total == 1 and bytes(batch.sources) == bytes(plain.sources)
    for orientation in (1, [4], [6]):
        with pytest.raises(ValueError, match="orientation"):
            packer.video_batch([video], [table], orientation=orientation)
    assert packer.video_batch([video], [table], orientation=[0]).total == 1
    with pytest.raises(ValueError, match="video_batch.*device_scale_crop"):
        packer(torch.zeros((4, 3, 4, 40, 60), dtype=torch.uint8))
    with pytest.raises(ValueError, match="video_batch"):
        packer.fill_video(video, [table.int()], 0, 1)
    # key frames, and their no-crop mode, are taken
    det = TR.DevicePacker(_dep(2, (36, 54), detection=True), short_side=36, src_layout="NTHWC", keyframes=True, interpolation="area")
    assert det.area and det.no_crop and det.video_batch([video], [table]).total == 1


def test_the_predictors_pass_the_argument_to_the_packer():
    from pytorchvideo_amd import data as D
    sampler = D.UniformClipSampler(1)
    for mode, area in (("bilinear", False), ("area", True)):
        assert INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, interpolation=mode).packer.area is area
        assert INF.VideoBatchPredictor(_dep(), sampler, None, None, False, 36, 32, interpolation=mode).packer.area is area
        assert INF.StreamPredictor(_dep(), 1.0, 1.0, 4, None, None, False, 36, 32, interpolation=mode).packer.area is area
        det = INF.KeyframeDetector(_det(), 1.0, None, None, False, 36, interpolation=mode)
        assert det.packer.area is area and det.packer.no_crop
    for make in (lambda: INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, interpolation="cubic"),
                 lambda: INF.VideoBatchPredictor(_dep(), sampler, None, None, False, 36, 32, interpolation="cubic"),
                 lambda: INF.KeyframeDetector(_det(), 1.0, None, None, False, 36, interpolation="cubic"),
                 lambda: INF.StreamPredictor(_dep(), 1.0, 1.0, 4, None, None, False, 36, 32, interpolation="cubic")):
        with pytest.raises(ValueError, match="'bilinear' or 'area'"):
            make()
    with pytest.raises(ValueError, match="hdr"):
        INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout="P010", hdr="hlg", interpolation="area")
    with pytest.raises(ValueError, match="orientation"):
        INF.StreamPredictor(_dep(), 1.0, 1.0, 4, None, None, False, 36, 32, orientation=1, interpolation="area")
    # a turned video is refused by the one-video walk of VideoPredictor before anything is uploaded
    pred = INF.VideoPredictor(_dep(), sampler, None, None, False, 36, 32, src_layout="NTHWC", interpolation="area")
    with pytest.raises(ValueError, match="orientation"):
        pred(torch.zeros((8, 40, 60, 3), dtype=torch.uint8), 4, orientation=1)


def _det():
    dep = _dep(2, (36, 54), detection=True)
    dep._pv_box_capacity, dep._pv_box_ptr = 5, None
    return dep
