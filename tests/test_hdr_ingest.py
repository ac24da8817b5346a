"""PQ / HLG sources of the ingest (`pv_hdr_views`, include/pv_mi355x.h "HDR sources"), without a GPU: the entry point --
exported, versioned, validated before any launch --, `transforms.tone_params` and the host mirror `transforms.hdr_to_sdr`
against the independent restatement of tests/hdr_util.py and the anchors of the standards, the `hdr=` argument of the Python
entry points, and the code-object metadata of the kernels of pv_hdr.hip."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

import hdr_util as HU
import test_yuv16_ingest as T16
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- export, versioning
def test_hdr_views_is_exported_and_versioned(pv_lib, tmp_path):
    assert "pv_hdr_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_hdr_views")
    assert (L.TRANSFER_PQ, L.TRANSFER_HLG) == (1, 2)
    assert pv_lib.pv_version() == L.ABI_VERSION == 36            # additive: no descriptor changed
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "int pv_hdr_views(const pv_hdr_views_desc* d, pv_stream_t stream);" in header
    assert C.sizeof(L.HdrViewsDesc) == C.sizeof(L.FrameViewsDesc) + 16
    assert C.sizeof(L.YuvViewsDesc) == 184 and C.sizeof(L.ViewSource) == 96          # what they were
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    text = ('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_hdr_views_desc) == sizeof(pv_frame_views_desc) + 16, "size");\n'
            '_Static_assert(sizeof(pv_hdr_views_desc) == %d, "size");\n'
            '_Static_assert(PV_TRANSFER_PQ == 1 && PV_TRANSFER_HLG == 2, "value");\n'
            '_Static_assert(sizeof(pv_yuv_views_desc) == 184, "size");\n_Static_assert(sizeof(pv_view_source) == 96, "size");\n'
            '_Static_assert(sizeof(pv_frame_views_desc) == %d, "size");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    src.write_text(text % (C.sizeof(L.HdrViewsDesc), C.sizeof(L.FrameViewsDesc)))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src.write_text(text % (C.sizeof(L.HdrViewsDesc) + 8, C.sizeof(L.FrameViewsDesc)))
    assert subprocess.run(cmd, capture_output=True).returncode != 0          # the assertion does fire


# ----------------------------------------------------------------------------- rejection table
def _hdr_desc(keep, frames):
    """The smallest descriptor that passes EVERY check but the last (tests/test_yuv16_ingest.py `_batch_desc`: two P010 sources
    of 20000 columns, beyond the LDS limit of a staged strip), wrapped: a host `tone`, PQ.  Without `frames` the table fields
    are null and the records are whole videos."""
    f, sources, ptrs = T16._batch_desc(keep, frames)
    tone = (C.c_float * 16)()
    keep.append(tone)
    h = L.HdrViewsDesc()
    C.memmove(C.byref(h.frames), C.byref(f), C.sizeof(f))
    if not frames:
        h.frames.frame_ptrs = h.frames.frame_ptrs_dev = None
        h.frames.n_frame_ptrs = 0
    h.tone, h.transfer = C.addressof(tone), L.TRANSFER_PQ
    return h, sources, ptrs


def _status(h):
    return L.lib().pv_hdr_views(C.byref(h), None)


@pytest.mark.parametrize("frames", [False, True], ids=["whole_videos", "frame_list"])
def test_hdr_views_is_validated_before_any_launch(pv_lib, frames):
    keep = []
    assert pv_lib.pv_hdr_views(None, None) == INV
    assert _status(L.HdrViewsDesc()) == INV
    # the positive control: the valid base stops at the last check only, for either transfer
    for transfer in (L.TRANSFER_PQ, L.TRANSFER_HLG):
        h, _, _ = _hdr_desc(keep, frames)
        h.transfer = transfer
        assert _status(h) == UNS
    # this entry point's own fields
    h, _, _ = _hdr_desc(keep, frames)
    h.tone = None
    assert _status(h) == INV
    for transfer in (0, 3, -1, 256 + 1):
        h, _, _ = _hdr_desc(keep, frames)
        h.transfer = transfer
        assert _status(h) == INV, transfer
    h, _, _ = _hdr_desc(keep, frames)
    h.reserved = 1
    assert _status(h) == INV
    # a pointer table only half given
    full, _, ptrs = _hdr_desc(keep, True)
    for field in ("frame_ptrs", "frame_ptrs_dev"):
        h, _, _ = _hdr_desc(keep, frames)
        h.frames.frame_ptrs, h.frames.frame_ptrs_dev, h.frames.n_frame_ptrs = full.frames.frame_ptrs, full.frames.frame_ptrs_dev, 6
        setattr(h.frames, field, None)
        assert _status(h) == INV, field
    if not frames:
        h, _, _ = _hdr_desc(keep, False)
        h.frames.n_frame_ptrs = 6                                # a length without a table
        assert _status(h) == INV
    else:
        for n in (0, -1, 4):                                     # the wrapped entry point's table checks (4: a slice leaves it)
            h, _, _ = _hdr_desc(keep, True)
            h.frames.n_frame_ptrs = n
            assert _status(h) == INV, n
    # only 16-bit YUV 4:2:0: every other pair is unsupported, the pairs the wrapped entry points take included
    for layout, dtype in ((L.SRC_YUV420, L.PV_U8), (L.SRC_NCTHW, L.PV_U8), (L.SRC_NCTHW, L.PV_F32), (L.SRC_NTHWC, L.PV_U8),
                          (L.SRC_NCTHW, L.PV_U16), (L.SRC_YUV420, L.PV_F32), (L.SRC_YUV420, L.PV_BF16)):
        h, _, _ = _hdr_desc(keep, frames)
        h.frames.batch.src_layout, h.frames.batch.src_dtype = layout, dtype
        assert _status(h) == UNS, (layout, dtype)
    # own fields are checked before the pair: an invalid transfer on an unsupported pair is invalid
    h, _, _ = _hdr_desc(keep, frames)
    h.frames.batch.src_dtype, h.transfer = L.PV_U8, 0
    assert _status(h) == INV
    # what the wrapped entry point rejects
    for field in ("sources", "sources_dev", "items", "items_dev", "t_index", "dst", "yuv2rgb"):
        h, _, _ = _hdr_desc(keep, frames)
        setattr(h.frames.batch, field, None)
        assert _status(h) == INV, field
    for field in ("n_sources", "n_items", "n_rows", "T", "Ho", "Wo", "C", "c_step", "n_views"):
        h, _, _ = _hdr_desc(keep, frames)
        setattr(h.frames.batch, field, 0)
        assert _status(h) == INV, field
    for index in (0, 1):
        for field, delta in (("frame_stride", 1), ("v_offset", 1), ("y_pitch", 1), ("c_pitch", 1)):
            h, sources, _ = _hdr_desc(keep, frames)
            setattr(sources[index], field, getattr(sources[index], field) + delta)
            assert _status(h) == INV, (index, field)
        for orient in (8, -1):
            h, sources, _ = _hdr_desc(keep, frames)
            sources[index].orient = orient
            assert _status(h) == INV, (index, orient)
        h, sources, _ = _hdr_desc(keep, frames)
        sources[index].sy = sources[index].sy * 1.5              # not the library's own division
        assert _status(h) == INV
    h, sources, ptrs = _hdr_desc(keep, frames)
    if frames:
        ptrs[1] += 1                                             # an odd frame address in a slice an item names
    else:
        sources[1].src += 1
    assert _status(h) == INV
    h, _, _ = _hdr_desc(keep, frames)
    h.frames.batch.dst_dtype = L.PV_U8
    assert _status(h) == UNS


def test_an_oriented_record_is_sized_as_a_tile(pv_lib):
    """The base with its second record turned a quarter: the record's views must then lie in the displayed frame (W x 6), so
    the unchanged windows are invalid -- the orientation is read, not ignored."""
    keep = []
    h, sources, _ = _hdr_desc(keep, False)
    sources[1].orient = 1
    assert _status(h) == INV


# ----------------------------------------------------------------------------- tone_params
def test_tone_params_against_the_restatement_and_its_errors():
    for transfer in ("pq", "hlg"):
        got = TR.tone_params(transfer)
        assert got.dtype == torch.float32 and tuple(got.shape) == (16,)
        assert torch.equal(got, torch.tensor(HU.tone(transfer), dtype=torch.float64).float())
        other = TR.tone_params(transfer, peak_nits=4000.0, white_nits=100.0, knee=0.5, gamut=None)
        want = HU.tone(transfer, 4000.0, 100.0, 0.5, gamut=HU.IDENTITY)
        assert torch.equal(other, torch.tensor(want, dtype=torch.float64).float())
        clip = TR.tone_params(transfer, tone_map="clip")
        assert torch.equal(clip, torch.tensor(HU.tone(transfer, curve=False), dtype=torch.float64).float())
        assert float(clip[2]) > 1e38 and math.isfinite(float(clip[2]))
        assert float(got[15]) == 0.0
    # the defaults reproduce the BT.2087 matrix
    assert torch.equal(TR.tone_params("pq")[6:15].reshape(3, 3), torch.tensor(HU.BT2087, dtype=torch.float64).float())
    assert abs(float(TR.tone_params("pq")[0]) - 10000.0 / 203.0) < 1e-5 and float(TR.tone_params("pq")[1]) == 0.0
    assert abs(float(TR.tone_params("hlg")[1]) - 0.2) < 1e-7 and abs(float(TR.tone_params("hlg")[0]) - 1000.0 / 203.0) < 1e-6
    for bad in (dict(transfer="srgb"), dict(transfer="pq", tone_map="reinhard"), dict(transfer="pq", gamut="p3"),
                dict(transfer="hlg", peak_nits=203.0), dict(transfer="hlg", peak_nits=100.0), dict(transfer="pq", knee=0.0),
                dict(transfer="pq", knee=1.0), dict(transfer="pq", knee=-0.1)):
        with pytest.raises(ValueError):
            TR.tone_params(**bad)


def test_the_anchors_of_the_standards():
    f64 = torch.float64
    assert float(HU.pq_eotf(0.0)) == 0.0 and abs(float(HU.pq_eotf(1.0)) - 10000.0) < 1e-8
    nits = torch.tensor([0.005, 0.1, 1.0, 100.0, 203.0, 1000.0, 4000.0, 10000.0], dtype=f64)
    assert torch.allclose(HU.pq_eotf(HU.pq_inverse_eotf(nits)), nits, rtol=1e-11, atol=0)
    assert abs(float(HU.pq_inverse_eotf(100.0)) - 0.508078421517399) < 1e-9          # ST 2084: 100 nits is code 0.5081
    assert abs(float(HU.hlg_inverse_oetf(0.5)) - 1.0 / 12.0) < 1e-15 and abs(float(HU.hlg_inverse_oetf(1.0)) - 1.0) < 1e-7
    # the two branches of HLG meet at 1/2 to the precision of the published constants
    assert abs(float((torch.exp((torch.tensor(0.5, dtype=f64) - HU.C) / HU.A) + HU.B) / 12.0) - 1.0 / 12.0) < 1e-9
    # mobius: out(j) = j, slope 1 at j, out(P) = 1, the identity below the knee
    j, p = 0.3, 1000.0 / 203.0
    assert abs(float(HU.mobius(j + 1e-12, j, p)) - j) < 1e-11 and abs(float(HU.mobius(p, j, p)) - 1.0) < 1e-12
    h = 1e-6
    assert abs(float(HU.mobius(j + 2 * h, j, p) - HU.mobius(j + h, j, p)) / h - 1.0) < 1e-5
    below = torch.linspace(0.0, j, 50, dtype=f64)
    assert torch.equal(HU.mobius(below, j, p), below)
    # the tone table's s, a', b' are that curve as the kernel evaluates it: k = s (m + a') / ((m + b') m)
    t = HU.tone("pq")
    m = torch.linspace(j + 1e-3, p, 200, dtype=f64)
    assert torch.allclose(t[3] * (m + t[4]) / ((m + t[5]) * m) * m, HU.mobius(m, j, p), rtol=1e-13, atol=0)
    # the OETF is continuous at the switch (0.018 / 1.099 would jump by 0.066 of a code)
    lo, hi = 4.5 * HU.BETA, HU.ALPHA * HU.BETA ** 0.45 - (HU.ALPHA - 1.0)
    assert abs(lo - hi) < 1e-12
    assert abs(255.0 * (4.5 * 0.018 - (1.099 * 0.018 ** 0.45 - 0.099))) > 0.05


# ----------------------------------------------------------------------------- hdr_to_sdr
def _ramp(n=1024):
    g = torch.linspace(0.0, 255.0, n, dtype=torch.float64)
    return g.view(1, 1, n).expand(3, 1, n).clone()


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_hdr_to_sdr_against_the_restatement(transfer):
    g = torch.Generator().manual_seed(1900 + len(transfer))
    x = torch.rand((2, 3, 3, 40, 50), generator=g, dtype=torch.float64) * 255.0
    x[0, :, :, :4] = 0.0
    x[1, :, :, :4] = 255.0
    for kw in (dict(), dict(peak_nits=4000.0, knee=0.6), dict(tone_map="clip"), dict(gamut=None)):
        tone = TR.tone_params(transfer, **kw)
        got = TR.hdr_to_sdr(x, transfer, tone)
        want = HU.to_sdr(x, transfer, tone)
        assert got.dtype == torch.float64 and got.shape == x.shape
        assert torch.isfinite(got).all() and float(got.min()) >= 0.0 and float(got.max()) <= 255.0
        assert float((got - want).abs().max()) < 1e-9, kw
        assert torch.equal(got, TR.hdr_to_sdr(x, L.TRANSFER_PQ if transfer == "pq" else L.TRANSFER_HLG, tone))
    with pytest.raises(ValueError):
        TR.hdr_to_sdr(x, "gamma", TR.tone_params(transfer))
    with pytest.raises(ValueError):
        TR.hdr_to_sdr(x, transfer, torch.zeros(12))
    with pytest.raises(ValueError):
        TR.hdr_to_sdr(torch.zeros(4, 5, 6), transfer, TR.tone_params(transfer))         # no channel dimension of 3


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_a_grey_ramp_is_monotone_from_black_to_white(transfer):
    """0 -> 0, the signal of peak_nits -> 255 (a grey keeps its hue through the gamut matrix up to the rounding of BT.2087's
    four decimals: its rows sum to 1.0001, 1.0000 and 0.9999), monotone in between and constant above the peak."""
    tone = TR.tone_params(transfer)
    out = TR.hdr_to_sdr(_ramp(), transfer, tone)
    assert torch.equal(out[:, 0, 0], torch.zeros(3, dtype=torch.float64))
    assert bool((out[:, 0, 1:] >= out[:, 0, :-1] - 1e-9).all())
    peak = 255.0 * (float(HU.pq_inverse_eotf(1000.0)) if transfer == "pq" else 1.0)
    at_peak = TR.hdr_to_sdr(torch.full((3, 1, 1), peak, dtype=torch.float64), transfer, tone)
    assert float((at_peak - 255.0).abs().max()) < 0.02, at_peak.flatten().tolist()
    assert float(out[:, 0, -1].min()) > 254.98
    # mid-greys land ten codes and more off when the curve is ignored (HLG, which was built to degrade gently: 15; PQ: 60)
    mid = _ramp()[:, :, 300:700]
    assert float((TR.hdr_to_sdr(mid, transfer, tone) - mid).abs().max()) > 10.0


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_clip_is_the_curve_with_its_branch_disabled(transfer):
    g = torch.Generator().manual_seed(1910)
    x = torch.rand((3, 30, 30), generator=g, dtype=torch.float64) * 255.0
    mobius, clip = TR.tone_params(transfer), TR.tone_params(transfer, tone_map="clip")
    never = mobius.clone()
    never[2] = 3e38                                              # the same s, a', b': only the branch differs
    assert torch.equal(TR.hdr_to_sdr(x, transfer, clip), TR.hdr_to_sdr(x, transfer, never))
    # below the knee the curve is the identity: dark taps are the same under both tables
    dark = x * (0.25 if transfer == "pq" else 0.3)
    assert torch.equal(TR.hdr_to_sdr(dark, transfer, clip), TR.hdr_to_sdr(dark, transfer, mobius))
    assert not torch.equal(TR.hdr_to_sdr(x, transfer, clip), TR.hdr_to_sdr(x, transfer, mobius))


def test_the_fp32_mirror_takes_the_other_branch_only_at_the_switch():
    """The restatement in float32 (the floor the device is measured against) is finite on the whole code range and agrees
    with float64 to a fraction of a code."""
    for transfer in ("pq", "hlg"):
        tone = TR.tone_params(transfer)
        x = _ramp(4096)
        lo = HU.to_sdr(x, transfer, tone, torch.float32)
        assert lo.dtype == torch.float32 and torch.isfinite(lo).all()
        assert float((lo.double() - HU.to_sdr(x, transfer, tone)).abs().max()) < 0.01


# ----------------------------------------------------------------------------- the hdr= argument
def test_hdr_argument_forms_and_refusals():
    code, tone = TR._hdr_of("pq", "P010")
    assert code == L.TRANSFER_PQ and torch.equal(tone, TR.tone_params("pq"))
    custom = TR.tone_params("hlg", peak_nits=600.0)
    code, tone = TR._hdr_of(("hlg", custom), "I010")
    assert code == L.TRANSFER_HLG and torch.equal(tone, custom) and tone.dtype == torch.float32
    assert TR._hdr_of(None, "NV12") is None and TR._hdr_of(None, "P010") is None
    for layout in ("NV12", "I420", "NCTHW", "NTHWC"):
        with pytest.raises(ValueError, match="10- to 16-bit"):
            TR._hdr_of("pq", layout)
    for bad in ("sdr", ("pq",), ("pq", [0.0] * 16), ("pq", torch.zeros(15)), 1):
        with pytest.raises(ValueError):
            TR._hdr_of(bad, "P010")
    # no path ignores hdr: an 8-bit or RGB source is refused before anything touches a device
    clip = torch.zeros((1, 2, 6, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="10- to 16-bit"):
        TR.device_scale_crop(clip, 4, 4, src_layout="NV12", hdr="pq")
    with pytest.raises(ValueError, match="10- to 16-bit"):
        TR.device_scale_crop(torch.zeros((1, 3, 2, 4, 4), dtype=torch.uint8), 4, 4, hdr="hlg")
    with pytest.raises(ValueError, match="10- to 16-bit"):
        TR.DevicePacker(object(), short_side=4, crop_size=4, src_layout="NV12", hdr="pq")
    import inspect
    from pytorchvideo_amd import inference as INF
    for fn in (TR.device_scale_crop, TR.DevicePacker.__init__, INF.VideoPredictor.__init__, INF.VideoBatchPredictor.__init__,
               INF.KeyframeDetector.__init__, INF.StreamPredictor.__init__):
        assert inspect.signature(fn).parameters["hdr"].default is None, fn


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm_hdr(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path_factory.mktemp("isa_hdr") / "pv_hdr.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_hdr.hip")], stderr=subprocess.DEVNULL)
    return open(path).read()


def test_every_hdr_kernel_is_free_of_scratch_and_spills(asm_hdr):
    """2 transfers x 2 chroma forms x 5 destination forms of the strip and of the tile kernel: no private segment and no
    spilled register, the G = 8 planar forms included; the count is the one DESIGN.md 4.11 states.  The register counts are
    printed (DESIGN.md records them); they are not gated."""
    kernels = re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", asm_hdr, re.S)
    names = [k for k, _ in kernels]
    assert len([n for n in names if "hdr_strip_kernel" in n]) == 20 and len([n for n in names if "hdr_tile_kernel" in n]) == 20
    assert len(kernels) == 40, names
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.11"):]
    assert re.search(r"\b40 kernels\b", section[:section.index("\n## ") if "\n## " in section else len(section)])
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
