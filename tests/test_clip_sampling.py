"""The restated clip samplers (pytorchvideo_amd/data/clip_sampling.py) against sequences recorded from the reference's own
pytorchvideo/data/clip_sampling.py (tests/golden/clip_sampling.json, made by make_clip_sampling_golden.py), the frame
table that `pv_video_views` reads a video through, and everything of `pv_video_views` that is decided without a GPU:
descriptor validation, the ctypes mirror's size, and the resource usage of the shared kernel's gfx950 code."""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "clip_sampling.json")))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _dec(x):
    return Fraction(x[1], x[2]) if isinstance(x, list) and x and x[0] == "F" else x


def _case_id(c):
    return "%s%s@%s" % (c["sampler"], c["args"], c["duration"])


# ----------------------------------------------------------------------------- samplers
def test_the_fixture_covers_the_grid():
    names = {c["sampler"] for c in GOLD["cases"]}
    assert names == {"ConstantClipsPerVideoSampler", "UniformClipSampler", "UniformClipSamplerTruncateFromStart", "make_clip_sampler"}
    assert len(GOLD["cases"]) >= 200
    assert any(len(c["clips"]) == 1 for c in GOLD["cases"]) and any(len(c["clips"]) > 100 for c in GOLD["cases"])


@pytest.mark.parametrize("case", GOLD["cases"], ids=_case_id)
def test_samplers_reproduce_the_reference_sequences_exactly(case):
    args, duration = [_dec(a) for a in case["args"]], _dec(case["duration"])
    if case["sampler"] == "make_clip_sampler":
        sampler = D.make_clip_sampler(*args)
    else:
        sampler = getattr(D, case["sampler"])(*args)
    got, end = [], None
    for _ in range(len(case["clips"]) + 1):
        info = sampler(end, duration, {})
        assert isinstance(info, D.ClipInfo)
        got.append(info)
        end = info.clip_end_sec
        if info.is_last_clip:
            break
    assert len(got) == len(case["clips"])
    for g, (start, stop, index, aug, last) in zip(got, case["clips"]):
        assert Fraction(g.clip_start_sec) == Fraction(*start) and Fraction(g.clip_end_sec) == Fraction(*stop)   # exact
        assert (g.clip_index, g.aug_index, bool(g.is_last_clip)) == (index, aug, last)
    # the sampler has reset itself: a second video gives the same sequence
    again = D.sample_clips(sampler, duration)
    assert [tuple(a) for a in again] == [tuple(g) for g in got]


def test_the_docstring_example_of_the_reference():
    """clip_sampling.py:122-131: 39 frames at 30 fps, 32-frame clips, stride 16 frames; frames [0, 31], and with
    backpad_last a second clip moved back to end with the video."""
    clip, stride, dur = Fraction(32, 30), Fraction(16, 30), Fraction(39, 30)
    plain = D.sample_clips(D.UniformClipSampler(clip, stride, False), dur)
    assert [(c.clip_start_sec * 30, c.clip_end_sec * 30) for c in plain] == [(0, 32)]
    padded = D.sample_clips(D.UniformClipSampler(clip, stride, True), dur)
    assert [(c.clip_start_sec * 30, c.clip_end_sec * 30) for c in padded] == [(0, 32), (7, 39)]
    table, infos = D.clip_frame_table(D.UniformClipSampler(clip, stride, True), 39, 30, 32)
    assert table.tolist() == [list(range(0, 32)), list(range(7, 39))] and len(infos) == 2


@pytest.mark.parametrize("kind", ["random", "random_multi"])
def test_random_samplers_are_not_provided_and_say_so(kind):
    with pytest.raises(NotImplementedError, match="training-time"):
        D.make_clip_sampler(kind, 2.0)
    with pytest.raises(NotImplementedError):
        D.make_clip_sampler("nonsense", 2.0)


# ----------------------------------------------------------------------------- frame table
def test_frame_table_of_the_model_zoo_protocol():
    """300 frames at 30 fps, 10 clips of 80 frames subsampled to 16: clip k starts at k * 22/27 s = frame ceil(k * 220/9);
    the last clip is frames [220, 300)."""
    sampler = D.ConstantClipsPerVideoSampler(Fraction(80, 30), 10, 3)
    table, infos = D.clip_frame_table(sampler, 300, 30, 16)
    assert table.dtype == torch.int32 and tuple(table.shape) == (10, 16)       # the 3 augs of a clip share a row
    assert [i.clip_index for i in infos] == list(range(10)) and all(i.aug_index == 0 for i in infos)
    assert table[0, 0].item() == 0 and table[-1, -1].item() == 299
    sub = TR.temporal_indices(80, 16)
    for k in range(10):
        first = -((-k * 220) // 9)
        assert table[k].tolist() == (first + sub).tolist()
    assert table[0].tolist() == [0, 5, 10, 15, 21, 26, 31, 36, 42, 47, 52, 57, 63, 68, 73, 79]
    assert 0 <= int(table.min()) and int(table.max()) < 300


def test_frame_table_of_a_video_shorter_than_the_clip_repeats_frames():
    """5 frames at 30 fps under a 2 s clip: the clip is cut at the video's end and the subsample repeats its frames."""
    for sampler in (D.ConstantClipsPerVideoSampler(2.0, 3), D.UniformClipSampler(2.0)):
        table, infos = D.clip_frame_table(sampler, 5, 30, 8)
        want = TR.temporal_indices(5, 8).tolist()
        assert want == [0, 0, 1, 1, 2, 2, 3, 4]
        assert all(row == want for row in table.tolist())
        assert len(infos) == table.shape[0] == (3 if isinstance(sampler, D.ConstantClipsPerVideoSampler) else 1)


def test_frame_table_follows_get_clip_on_a_grid():
    """frame_video.py:149-200 by hand for every clip: range(ceil(fps * start), min(ceil(fps * min(end, duration)), N))."""
    import math
    for n, fps, t in ((300, 30, 16), (97, Fraction(30000, 1001), 8), (39, 30, 32), (1000, 25, 4), (17, 12.5, 5)):
        for sampler in (D.UniformClipSampler(Fraction(16, 15)), D.UniformClipSampler(Fraction(16, 15), Fraction(1, 3), True),
                        D.ConstantClipsPerVideoSampler(Fraction(1, 2), 7, 2), D.UniformClipSamplerTruncateFromStart(1.0, None, False, 1e-6, 2.5)):
            table, infos = D.clip_frame_table(sampler, n, fps, t)
            assert table.shape == (len(infos), t) and 0 <= int(table.min()) and int(table.max()) < n
            dur = Fraction(n) / Fraction(fps)
            for row, info in zip(table.tolist(), infos):
                a = math.ceil(Fraction(fps) * info.clip_start_sec)
                b = min(math.ceil(Fraction(fps) * min(info.clip_end_sec, dur)), n)
                assert row == (a + TR.temporal_indices(b - a, t)).tolist()


def test_a_clip_without_a_frame_is_an_error():
    class Late(D.ClipSampler):                       # a clip that starts where the video ends
        def __call__(self, last, duration, annotation):
            return D.ClipInfo(Fraction(duration), Fraction(duration) + 1, 0, 0, True)

    with pytest.raises(ValueError, match="no frame"):
        D.clip_frame_table(Late(1), 30, 30, 4)
    # 1 frame at 30 fps, two clips of 1/60 s: the second one, [1/60, 1/30), starts after the only frame
    with pytest.raises(ValueError, match="no frame"):
        D.clip_frame_table(D.UniformClipSampler(Fraction(1, 60)), 1, 30, 4)
    with pytest.raises(ValueError):
        D.clip_frame_table(D.UniformClipSampler(1), 0, 30, 4)


def test_pathway_tables_are_column_subsets_and_check_the_range():
    table, _ = D.clip_frame_table(D.ConstantClipsPerVideoSampler(Fraction(64, 30), 5), 300, 30, 32)
    slow, fast = TR.pathway_tables(table, [8, 32], 300)
    assert fast.dtype == slow.dtype == torch.int32 and torch.equal(fast, table)
    assert torch.equal(slow, table[:, TR.temporal_indices(32, 8)]) and tuple(slow.shape) == (5, 8)
    negative = table.clone()
    negative[2, 3] = -1
    for bad in (negative, table + 100, torch.zeros(0, 4, dtype=torch.int32), table.float(), table[0]):
        with pytest.raises(ValueError):
            TR.pathway_tables(bad, [8, 32], 300)
    with pytest.raises(ValueError):
        TR.pathway_tables(table, [32], 299)          # the video is one frame shorter than the table says


# ----------------------------------------------------------------------------- pv_video_views without a GPU
def _desc(keep):
    """A valid smallest descriptor: 2 clips of 1 frame from a 2-frame planar uint8 video of 2 x 2 (host memory: validation
    happens before any HIP call)."""
    src, dst, tab = (C.c_uint8 * 64)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)()
    keep.extend([src, dst, tab])
    d = L.VideoViewsDesc()
    d.src = C.addressof(src) + (-C.addressof(src)) % 16
    d.dst = C.addressof(dst) + (-C.addressof(dst)) % 16
    d.t_index = C.addressof(tab)
    d.n_clips, d.C, d.T, d.N, d.t_stride, d.Hs, d.Ws = 2, 3, 1, 2, 1, 2, 2
    d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NCTHW
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = 2, 2, 1, 1, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    return d


def _status(d):
    return L.lib().pv_video_views(C.byref(d), None)


def test_video_views_is_exported_and_versioned(pv_lib):
    assert "pv_video_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_video_views")
    assert pv_lib.pv_version() == L.ABI_VERSION >= 35


def test_video_views_rejects_invalid_descriptors_without_a_gpu(pv_lib):
    keep = []
    assert pv_lib.pv_video_views(None, None) == L.PV_ERR_INVALID
    assert _status(L.VideoViewsDesc()) == L.PV_ERR_INVALID
    for field in ("src", "dst", "t_index"):
        d = _desc(keep)
        setattr(d, field, None)
        assert _status(d) == L.PV_ERR_INVALID, field
    for field in ("n_clips", "T", "N"):
        for val in (0, -1):
            d = _desc(keep)
            setattr(d, field, val)
            assert _status(d) == L.PV_ERR_INVALID, field
    d = _desc(keep)
    d.T, d.t_stride = 2, 1                           # a row stride shorter than the row
    assert _status(d) == L.PV_ERR_INVALID
    # the checks of pv_resample_crop
    d = _desc(keep)
    d.C = 5
    assert _status(d) == L.PV_ERR_INVALID
    for nv in (0, 4, -1):
        d = _desc(keep)
        d.n_views = nv
        assert _status(d) == L.PV_ERR_INVALID
    for field, val in (("y_off", 2), ("x_off", 2), ("y_off", -1), ("x_off", -1)):
        d = _desc(keep)
        getattr(d, field)[0] = val
        assert _status(d) == L.PV_ERR_INVALID, field
    d = _desc(keep)
    d.Ho = 3
    assert _status(d) == L.PV_ERR_INVALID
    for dtype, ch in ((L.PV_F32, 3), (L.PV_U8, 4)):  # an interleaved video is uint8 with 3 channels
        d = _desc(keep)
        d.src_layout, d.src_dtype, d.C = L.SRC_NTHWC, dtype, ch
        assert _status(d) == L.PV_ERR_INVALID
    for item0, n in ((0, 3), (2, 1), (-1, 1), (1, 0)):   # 2 clips x 1 view: windows that leave the sequence
        d = _desc(keep)
        d.item0, d.n_items = item0, n
        assert _status(d) == L.PV_ERR_INVALID, (item0, n)
    d = _desc(keep)                                  # misaligned channels-last destination
    d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, 8, 8, 8
    d.dst += 2
    assert _status(d) == L.PV_ERR_INVALID
    d = _desc(keep)
    d.src_dtype = L.PV_BF16
    assert _status(d) == L.PV_ERR_UNSUPPORTED


def test_ctypes_mirror_has_the_size_of_the_c_struct(tmp_path):
    """sizeof(pv_video_views_desc) as the C compiler sees it (a static assertion against the header)."""
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    src.write_text('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_video_views_desc) == %d, "size");\n'
                   '_Static_assert(sizeof(pv_resample_desc) == %d, "size");\n'
                   % (C.sizeof(L.VideoViewsDesc), C.sizeof(L.ResampleDesc)))
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src.write_text('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_video_views_desc) == %d, "size");\n' % (C.sizeof(L.VideoViewsDesc) + 8))
    assert subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True).returncode != 0          # the assertion does fire


@pytest.fixture(scope="module")
def resample_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("isa_rs") / "pv_resample.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_resample.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_every_resample_instantiation_is_free_of_scratch_and_spills(resample_asm):
    """The per-clip table index and the clip stride ride in RsLaunch; the by-value descriptors are still selected, never
    indexed: 3 source forms x 5 destination forms, all with no private segment, no spilled register and at most 72 VGPRs."""
    kernels = re.findall(r"\.name:\s+(\S*resample_crop_kernel\S*)\n(.*?)\.wavefront_size", resample_asm, re.S)
    assert len(kernels) == 15, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
        assert meta["vgpr_count"] <= 72, (name, meta["vgpr_count"])     # 512 / 72: seven waves per SIMD, as before the table
    assert "pv_video_views" in open(os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_resample.hip")).read()
