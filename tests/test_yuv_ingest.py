"""Decoder-native YUV 4:2:0 sources of the ingest, without a GPU: the conversion matrix (`transforms.yuv_matrix`), the host
mirror of the tap rule (`transforms.yuv420_to_rgb`), the descriptor of `pv_yuv_views` (include/pv_mi355x.h) -- exported,
versioned, mirrored by ctypes, validated before any launch -- and the code-object metadata of its kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import yuv_util as YU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KR_KB = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
LAYOUTS = ("NV12", "NV21", "I420", "YV12")


# ----------------------------------------------------------------------------- matrix
def _apply(m, yuv):
    return m[:, :3] @ torch.tensor(yuv, dtype=torch.float64) + m[:, 3]


@pytest.mark.parametrize("standard", ["bt709", "bt601"])
def test_matrix_maps_the_grey_axis_onto_0_255(standard):
    lim = TR.yuv_matrix(standard, False)
    assert lim.dtype == torch.float64 and tuple(lim.shape) == (3, 4)
    assert torch.allclose(_apply(lim, (16, 128, 128)), torch.zeros(3, dtype=torch.float64), atol=1e-9)
    assert torch.allclose(_apply(lim, (235, 128, 128)), torch.full((3,), 255.0, dtype=torch.float64), atol=1e-9)
    full = TR.yuv_matrix(standard, True)
    for v in (0, 1, 77, 128, 255):
        assert torch.allclose(_apply(full, (v, 128, 128)), torch.full((3,), float(v), dtype=torch.float64), atol=1e-9)


def test_matrix_agrees_with_the_textbook_bt601_coefficients():
    m = TR.yuv_matrix("bt601", False)
    want = torch.tensor([[1.164, 0.0, 1.596], [1.164, -0.392, -0.813], [1.164, 2.017, 0.0]], dtype=torch.float64)
    assert (m[:, :3] - want).abs().max().item() <= 1e-3
    assert TR.yuv_matrix() .equal(TR.yuv_matrix("bt709", False))
    with pytest.raises(ValueError):
        TR.yuv_matrix("bt2020")


def _forward(standard, full_range):
    """RGB in [0, 255] -> unrounded 8-bit (Y, U, V), built here from (Kr, Kb) and the ranges: [3, 4]."""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    y_lo, y_span, c_span = (0.0, 255.0, 255.0) if full_range else (16.0, 219.0, 224.0)
    luma = torch.tensor([kr, kg, kb], dtype=torch.float64)
    pb = (torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64) - luma) / (2.0 * (1.0 - kb))
    pr = (torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64) - luma) / (2.0 * (1.0 - kr))
    a = torch.stack([luma * y_span, pb * c_span, pr * c_span]) / 255.0
    return torch.cat([a, torch.tensor([[y_lo], [128.0], [128.0]], dtype=torch.float64)], dim=1)


@pytest.mark.parametrize("standard", ["bt709", "bt601"])
@pytest.mark.parametrize("full_range", [False, True])
def test_matrix_round_trip(standard, full_range):
    rgb = torch.rand(3, 500, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * 255.0
    f = _forward(standard, full_range)
    yuv = f[:, :3] @ rgb + f[:, 3:]
    m = TR.yuv_matrix(standard, full_range)
    back = m[:, :3] @ yuv + m[:, 3:]
    assert (back - rgb).abs().max().item() <= 1e-9


# ----------------------------------------------------------------------------- mirror
M709 = TR.yuv_matrix("bt709", False)


def test_mirror_gives_the_same_rgb_for_every_packing_pitch_and_coded_height():
    y, u, v = YU.planes(3, 10, 12, 21)
    want = YU.rgb_of_planes(y, u, v, M709).float()
    for layout in LAYOUTS:
        plain = TR.yuv420_to_rgb(YU.pack(y, u, v, layout).frames(), layout, M709)
        assert plain.dtype == torch.float32 and tuple(plain.shape) == (3, 3, 10, 12)
        assert torch.equal(plain, want), layout
        coded = TR.yuv420_to_rgb(YU.pack(y, u, v, layout, coded_height=16, garbage=5).frames(), layout, M709,
                                 coded_height=16, height=10)
        assert torch.equal(coded, want), layout
        pitched = YU.pack(y, u, v, layout, pitch=18, base=3, garbage=6).frames()
        assert pitched.stride() == (15 * 18, 18, 1) and not pitched.is_contiguous()
        assert torch.equal(TR.yuv420_to_rgb(pitched, layout, M709), want), layout
        both = YU.pack(y, u, v, layout, coded_height=12, pitch=14, base=1, garbage=7).frames()
        assert torch.equal(TR.yuv420_to_rgb(both, layout, M709, height=10), want), layout
    clips = YU.pack(y, u, v, "NV12").frames()[:2].reshape(2, 1, 15, 12)          # [B, T, Hc*3/2, W]
    assert torch.equal(TR.yuv420_to_rgb(clips, "NV12", M709), want[:2].reshape(2, 1, 3, 10, 12))


def test_mirror_replicates_chroma_over_2x2_blocks():
    y = torch.full((1, 6, 8), 120, dtype=torch.uint8)
    u = torch.full((1, 3, 4), 128, dtype=torch.uint8)
    v = torch.full((1, 3, 4), 128, dtype=torch.uint8)
    u[0, 1, 2], v[0, 1, 2] = 90, 200                       # one distinct chroma sample: luma rows 2..3, columns 4..5
    for layout in LAYOUTS:
        rgb = TR.yuv420_to_rgb(YU.pack(y, u, v, layout).frames(), layout, M709)[0]
        grey = rgb[:, 0, 0]
        different = (rgb != grey.view(3, 1, 1)).any(dim=0)
        want = torch.zeros(6, 8, dtype=torch.bool)
        want[2:4, 4:6] = True
        assert torch.equal(different, want), layout
        block = rgb[:, 2:4, 4:6]
        assert torch.equal(block, block[:, :1, :1].expand(3, 2, 2)), layout


def test_mirror_clamps_out_of_gamut_input():
    corners = [(255, 255, 255), (0, 0, 0), (255, 0, 255), (0, 255, 0), (255, 255, 0), (0, 0, 255)]
    y = torch.tensor([c[0] for c in corners], dtype=torch.uint8).repeat_interleave(2).view(1, 1, 12).repeat(1, 2, 1)
    u = torch.tensor([c[1] for c in corners], dtype=torch.uint8).view(1, 1, 6)
    v = torch.tensor([c[2] for c in corners], dtype=torch.uint8).view(1, 1, 6)
    m = TR.yuv_matrix("bt601", False)
    rgb = TR.yuv420_to_rgb(YU.pack(y, u, v, "I420").frames(), "I420", m)
    assert rgb.min().item() == 0.0 and rgb.max().item() == 255.0
    raw = torch.stack([m[:, :3] @ torch.tensor(c, dtype=torch.float64) + m[:, 3] for c in corners])     # [6, 3]
    assert raw.min().item() < -100 and raw.max().item() > 400                                            # far outside
    assert torch.equal(rgb[0, :, 0, ::2], torch.clamp(raw, 0, 255).float().t())


def test_geometry_reads_pitch_and_offsets_off_the_strides_and_refuses_what_it_cannot_describe():
    y, u, v = YU.planes(2, 10, 12, 22)
    g = TR.yuv_geometry(YU.pack(y, u, v, "NV21", coded_height=16, pitch=20, base=5).frames(), "NV21", coded_height=16, height=10)
    assert g == dict(N=2, Hs=10, Ws=12, Hc=16, frame_stride=24 * 20, y_pitch=20, c_pitch=20, c_step=2,
                     u_offset=16 * 20 + 1, v_offset=16 * 20)
    g = TR.yuv_geometry(YU.pack(y, u, v, "YV12", pitch=16).frames(), "YV12")
    assert (g["c_step"], g["c_pitch"], g["v_offset"], g["u_offset"]) == (1, 8, 10 * 16, 10 * 16 + 5 * 8)
    frames = YU.pack(y, u, v, "NV12").frames()
    for bad, kw in ((frames.float(), {}), (frames[:, :14], {}), (frames[..., :11], {}), (frames, dict(coded_height=12)),
                    (frames, dict(height=9)), (frames, dict(height=12)), (frames.transpose(1, 2), {}), (frames[0, 0], {})):
        with pytest.raises(RuntimeError):
            TR.yuv_geometry(bad, "NV12", **kw)
    with pytest.raises(RuntimeError, match="even"):
        TR.yuv_geometry(YU.pack(y, u, v, "NV12", pitch=13).frames(), "I420")     # planar chroma: half of an odd pitch
    with pytest.raises(ValueError):
        TR.yuv_geometry(frames, "NTHWC")


# ----------------------------------------------------------------------------- descriptor
def _desc(keep):
    """A valid smallest descriptor: 2 clips of 1 frame from two NV12 frames of 2 x 2 (host memory: validation happens
    before any HIP call)."""
    src, dst, tab, mat = (C.c_uint8 * 64)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)(), (C.c_float * 12)()
    keep.extend([src, dst, tab, mat])
    d = L.YuvViewsDesc()
    d.src = C.addressof(src) + 1
    d.dst = C.addressof(dst) + (-C.addressof(dst)) % 16
    d.t_index, d.yuv2rgb = C.addressof(tab), C.addressof(mat)
    d.n_clips, d.T, d.N, d.t_stride, d.Hs, d.Ws = 2, 1, 2, 1, 2, 2
    d.frame_stride, d.y_pitch, d.c_pitch, d.c_step, d.u_offset, d.v_offset = 6, 2, 2, 2, 4, 5
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = 2, 2, 1, 1, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    return d


def _status(d):
    return L.lib().pv_yuv_views(C.byref(d), None)


def test_yuv_views_is_exported_and_versioned(pv_lib):
    assert "pv_yuv_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_yuv_views")
    assert pv_lib.pv_version() == L.ABI_VERSION == 36


def _with(keep, **fields):
    d = _desc(keep)
    for k, val in fields.items():
        setattr(d, k, val)
    return d


def test_yuv_views_rejects_invalid_descriptors_without_a_gpu(pv_lib):
    keep = []
    inv = L.PV_ERR_INVALID
    assert pv_lib.pv_yuv_views(None, None) == inv
    assert _status(L.YuvViewsDesc()) == inv
    for field in ("src", "dst", "t_index", "yuv2rgb"):
        assert _status(_with(keep, **{field: None})) == inv, field
    for field in ("n_clips", "T", "N", "Hs", "Ws"):
        for val in (0, -2):
            assert _status(_with(keep, **{field: val})) == inv, field
    assert _status(_with(keep, T=2, t_stride=1)) == inv                       # a row stride shorter than the row
    # odd frame sizes (everything else large enough for them)
    assert _status(_with(keep, Hs=3, Hn=3, frame_stride=64, u_offset=8, v_offset=9)) == inv
    assert _status(_with(keep, Ws=3, Wn=3, y_pitch=4, c_pitch=4, frame_stride=64, u_offset=8, v_offset=9)) == inv
    for step in (0, 3, 4, -1):
        assert _status(_with(keep, c_step=step)) == inv, step
    assert _status(_with(keep, y_pitch=1)) == inv                             # y_pitch < Ws
    assert _status(_with(keep, c_pitch=1)) == inv                             # c_pitch < (Ws/2) * c_step
    assert _status(_with(keep, c_step=1, c_pitch=0, u_offset=4, v_offset=5)) == inv
    # planes that leave the frame
    assert _status(_with(keep, frame_stride=3)) == inv                        # luma: 2 rows of pitch 2 need 4 bytes
    assert _status(_with(keep, frame_stride=5)) == inv                        # the V sample at byte 5
    assert _status(_with(keep, frame_stride=0)) == inv
    assert _status(_with(keep, frame_stride=-6)) == inv
    assert _status(_with(keep, u_offset=-1, v_offset=0)) == inv
    assert _status(_with(keep, u_offset=5, v_offset=6)) == inv
    assert _status(_with(keep, c_step=1, c_pitch=1, u_offset=4, v_offset=6)) == inv     # planar V behind the frame
    assert _status(_with(keep, u_offset=1 << 40, v_offset=(1 << 40) + 1)) == inv
    # an interleaved plane holds U and V side by side
    assert _status(_with(keep, frame_stride=8, u_offset=4, v_offset=6)) == inv
    assert _status(_with(keep, u_offset=4, v_offset=4)) == inv
    # the checks of pv_resample_crop
    for nv in (0, 4, -1):
        assert _status(_with(keep, n_views=nv)) == inv
    for field, val in (("y_off", 2), ("x_off", 2), ("y_off", -1), ("x_off", -1)):
        d = _desc(keep)
        getattr(d, field)[0] = val
        assert _status(d) == inv, field
    assert _status(_with(keep, Ho=3)) == inv
    for item0, n in ((0, 3), (2, 1), (-1, 1), (1, 0)):       # 2 clips x 1 view: windows that leave the sequence
        assert _status(_with(keep, item0=item0, n_items=n)) == inv, (item0, n)
    d = _with(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=8)                # misaligned channels-last destination
    d.dst += 2
    assert _status(d) == inv
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=4)) == inv       # items overlap
    d = _desc(keep)
    d.dst += 1                                                                # a bf16 destination at an odd address
    assert _status(d) == inv
    # outside the destination matrix
    uns = L.PV_ERR_UNSUPPORTED
    assert _status(_with(keep, dst_dtype=L.PV_U8)) == uns
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, dst_dtype=L.PV_F32, c_p=4, ld=4, bs=4)) == uns
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, c_p=6, ld=8, bs=8)) == uns
    assert _status(_with(keep, dst_layout=7)) == uns


def test_ctypes_mirror_of_the_yuv_descriptor_has_the_size_of_the_c_struct(tmp_path):
    """sizeof(pv_yuv_views_desc) as the C compiler sees it; pv_resample_desc and pv_video_views_desc have kept theirs."""
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    text = '#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_yuv_views_desc) == %d, "size");\n'
    src.write_text(text % C.sizeof(L.YuvViewsDesc)
                   + '_Static_assert(sizeof(pv_video_views_desc) == %d, "size");\n_Static_assert(sizeof(pv_resample_desc) == %d, "size");\n'
                   % (C.sizeof(L.VideoViewsDesc), C.sizeof(L.ResampleDesc)))
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(L.VideoViewsDesc) == 152 and C.sizeof(L.ResampleDesc) == 152        # byte for byte what they were
    src.write_text(text % (C.sizeof(L.YuvViewsDesc) + 8))
    assert subprocess.run(cmd, capture_output=True).returncode != 0                      # the assertion does fire


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def yuv_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("isa_yuv") / "pv_yuv.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_yuv.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_every_yuv_instantiation_is_free_of_scratch_and_spills(yuv_asm):
    """2 chroma forms (c_step 1, 2) x 5 destination forms: no private segment and no spilled register.  The VGPR counts are
    printed (DESIGN.md 4.6 records them); they are not gated."""
    kernels = re.findall(r"\.name:\s+(\S*yuv_views_kernel\S*)\n(.*?)\.wavefront_size", yuv_asm, re.S)
    assert len(kernels) == 10, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
    assert "resample_crop_kernel" not in yuv_asm                 # pv_resample.hip keeps its kernels to itself
