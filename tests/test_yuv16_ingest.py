"""10- to 16-bit YUV 4:2:0 sources of the ingest (P010 / P012 / P016, I010 / I012 / I016), without a GPU: the entry point
`pv_yuv16_views` and the `PV_U16` source dtype of `pv_batch_views` / `pv_frame_views` (include/pv_mi355x.h) -- exported,
versioned, validated before any launch --, `transforms.yuv_matrix` with a bit depth and a bit alignment, `yuv_geometry` and
the host mirror `yuv420_to_rgb` on 16-bit surfaces, the code-object metadata of the 30 new kernels, and the host plumbing
(`FrameList`, `build_video_batch`)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import yuv16_util as Y16
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- export, versioning
def test_yuv16_views_is_exported_and_versioned(pv_lib, tmp_path):
    assert "pv_yuv16_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_yuv16_views")
    assert L.PV_U16 == 3 and (L.PV_F32, L.PV_BF16, L.PV_U8) == (0, 1, 2)
    assert pv_lib.pv_version() == L.ABI_VERSION == 36            # additive: no descriptor changed
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "int pv_yuv16_views(const pv_yuv_views_desc* d, pv_stream_t stream);" in header
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    src = tmp_path / "size.c"
    text = ('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_yuv_views_desc) == %d, "size");\n'
            '_Static_assert(PV_U16 == 3, "value");\n_Static_assert(sizeof(pv_batch_views_desc) == %d, "size");\n'
            '_Static_assert(sizeof(pv_view_source) == 96, "size");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    assert C.sizeof(L.YuvViewsDesc) == 184                       # what it was before the 16-bit entry point
    src.write_text(text % (C.sizeof(L.YuvViewsDesc), C.sizeof(L.BatchViewsDesc)))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src.write_text(text % (C.sizeof(L.YuvViewsDesc) + 8, C.sizeof(L.BatchViewsDesc)))
    assert subprocess.run(cmd, capture_output=True).returncode != 0          # the assertion does fire


# ----------------------------------------------------------------------------- pv_yuv16_views: rejection table
def _desc(keep):
    """A valid smallest descriptor: 2 clips of 1 frame from two P010 frames of 2 x 2 -- 12 bytes each: two luma rows of 4
    bytes, one chroma row of 4 -- in host memory (validation happens before any HIP call)."""
    src, dst, tab, mat = (C.c_uint8 * 64)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)(), (C.c_float * 12)()
    keep.extend([src, dst, tab, mat])
    d = L.YuvViewsDesc()
    d.src = C.addressof(src) + (-C.addressof(src)) % 16 + 2      # even, and no more than that
    d.dst = C.addressof(dst) + (-C.addressof(dst)) % 16
    d.t_index, d.yuv2rgb = C.addressof(tab), C.addressof(mat)
    d.n_clips, d.T, d.N, d.t_stride, d.Hs, d.Ws = 2, 1, 2, 1, 2, 2
    d.frame_stride, d.y_pitch, d.c_pitch, d.c_step, d.u_offset, d.v_offset = 12, 4, 4, 2, 8, 10
    d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = 2, 2, 1, 1, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    return d


def _status(d):
    return L.lib().pv_yuv16_views(C.byref(d), None)


def _with(keep, **fields):
    d = _desc(keep)
    for k, val in fields.items():
        setattr(d, k, val)
    return d


def _huge(keep, hs=16, ws=9000):
    """One P010 frame of 16 x 9000 taken whole: every check passes but the last, the LDS limit of a staged strip (two luma
    rows of 18 000 bytes and their chroma rows are beyond 64 KiB).  Nothing is read: the source is never dereferenced."""
    d = _desc(keep)
    d.n_clips, d.N, d.Hs, d.Ws, d.Hn, d.Wn, d.Ho, d.Wo = 1, 1, hs, ws, hs, ws, hs, ws
    d.y_pitch = d.c_pitch = 2 * ws
    d.u_offset, d.v_offset, d.frame_stride = hs * 2 * ws, hs * 2 * ws + 2, hs * 3 * ws
    return d


def test_the_valid_base_stops_at_the_last_check_only(pv_lib):
    """The positive control of the table below: the same fields at a size the kernels cannot stage are PV_ERR_UNSUPPORTED,
    from the check that comes last, so PV_ERR_INVALID below is the named field's doing.  And the 8-bit entry point refuses
    the base for its own reason (|v - u| is 2, not 1), so the two entry points do count differently."""
    keep = []
    assert _status(_huge(keep)) == UNS
    assert pv_lib.pv_yuv_views(C.byref(_desc(keep)), None) == INV
    d = _huge(keep)
    d.src += 1
    assert _status(d) == INV                                     # validation order: evenness before the LDS limit


def test_yuv16_views_rejects_invalid_descriptors_without_a_gpu(pv_lib):
    keep = []
    assert pv_lib.pv_yuv16_views(None, None) == INV
    assert _status(L.YuvViewsDesc()) == INV
    for field in ("src", "dst", "t_index", "yuv2rgb"):
        assert _status(_with(keep, **{field: None})) == INV, field
    for field in ("n_clips", "T", "N", "Hs", "Ws"):
        for val in (0, -2):
            assert _status(_with(keep, **{field: val})) == INV, field
    assert _status(_with(keep, T=2, t_stride=1)) == INV
    # odd frame sizes (everything else large enough for them)
    assert _status(_with(keep, Hs=3, Hn=3, frame_stride=128, u_offset=16, v_offset=18)) == INV
    assert _status(_with(keep, Ws=3, Wn=3, y_pitch=8, c_pitch=8, frame_stride=128, u_offset=16, v_offset=18)) == INV
    for step in (0, 3, 4, -1):
        assert _status(_with(keep, c_step=step)) == INV, step
    # extents count 2 bytes per sample
    assert _status(_with(keep, y_pitch=2)) == INV                              # y_pitch < 2 * Ws (2 would do for bytes)
    assert _status(_with(keep, c_pitch=2)) == INV                              # c_pitch < 2 * (Ws/2) * c_step
    assert _status(_with(keep, c_step=1, c_pitch=0, u_offset=8, v_offset=10)) == INV
    # planes that leave the frame
    assert _status(_with(keep, frame_stride=6)) == INV                         # luma: 2 rows of pitch 4 need 8 bytes
    assert _status(_with(keep, frame_stride=10)) == INV                        # the V sample is bytes 10..11
    assert _status(_with(keep, frame_stride=0)) == INV
    assert _status(_with(keep, frame_stride=-12)) == INV
    assert _status(_with(keep, u_offset=-2, v_offset=0)) == INV
    assert _status(_with(keep, u_offset=10, v_offset=12)) == INV
    assert _status(_with(keep, c_step=1, c_pitch=2, u_offset=8, v_offset=12)) == INV       # planar V behind the frame
    assert _status(_with(keep, u_offset=1 << 40, v_offset=(1 << 40) + 2)) == INV
    # an interleaved plane holds U and V side by side: 2 bytes apart, not 1, not 4, not 0
    assert _status(_with(keep, frame_stride=16, u_offset=8, v_offset=12)) == INV
    assert _status(_with(keep, u_offset=8, v_offset=8)) == INV
    assert _status(_with(keep, frame_stride=16, u_offset=8, v_offset=9)) == INV             # |v - u| == 1: the 8-bit form
    # the six evenness checks, one at a time, everything else large enough
    d = _desc(keep)
    d.src += 1
    assert _status(d) == INV
    assert _status(_with(keep, frame_stride=13)) == INV
    assert _status(_with(keep, frame_stride=16, y_pitch=5)) == INV
    assert _status(_with(keep, frame_stride=16, c_pitch=5)) == INV
    assert _status(_with(keep, frame_stride=32, c_step=1, c_pitch=2, u_offset=9, v_offset=12)) == INV
    assert _status(_with(keep, frame_stride=32, c_step=1, c_pitch=2, u_offset=8, v_offset=13)) == INV
    # the checks of pv_resample_crop
    for nv in (0, 4, -1):
        assert _status(_with(keep, n_views=nv)) == INV
    for field, val in (("y_off", 2), ("x_off", 2), ("y_off", -1), ("x_off", -1)):
        d = _desc(keep)
        getattr(d, field)[0] = val
        assert _status(d) == INV, field
    assert _status(_with(keep, Ho=3)) == INV
    for item0, n in ((0, 3), (2, 1), (-1, 1), (1, 0)):
        assert _status(_with(keep, item0=item0, n_items=n)) == INV, (item0, n)
    d = _with(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=8)
    d.dst += 2
    assert _status(d) == INV
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=4)) == INV
    d = _desc(keep)
    d.dst += 1
    assert _status(d) == INV
    # outside the destination matrix
    assert _status(_with(keep, dst_dtype=L.PV_U8)) == UNS
    assert _status(_with(keep, dst_dtype=L.PV_U16)) == UNS
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, dst_dtype=L.PV_F32, c_p=4, ld=4, bs=4)) == UNS
    assert _status(_with(keep, dst_layout=L.DST_NDHWC, c_p=6, ld=8, bs=8)) == UNS
    assert _status(_with(keep, dst_layout=7)) == UNS


# ----------------------------------------------------------------------------- pv_batch_views / pv_frame_views: PV_U16
W = 20000


def _f32(a, b):
    return C.c_float(a / b).value


def _batch_desc(keep, frames=False):
    """Two P010 sources -- 2 frames of 2 x W and 3 frames of 6 x W scaled to 3 x W, W = 20000 -- and 4 items of 1 x W that
    pass EVERY check but the last, the LDS limit (tests/test_batch_views.py, `_desc`, in bytes of 2-byte samples).  With
    `frames` the sources are slices of a pointer table of 6 even frame addresses (tests/test_frame_views.py)."""
    src, dst, tab, mat = (C.c_uint8 * 512)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)(), (C.c_float * 12)()
    sources, items, ptrs = (L.ViewSource * 2)(), (L.ViewItem * 4)(), (C.c_uint64 * 6)()
    keep.extend([src, dst, tab, mat, sources, items, ptrs])
    base = C.addressof(src) + (-C.addressof(src)) % 16
    for i in range(6):
        ptrs[i] = base + 16 * (5 - i) + 2
    firsts = (C.addressof(ptrs), C.addressof(ptrs) + 16) if frames else (base + 2, base + 64)
    for rec, first, (n, hs, hn) in zip(sources, firsts, ((2, 2, 2), (3, 6, 3))):
        rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn = first, n, hs, W, hn, W
        rec.sy, rec.sx = _f32(hs, hn), _f32(W, W)
        rec.y_pitch = rec.c_pitch = 2 * W
        rec.u_offset, rec.v_offset, rec.frame_stride = hs * 2 * W, hs * 2 * W + 2, hs * 3 * W
    for i, (s, r) in enumerate(((1, 2), (0, 0), (1, 1), (0, 0))):
        items[i].source, items[i].row, items[i].view = s, r, 0
    f = L.FrameViewsDesc()
    f.frame_ptrs = f.frame_ptrs_dev = C.addressof(ptrs)
    f.n_frame_ptrs = 6
    d = f.batch
    d.sources = d.sources_dev = C.addressof(sources)
    d.items = d.items_dev = C.addressof(items)
    d.t_index, d.dst = C.addressof(tab), C.addressof(dst) + (-C.addressof(dst)) % 16
    d.n_sources, d.n_items, d.n_rows, d.t_stride, d.C, d.T = 2, 4, 3, 1, 3, 1
    d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U16, L.SRC_YUV420, 2, C.addressof(mat)
    d.Ho, d.Wo, d.n_views = 1, W, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    return f, sources, ptrs


def _bstatus(f, frames):
    return L.lib().pv_frame_views(C.byref(f), None) if frames else L.lib().pv_batch_views(C.byref(f.batch), None)


@pytest.mark.parametrize("frames", [False, True], ids=["batch_views", "frame_views"])
def test_u16_launches_are_validated_before_any_launch(pv_lib, frames):
    keep = []
    f, _, _ = _batch_desc(keep, frames)
    assert _bstatus(f, frames) == UNS                            # the valid base stops at the last check only
    # PV_U16 belongs to YUV 4:2:0: 16-bit RGB is out of scope
    for layout in (L.SRC_NCTHW, L.SRC_NTHWC):
        f, _, _ = _batch_desc(keep, frames)
        f.batch.src_layout = layout
        assert _bstatus(f, frames) == UNS, layout
    # the evenness checks per record named by an item (both records are named)
    for index in (0, 1):
        for field, delta in (("frame_stride", 1), ("u_offset", -1), ("v_offset", 1), ("y_pitch", 1), ("c_pitch", 1)):
            f, sources, _ = _batch_desc(keep, frames)
            setattr(sources[index], field, getattr(sources[index], field) + delta)
            if field == "u_offset":
                sources[index].v_offset -= 1                     # keeps |v - u| == 2: only the parity is wrong
            assert _bstatus(f, frames) == INV, (index, field)
    # extents in bytes: the 8-bit pitch of the same frame is too short, and |v - u| == 1 is the 8-bit form
    f, sources, _ = _batch_desc(keep, frames)
    sources[1].y_pitch = W
    assert _bstatus(f, frames) == INV
    f, sources, _ = _batch_desc(keep, frames)
    sources[0].v_offset = sources[0].u_offset + 1
    assert _bstatus(f, frames) == INV
    if frames:
        for k in (0, 1, 2, 4):                                   # an odd frame address in a slice that an item names
            f, _, ptrs = _batch_desc(keep, True)
            ptrs[k] += 1
            assert _bstatus(f, True) == INV, k
        f, _, ptrs = _batch_desc(keep, True)
        ptrs[5] += 1                                             # the spare entry belongs to no slice
        assert _bstatus(f, True) == UNS
        f, _, ptrs = _batch_desc(keep, True)
        f.batch.src_dtype = L.PV_U8                              # ... and bytes may lie anywhere (|v - u| is then wrong)
        ptrs[0] += 1
        assert _bstatus(f, True) == INV
    else:
        for index in (0, 1):
            f, sources, _ = _batch_desc(keep, False)
            sources[index].src += 1
            assert _bstatus(f, False) == INV, index


# ----------------------------------------------------------------------------- matrix
KR_KB = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114), "bt2020": (0.2627, 0.0593)}


def _old_matrix(standard, full_range):
    """`yuv_matrix` as it was before it took a depth, restated."""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    y_lo, y_span, c_span = (0.0, 255.0, 255.0) if full_range else (16.0, 219.0, 224.0)
    ys, cs = 255.0 / y_span, 255.0 / c_span
    m = torch.tensor([[ys, 0.0, 2.0 * (1.0 - kr) * cs],
                      [ys, -2.0 * kb * (1.0 - kb) / kg * cs, -2.0 * kr * (1.0 - kr) / kg * cs],
                      [ys, 2.0 * (1.0 - kb) * cs, 0.0]], dtype=torch.float64)
    const = -(m[:, 0] * y_lo + (m[:, 1] + m[:, 2]) * 128.0)
    return torch.cat([m, const[:, None]], dim=1)


def _apply(m, yuv):
    return m[:, :3] @ torch.tensor(yuv, dtype=torch.float64) + m[:, 3]


def test_matrix_defaults_are_the_8_bit_matrix_bit_for_bit():
    for standard in ("bt709", "bt601"):
        for full in (False, True):
            want = _old_matrix(standard, full)
            assert torch.equal(TR.yuv_matrix(standard, full), want)
            assert torch.equal(TR.yuv_matrix(standard, full, 8, False), want)
            assert torch.equal(TR.yuv_matrix(standard, full, bit_depth=8, msb_aligned=False), want)
    assert torch.equal(TR.yuv_matrix(), _old_matrix("bt709", False))
    for bad in (7, 17, 10.0):
        with pytest.raises(ValueError):
            TR.yuv_matrix("bt709", False, bad)


@pytest.mark.parametrize("standard", ["bt709", "bt601"])
def test_matrix_of_a_deeper_limited_stream_is_the_8_bit_matrix_scaled(standard):
    m8 = TR.yuv_matrix(standard, False)
    msb = []
    for d in (10, 12, 16):
        m = TR.yuv_matrix(standard, False, d)
        k = 2.0 ** -(d - 8)
        assert ((m[:, :3] - m8[:, :3] * k).abs() <= 1e-15 * (m8[:, :3] * k).abs()).all(), d
        assert ((m[:, 3] - m8[:, 3]).abs() <= 1e-15 * m8[:, 3].abs()).all(), d
        lo, hi = 16 * 2 ** (d - 8), 235 * 2 ** (d - 8)
        assert torch.allclose(_apply(m, (lo, 2 ** (d - 1), 2 ** (d - 1))), torch.zeros(3, dtype=torch.float64), atol=1e-9)
        assert torch.allclose(_apply(m, (hi, 2 ** (d - 1), 2 ** (d - 1))), torch.full((3,), 255.0, dtype=torch.float64), atol=1e-9)
        msb.append(TR.yuv_matrix(standard, False, d, True))
        assert torch.equal(msb[-1][:, :3], m[:, :3] * 2.0 ** -(16 - d)) and torch.equal(msb[-1][:, 3], m[:, 3])
    # MSB-aligned, the three depths are one matrix: the 8-bit one with its Y, U, V columns times 2^-8
    assert torch.equal(msb[0], msb[1]) and torch.equal(msb[1], msb[2])
    assert torch.equal(msb[0][:, :3], m8[:, :3] * 2.0 ** -8) and torch.equal(msb[0][:, 3], m8[:, 3])


def test_matrix_full_range_depth_10_and_bt2020():
    for standard in ("bt709", "bt601", "bt2020"):
        full = TR.yuv_matrix(standard, True, 10)
        assert torch.allclose(_apply(full, (1023, 512, 512)), torch.full((3,), 255.0, dtype=torch.float64), atol=1e-9)
        assert torch.allclose(_apply(full, (0, 512, 512)), torch.zeros(3, dtype=torch.float64), atol=1e-9)
    # bt2020: the rows reproduce (Kr, Kb) -- Y' = Kr R' + Kg G' + Kb B' of the matrix's own primaries, and white is white
    kr, kb = KR_KB["bt2020"]
    m = TR.yuv_matrix("bt2020", False, 10)
    a = m[:, :3]
    luma = torch.tensor([kr, 1.0 - kr - kb, kb], dtype=torch.float64)
    # the luma of RGB = M . (Y, U, V) depends on Y alone: luma . (U column) == luma . (V column) == 0
    assert abs(float(luma @ a[:, 1])) <= 1e-12 and abs(float(luma @ a[:, 2])) <= 1e-12
    assert torch.allclose(a[:, 0], torch.full((3,), 255.0 / (219.0 * 4.0), dtype=torch.float64), rtol=1e-15, atol=0)
    assert abs(float(a[0, 2]) - 2.0 * (1.0 - kr) * 255.0 / 896.0) <= 1e-15 and abs(float(a[2, 1]) - 2.0 * (1.0 - kb) * 255.0 / 896.0) <= 1e-15
    assert torch.allclose(_apply(m, (940, 512, 512)), torch.full((3,), 255.0, dtype=torch.float64), atol=1e-9)
    assert torch.allclose(_apply(m, (64, 512, 512)), torch.zeros(3, dtype=torch.float64), atol=1e-9)
    with pytest.raises(ValueError, match="bit_depth >= 10"):
        TR.yuv_matrix("bt2020", False, 8)                        # Rec. 2020 defines no 8-bit quantisation
    # a (standard, full_range) pair is composed with the layout; an explicit matrix is taken as it is
    assert torch.equal(TR._yuv_matrix_of(("bt2020", False), "P010"), TR.yuv_matrix("bt2020", False, 10, True))
    assert torch.equal(TR._yuv_matrix_of(("bt709", True), "I012"), TR.yuv_matrix("bt709", True, 12, False))
    assert torch.equal(TR._yuv_matrix_of(("bt601", False), "NV12"), TR.yuv_matrix("bt601", False))
    assert torch.equal(TR._yuv_matrix_of(m, "P016"), m)
    assert TR.YUV_LAYOUTS == ("NV12", "NV21", "I420", "YV12")
    assert TR.YUV16_LAYOUTS == ("P010", "P012", "P016", "I010", "I012", "I016")


# ----------------------------------------------------------------------------- geometry, mirror
M10 = TR.yuv_matrix("bt2020", False, 10)
M16 = TR.yuv_matrix("bt709", False, 16, True)


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int16], ids=["uint16", "int16"])
@pytest.mark.parametrize("layout", ["P010", "I010"])
def test_geometry_and_mirror_against_independently_packed_surfaces(layout, dtype):
    """Pitch W + 3 samples (I010: W + 4, its chroma rows have half the pitch), coded height above the display height, the
    base one sample into the buffer, garbage everywhere else; codes up to 65535, so that a signed read is off by 65536 M."""
    y, u, v = Y16.planes(3, 10, 12, 2100, 0, 65536)
    assert int((y >= 32768).sum()) > 100 and int((u >= 32768).sum()) > 20
    want = Y16.rgb_of_planes(y, u, v, M16).float()
    pitch = 15 if layout == "P010" else 16
    packed = Y16.pack(y, u, v, layout, coded_height=12, pitch=pitch, base=1, garbage=8)
    frames = packed.frames(dtype=dtype)
    assert frames.dtype == dtype and frames.stride() == (18 * pitch, pitch, 1) and frames.storage_offset() == 1
    g = TR.yuv_geometry(frames, layout, coded_height=12, height=10)
    first = 12 * pitch
    if layout == "P010":
        chroma = dict(c_pitch=2 * pitch, c_step=2, u_offset=2 * first, v_offset=2 * first + 2)
    else:
        chroma = dict(c_pitch=pitch, c_step=1, u_offset=2 * first, v_offset=2 * (first + 6 * (pitch // 2)))
    assert g == dict(N=3, Hs=10, Ws=12, Hc=12, frame_stride=2 * 18 * pitch, y_pitch=2 * pitch, **chroma)     # bytes
    got = TR.yuv420_to_rgb(frames, layout, M16, coded_height=12, height=10)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, 10, 12)
    assert torch.equal(got, want)
    # tight, and as clips [B, T, Hc*3/2, W]
    tight = Y16.pack(y, u, v, layout).frames(dtype=dtype)
    assert torch.equal(TR.yuv420_to_rgb(tight, layout, M16), want)
    clips = tight[:2].reshape(2, 1, 15, 12)
    assert torch.equal(TR.yuv420_to_rgb(clips, layout, M16), want[:2].reshape(2, 1, 3, 10, 12))
    # a 10-bit stream, LSB-aligned codes
    y, u, v = Y16.planes(2, 10, 12, 2101)
    ten = Y16.pack(y, u, v, layout, pitch=pitch, base=1, garbage=9).frames(dtype=dtype)
    assert torch.equal(TR.yuv420_to_rgb(ten, layout, M10), Y16.rgb_of_planes(y, u, v, M10).float())


def test_geometry_refuses_the_wrong_sample_width():
    y, u, v = Y16.planes(2, 10, 12, 2102)
    wide = Y16.pack(y, u, v, "P010").frames()
    narrow = torch.zeros((2, 15, 12), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint16 or int16"):
        TR.yuv_geometry(narrow, "P010")
    with pytest.raises(RuntimeError, match="NV12 frames are uint8"):
        TR.yuv_geometry(wide, "NV12")
    with pytest.raises(RuntimeError, match="even"):
        TR.yuv_geometry(Y16.pack(y, u, v, "P010", pitch=13).frames(), "I010")
    for layout in TR.YUV16_LAYOUTS:
        g = TR.yuv_geometry(wide, layout)
        assert g["c_step"] == (2 if layout.startswith("P") else 1) and g["y_pitch"] == 24 and g["frame_stride"] == 2 * 15 * 12


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def asm16(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = {}
    tmp = tmp_path_factory.mktemp("isa_yuv16")
    for unit in ("pv_yuv", "pv_batch", "pv_frames16"):
        path = str(tmp / (unit + ".s"))
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                               os.path.join(ROOT, "pytorchvideo_amd", "csrc", unit + ".hip")], stderr=subprocess.DEVNULL)
        out[unit] = open(path).read()
    return out


@pytest.mark.parametrize("unit,kernel", [("pv_yuv", "yuv16_views_kernel"), ("pv_batch", "batch_yuv16_kernel"),
                                         ("pv_frames16", "frame_yuv16_kernel")])
def test_every_16_bit_instantiation_is_free_of_scratch_and_spills(asm16, unit, kernel):
    """2 chroma forms x 5 destination forms of each of the three new kernels: no private segment and no spilled register,
    the G = 8 planar forms included.  The register counts are printed (DESIGN.md 4.9 records them); they are not gated."""
    kernels = re.findall(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % kernel, asm16[unit], re.S)
    assert len(kernels) == 10, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


# ----------------------------------------------------------------------------- host plumbing
def _tables(counts, frames, t):
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, n, (c, t), generator=g, dtype=torch.int32) for c, n in zip(counts, frames)]


def test_frame_list_of_16_bit_surfaces():
    y, u, v = Y16.planes(4, 10, 12, 2103)
    for dtype in (torch.uint16, torch.int16):
        video = Y16.pack(y, u, v, "P010", coded_height=12, pitch=16, base=1).frames(dtype=dtype)
        fl = TR.FrameList(list(video.unbind(0)), src_layout="P010")
        assert len(fl) == 4 and fl.dtype == dtype
        c, hs, ws, geom = fl.geometry("P010", coded_height=12, height=10)
        assert (c, hs, ws) == (3, 10, 12)
        assert (geom["y_pitch"], geom["c_pitch"], geom["u_offset"], geom["v_offset"]) == (32, 32, 12 * 32, 12 * 32 + 2)
        with pytest.raises(RuntimeError, match="NV12 frames are uint8"):
            fl.geometry("NV12")
    with pytest.raises(RuntimeError, match="uint16 or int16"):
        TR.FrameList([torch.zeros((15, 12), dtype=torch.uint8)], src_layout="I010")


def test_video_batch_of_16_bit_videos_carries_byte_geometry_and_pv_u16():
    cpu = torch.device("cpu")
    a = Y16.pack(*Y16.planes(6, 64, 86, 2104), "P010", coded_height=72, pitch=96, base=1).frames()
    b = Y16.pack(*Y16.planes(5, 70, 60, 2105), "P010").frames(dtype=torch.int16)
    tables = _tables((2, 3), (6, 5), 4)
    uploaded = []

    def upload(t):
        uploaded.append(t)
        return t

    batch = TR.build_video_batch([a, b], tables, "P010", 56, 56, (0, 1, 2), [4], 3, cpu, upload, height=[64, None],
                                 coded_height=[72, None])
    assert batch.src_dtype == L.PV_U16 == 3 and batch.total == 15
    ra, rb = batch.sources[0], batch.sources[1]
    assert (ra.N, ra.Hs, ra.Ws, ra.y_pitch, ra.c_pitch) == (6, 64, 86, 192, 192)
    assert (ra.frame_stride, ra.u_offset, ra.v_offset) == (108 * 192, 72 * 192, 72 * 192 + 2)
    assert ra.src == a.data_ptr() and ra.src % 2 == 0
    assert (rb.N, rb.Hs, rb.Ws, rb.y_pitch, rb.c_pitch, rb.frame_stride) == (5, 70, 60, 120, 120, 105 * 120)
    assert (rb.u_offset, rb.v_offset) == (70 * 120, 70 * 120 + 2)
    planar = TR.build_video_batch([Y16.pack(*Y16.planes(5, 70, 60, 2105), "I010").frames()], tables[1:], "I010", 56, 56, (1,),
                                  [4], 3, cpu, upload)
    rp = planar.sources[0]
    assert planar.src_dtype == L.PV_U16 and (rp.y_pitch, rp.c_pitch, rp.u_offset, rp.v_offset) == (120, 60, 70 * 120, 70 * 120 + 35 * 60)
    # the 8-bit layouts keep PV_U8
    nv12 = torch.zeros((5, 105, 60), dtype=torch.uint8)
    assert TR.build_video_batch([nv12], tables[1:], "NV12", 56, 56, (1,), [4], 3, cpu, upload).src_dtype == L.PV_U8
    # one launch has one sample width: a mixed list is refused, with the reason
    with pytest.raises(RuntimeError, match="P010 frames are uint16 or int16.*torch.uint8"):
        TR.build_video_batch([b, nv12], tables, "P010", 56, 56, (0, 1, 2), [4], 3, cpu, upload)
    with pytest.raises(RuntimeError, match="NV12 frames are uint8.*int16"):
        TR.build_video_batch([nv12, b], [tables[1], tables[1]], "NV12", 56, 56, (0, 1, 2), [4], 3, cpu, upload)
    lists = [TR.FrameList(list(b.unbind(0))), TR.FrameList(list(nv12.unbind(0)))]
    with pytest.raises(RuntimeError):
        TR.build_video_batch(lists, [tables[1], tables[1]], "P010", 56, 56, (0, 1, 2), [4], 3, cpu, upload)
    fl = TR.build_video_batch(lists[:1], tables[1:], "P010", 56, 56, (0, 1, 2), [4], 3, cpu, upload)
    assert fl.src_dtype == L.PV_U16 and fl.frame_ptrs.numel() == 5 and fl.sources[0].y_pitch == 120
