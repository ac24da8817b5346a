"""Frame-list sources, without a GPU: the descriptor of `pv_frame_views` (include/pv_mi355x.h) -- exported, versioned,
mirrored by ctypes, validated before any launch --, the code-object metadata of its kernels (pytorchvideo_amd/csrc/
pv_frames.hip), `transforms.FrameList` and the pointer table `build_video_batch` makes of a list of them, and the host half
of `inference.StreamPredictor`: `data.stream_windows` against the uniform sampler and the bound on the frames held."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import inference as INF
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.data import UniformClipSampler, clip_frame_table, stream_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- descriptor
def _f32(a, b):
    """(float)a / (float)b as the C compiler divides: rounded to fp32."""
    return C.c_float(a / b).value


def _record(rec, src, n, hs, ws, hn, wn):
    rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn = src, n, hs, ws, hn, wn
    rec.sy, rec.sx = _f32(hs, hn), _f32(ws, wn)


W = 40000


def _desc(keep, yuv=False):
    """A descriptor in host memory that passes EVERY check but the last one, the LDS limit of a staged strip: two sources --
    2 frames of 2 x W and 3 frames of 6 x W scaled to 3 x W, W = 40000 --, a pointer table of 6 entries (source 0: entries
    0..1, source 1: entries 2..4, one spare), a frame table of 3 rows, 4 items of 1 x W, one view.  RGB planar uint8, or NV12
    with frames at odd addresses.  The limit is checked last, so this base returns PV_ERR_UNSUPPORTED -- the positive
    control of every PV_ERR_INVALID case below -- and nothing here is ever launched, with a GPU or without."""
    src, dst, tab, mat = (C.c_uint8 * 512)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)(), (C.c_float * 12)()
    sources, items, ptrs = (L.ViewSource * 2)(), (L.ViewItem * 4)(), (C.c_uint64 * 6)()
    keep.extend([src, dst, tab, mat, sources, items, ptrs])
    base = C.addressof(src) + (-C.addressof(src)) % 16
    for i in range(6):
        ptrs[i] = base + 16 * (5 - i) + (1 if yuv else 0)         # any order; uint8 frames need no alignment
    _record(sources[0], C.addressof(ptrs), 2, 2, W, 2, W)
    _record(sources[1], C.addressof(ptrs) + 16, 3, 6, W, 3, W)
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
    d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NCTHW
    d.Ho, d.Wo, d.n_views = 1, W, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    if yuv:
        d.src_layout, d.c_step, d.yuv2rgb = L.SRC_YUV420, 2, C.addressof(mat)
        for rec, (hs, ws) in zip(sources, ((2, W), (6, W))):
            rec.y_pitch = rec.c_pitch = ws
            rec.u_offset, rec.v_offset, rec.frame_stride = hs * ws, hs * ws + 1, hs * ws * 3 // 2
    return f, sources, items, ptrs


def _status(f):
    return L.lib().pv_frame_views(C.byref(f), None)


def _bad(keep, yuv=False, outer=None, **fields):
    f, _, _, _ = _desc(keep, yuv)
    for k, v in (outer or {}).items():
        setattr(f, k, v)
    for k, v in fields.items():
        setattr(f.batch, k, v)
    return _status(f)


def _bad_record(keep, index, yuv=False, **fields):
    f, sources, _, _ = _desc(keep, yuv)
    for k, v in fields.items():
        setattr(sources[index], k, v)
    return _status(f)


def test_frame_views_is_exported_and_versioned(pv_lib):
    assert "pv_frame_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_frame_views")
    assert pv_lib.pv_version() == L.ABI_VERSION == 36            # additive: no descriptor changed
    header = open(os.path.join(ROOT, "include", "pv_mi355x.h")).read()
    assert "int pv_frame_views(const pv_frame_views_desc* d, pv_stream_t stream);" in header


def test_ctypes_mirror_has_the_size_of_the_c_struct(tmp_path):
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    assert C.sizeof(L.FrameViewsDesc) == C.sizeof(L.BatchViewsDesc) + 24 and C.sizeof(L.ViewSource) == 96
    assert L.FrameViewsDesc.batch.offset == 0 and L.FrameViewsDesc.frame_ptrs.offset == C.sizeof(L.BatchViewsDesc)
    src = tmp_path / "size.c"
    text = ('#include <stddef.h>\n#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_frame_views_desc) == %d, "size");\n'
            '_Static_assert(offsetof(pv_frame_views_desc, frame_ptrs_dev) == %d, "offset");\n'
            '_Static_assert(offsetof(pv_frame_views_desc, n_frame_ptrs) == %d, "offset");\n'
            '_Static_assert(sizeof(pv_view_source) == 96, "the record keeps its layout");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    sizes = [C.sizeof(L.FrameViewsDesc), L.FrameViewsDesc.frame_ptrs_dev.offset, L.FrameViewsDesc.n_frame_ptrs.offset]
    src.write_text(text % tuple(sizes))
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i in range(3):                                           # every assertion does fire
        off = list(sizes)
        off[i] += 8
        src.write_text(text % tuple(off))
        assert subprocess.run(cmd, capture_output=True).returncode != 0, i


def test_the_base_descriptors_stop_at_the_last_check_only(pv_lib):
    keep = []
    for yuv in (False, True):
        f, _, _, _ = _desc(keep, yuv)
        assert _status(f) == UNS, yuv


def test_frame_views_rejects_what_batch_views_rejects(pv_lib):
    keep = []
    assert pv_lib.pv_frame_views(None, None) == INV
    assert _status(L.FrameViewsDesc()) == INV
    for field in ("sources", "sources_dev", "items", "items_dev", "t_index", "dst"):
        assert _bad(keep, **{field: None}) == INV, field
    assert _bad(keep, yuv=True, yuv2rgb=None) == INV
    for field in ("n_sources", "n_items", "n_rows", "T"):
        for val in (0, -1):
            assert _bad(keep, **{field: val}) == INV, (field, val)
    assert _bad(keep, T=2, t_stride=1) == INV                    # a row stride shorter than the row
    assert _bad(keep, n_items=65536) == INV                      # refused by the count, before any item is read
    assert _bad(keep, T=65536, t_stride=65536) == INV            # more frames than grid.y holds
    assert _bad(keep, T=65535, t_stride=65535) == UNS            # the positive control: the last count that fits
    assert _bad(keep, C=5) == INV
    assert _bad(keep, C=0) == INV
    for nv in (0, 4, -1):
        assert _bad(keep, n_views=nv) == INV, nv
    for dtype, ch in ((L.PV_F32, 3), (L.PV_U8, 4)):              # an interleaved frame is uint8 with 3 channels
        assert _bad(keep, src_layout=L.SRC_NTHWC, src_dtype=dtype, C=ch) == INV
    assert _bad(keep, src_layout=3) == INV
    assert _bad(keep, Ho=0) == INV
    assert _bad(keep, Wo=-1) == INV
    assert _bad(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=4) == INV      # items overlap
    f, _, _, _ = _desc(keep)
    f.batch.dst += 1                                             # a bf16 destination at an odd address
    assert _status(f) == INV
    assert _bad(keep, yuv=True, C=4) == INV
    for step in (0, 3, -1):
        assert _bad(keep, yuv=True, c_step=step) == INV, step
    # the dtype / layout matrix is reported as unsupported, as there
    assert _bad(keep, src_dtype=L.PV_BF16) == UNS
    assert _bad(keep, yuv=True, src_dtype=L.PV_F32) == UNS
    assert _bad(keep, dst_dtype=L.PV_U8) == UNS
    # records: sizes, the library's own division, windows inside the scaled frame
    for index in (0, 1):
        for field in ("N", "Hs", "Ws", "Hn", "Wn"):
            for val in (0, -3):
                assert _bad_record(keep, index, **{field: val}) == INV, (index, field, val)
    for field in ("sy", "sx"):
        f, sources, _, _ = _desc(keep)
        bits = C.c_uint32.from_buffer_copy(C.c_float(getattr(sources[1], field))).value
        setattr(sources[1], field, C.c_float.from_buffer_copy(C.c_uint32(bits + 1)).value)
        assert _status(f) == INV, field
    for field, val in (("y_off", 3), ("x_off", 1), ("y_off", -1), ("x_off", -1)):
        f, sources, _, _ = _desc(keep)
        getattr(sources[1], field)[0] = val
        assert _status(f) == INV, (field, val)
    # items
    for field, bad in (("source", 2), ("source", -1), ("row", 3), ("row", -1), ("view", 1), ("view", -1)):
        for index in (0, 3):
            f, _, items, _ = _desc(keep)
            setattr(items[index], field, bad)
            assert _status(f) == INV, (field, bad, index)
    # YUV planes of one frame: frame_stride is the extent of ONE frame
    assert _bad_record(keep, 1, yuv=True, Hs=5, Hn=5, sy=1.0) == INV                 # odd height
    assert _bad_record(keep, 1, yuv=True, y_pitch=W - 1) == INV
    assert _bad_record(keep, 1, yuv=True, c_pitch=W - 1) == INV
    assert _bad_record(keep, 1, yuv=True, frame_stride=0) == INV
    assert _bad_record(keep, 1, yuv=True, frame_stride=9 * W - 1) == INV             # the last V sample at byte 9 W - 1
    assert _bad_record(keep, 1, yuv=True, u_offset=6 * W, v_offset=6 * W + 2) == INV
    assert _bad_record(keep, 0, yuv=True, frame_stride=5) == INV
    assert _bad_record(keep, 1, yuv=True, u_offset=6 * W + 1, v_offset=6 * W) == UNS # NV21 beside NV12 in one launch


def test_frame_views_rejects_a_missing_pointer_table(pv_lib):
    keep = []
    for field in ("frame_ptrs", "frame_ptrs_dev"):
        assert _bad(keep, outer={field: None}) == INV, field
    for n in (0, -1):
        assert _bad(keep, outer={"n_frame_ptrs": n}) == INV, n


def test_frame_views_rejects_a_record_that_is_no_slice_of_the_table(pv_lib):
    keep = []
    for yuv in (False, True):
        for index in (0, 1):
            assert _bad_record(keep, index, yuv, src=None) == INV
        f, sources, _, ptrs = _desc(keep, yuv)
        table = C.addressof(ptrs)
        for index, n in ((0, 2), (1, 3)):
            good = sources[index].src
            for bad in (good + 4, good + 1, table - 8, table - 8 * n,          # not 8 k behind the table / in front of it
                        table + 8 * (6 - n + 1), table + 8 * 6, table + 8 * 100):   # k + N > n_frame_ptrs
                sources[index].src = bad
                assert _status(f) == INV, (yuv, index, bad - table)
            sources[index].src = table + 8 * (6 - n)             # the last slice that fits
            assert _status(f) == UNS, (yuv, index)
            sources[index].src = good
        # a table one entry shorter cuts the slice of source 1 (entries 2..4) only when it ends before entry 5
        f.n_frame_ptrs = 5
        assert _status(f) == UNS
        f.n_frame_ptrs = 4
        assert _status(f) == INV
        # slices may overlap and a record may be named by no item: only the records the items name are read
        f, sources, items, _ = _desc(keep, yuv)
        sources[1].src = sources[0].src
        assert _status(f) == UNS
        sources[0].src = 12345
        for it in items:
            it.source = 1
        assert _status(f) == UNS


def test_frame_views_rejects_a_null_frame_and_a_misaligned_fp32_frame(pv_lib):
    keep = []
    for yuv in (False, True):
        for entry in range(5):                                   # every entry of both slices
            f, _, _, ptrs = _desc(keep, yuv)
            ptrs[entry] = 0
            assert _status(f) == INV, (yuv, entry)
        f, _, _, ptrs = _desc(keep, yuv)
        ptrs[5] = 0                                              # the spare entry belongs to no slice
        assert _status(f) == UNS
    # uint8 frames may start at any byte; fp32 frames at multiples of 4
    for off in (1, 2, 3, 7):
        f, _, _, ptrs = _desc(keep)
        ptrs[3] += off
        assert _status(f) == UNS, off
        f.batch.src_dtype = L.PV_F32
        assert _status(f) == INV, off
    f, _, _, ptrs = _desc(keep)
    f.batch.src_dtype = L.PV_F32
    assert _status(f) == UNS
    ptrs[3] += 4
    assert _status(f) == UNS
    ptrs[5] += 2                                                 # the spare entry again
    assert _status(f) == UNS


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def frames_remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("isa_frames") / "pv_frames.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", out,
                        os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_frames.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stderr


def test_every_frame_instantiation_is_free_of_scratch_and_spills(frames_remarks):
    """3 source forms x 5 destination forms of the RGB / planar kernel and 2 chroma forms x 5 of the YUV kernel: no private
    segment and no spilled register in the code object's metadata, and the same in the compiler's resource-usage remarks;
    the RGB / planar kernels within the 72 VGPRs of their pv_batch_views twins (seven waves per SIMD)."""
    asm, remarks = frames_remarks
    kernels = re.findall(r"\.name:\s+(\S*frame_(?:views|yuv)_kernel\S*)\n(.*?)\.wavefront_size", asm, re.S)
    assert len([k for k in kernels if "frame_views_kernel" in k[0]]) == 15
    assert len([k for k in kernels if "frame_yuv_kernel" in k[0]]) == 10, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
        if "frame_views_kernel" in name:
            assert meta["vgpr_count"] <= 72, (name, meta["vgpr_count"])
    blocks = re.findall(r"Function Name: (\S+)(.*?)LDS Size", remarks, re.S)
    assert len(blocks) == 25
    for name, body in blocks:
        usage = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", body)}
        assert usage["ScratchSize"] == 0 and usage["SGPRs Spill"] == 0 and usage["VGPRs Spill"] == 0, (name, usage)
        assert usage["Occupancy"] >= 7, (name, usage)
    assert "batch_views_kernel" not in asm and "batch_yuv_kernel" not in asm


# ----------------------------------------------------------------------------- FrameList
def test_frame_list_accepts_views_repeats_and_any_order():
    buf = torch.zeros(5 * 30 * 3 + 16, dtype=torch.uint8)
    frames = [buf[off:off + 30].view(2, 5, 3) for off in (7, 301, 91, 7)]    # views at odd offsets, one twice, any order
    fl = TR.FrameList(frames, "NTHWC")
    assert len(fl) == 4 and fl.device == buf.device and fl.dtype == torch.uint8 and fl.shape == (2, 5, 3)
    assert all(a is b for a, b in zip(fl.frames, frames))        # kept alive, not copied
    assert fl.geometry("NTHWC") == (3, 2, 5, None)
    assert tuple(fl.stack("NTHWC").shape) == (4, 2, 5, 3)
    planar = TR.FrameList([torch.zeros(3, 4, 6) for _ in range(2)], "NCTHW")
    assert planar.geometry("NCTHW") == (3, 4, 6, None) and tuple(planar.stack("NCTHW").shape) == (3, 2, 4, 6)
    assert len(TR.FrameList(iter([torch.zeros(3, 4, 6, dtype=torch.uint8)]))) == 1    # any iterable
    # a YUV surface: any row pitch >= W, geometry from yuv_geometry of a one-frame view
    surf = torch.zeros(2, 12, 40, dtype=torch.uint8)
    nv = TR.FrameList([surf[1, :, :32], surf[0, :, :32]], "NV12")
    c, hs, ws, geom = nv.geometry("NV12")
    assert (c, hs, ws) == (3, 8, 32) and geom["y_pitch"] == 40 and geom["u_offset"] == 8 * 40 and geom["v_offset"] == 8 * 40 + 1
    assert geom["frame_stride"] == 12 * 40 and geom["N"] == 1
    assert nv.geometry("I420", height=6)[3]["c_pitch"] == 20


def test_frame_list_refuses_mixed_and_malformed_frames():
    f = torch.zeros(4, 6, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at least one frame"):
        TR.FrameList([])
    with pytest.raises(RuntimeError, match="shape"):
        TR.FrameList([f, torch.zeros(4, 5, 3, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="dtype"):
        TR.FrameList([f, f.float()])
    with pytest.raises(RuntimeError, match="strides"):
        TR.FrameList([f, torch.zeros(4, 3, 6, dtype=torch.uint8).transpose(1, 2)])
    with pytest.raises(RuntimeError, match="device"):
        TR.FrameList([f, torch.zeros(4, 6, 3, dtype=torch.uint8, device="meta")])
    with pytest.raises(TypeError):
        TR.FrameList([f, None])
    # the per-layout forms
    with pytest.raises(RuntimeError, match="contiguous"):
        TR.FrameList([torch.zeros(4, 3, 6, dtype=torch.uint8).transpose(1, 2)] * 2, "NTHWC")
    with pytest.raises(RuntimeError, match="contiguous"):
        TR.FrameList([torch.zeros(3, 4, 12, dtype=torch.uint8)[:, :, ::2]], "NCTHW")     # pitched RGB rows
    with pytest.raises(RuntimeError):
        TR.FrameList([f.float()], "NTHWC")                       # an interleaved frame is uint8
    with pytest.raises(RuntimeError):
        TR.FrameList([torch.zeros(4, 6, 2, dtype=torch.uint8)], "NTHWC")
    with pytest.raises(RuntimeError):
        TR.FrameList([torch.zeros(3, 4, 6, dtype=torch.float64)], "NCTHW")
    with pytest.raises(RuntimeError):
        TR.FrameList([f], "NV12")                                # a YUV frame is 2-d
    with pytest.raises(RuntimeError, match="pitch"):
        TR.FrameList([torch.as_strided(torch.zeros(400, dtype=torch.uint8), (12, 32), (30, 1))], "NV12")   # pitch below W
    with pytest.raises(RuntimeError, match="stride"):
        TR.FrameList([torch.zeros(12, 64, dtype=torch.uint8)[:, ::2]], "NV12")
    with pytest.raises(RuntimeError):
        TR.FrameList([torch.zeros(12, 32, dtype=torch.float32)], "NV12")
    with pytest.raises(ValueError):
        TR.FrameList([f], "NHWC")


# ----------------------------------------------------------------------------- host logic of video_batch
def _tables(counts, frames, t):
    out = []
    for j, (c, n) in enumerate(zip(counts, frames)):
        tab = (torch.arange(c * t).view(c, t) * 3 + j) % n
        tab[-1, -1] = n - 1
        out.append(tab.to(torch.int32))
    return out


def test_video_batch_builds_the_pointer_table_and_the_slices_on_the_host():
    """`build_video_batch` on FrameLists of CPU tensors, the upload stubbed out: three NTHWC videos of 4, 1 and 3 clips x 3
    views; the second list names one frame twice and runs against the allocation order."""
    frames, sizes, counts = (12, 9, 5), ((97, 131), (131, 97), (40, 53)), (4, 1, 3)
    lists = []
    for n, (h, w) in zip(frames, sizes):
        own = [torch.zeros((h, w, 3), dtype=torch.uint8) for _ in range(n)]
        lists.append(own)
    lists[1] = lists[1][::-1]
    lists[1][4] = lists[1][2]
    videos = [TR.FrameList(own) for own in lists]
    tables = _tables(counts, frames, 8)
    uploads = []

    def upload(t):
        uploads.append(t)
        return t

    b = TR.build_video_batch(videos, tables, "NTHWC", 64, 56, (0, 1, 2), [2, 8], 3, torch.device("cpu"), upload)
    assert len(uploads) == 7                                     # the pointer table, then what a batch of tensors uploads
    assert uploads[0] is b.frame_ptrs and b.frame_ptrs_dev is b.frame_ptrs
    assert b.frame_ptrs.dtype == torch.int64 and b.frame_ptrs.numel() == sum(frames) and b.frame_first == [0, 12, 21]
    assert b.frame_ptrs.tolist() == [f.data_ptr() for own in lists for f in own]     # video-major, list order
    assert b.frame_ptrs[12 + 4] == b.frame_ptrs[12 + 2]
    base = b.frame_ptrs_dev.data_ptr()
    assert base % 8 == 0
    for rec, first, (h, w), n in zip(b.sources, b.frame_first, sizes, frames):
        hn, wn = TR.scaled_size(h, w, 64)
        assert (rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (base + 8 * first, n, h, w, hn, wn)
        assert [(rec.y_off[k], rec.x_off[k]) for k in range(3)] == [TR.crop_offsets(hn, wn, 56, v) for v in (0, 1, 2)]
        assert rec.sy == _f32(h, hn) and rec.sx == _f32(w, wn) and rec.reserved == 0
    assert bytes(b.sources_dev.numpy().tobytes()) == bytes(b.sources)        # uploaded AFTER the slices were written
    # everything else is what a batch of tensors gets
    ref = TR.build_video_batch([v.stack() for v in videos], tables, "NTHWC", 64, 56, (0, 1, 2), [2, 8], 3, torch.device("cpu"),
                               lambda t: t)
    assert ref.frame_ptrs is None and ref.frame_ptrs_dev is None
    assert torch.equal(b.items_dev, ref.items_dev) and all(torch.equal(x, y) for x, y in zip(b.tables, ref.tables))
    assert (b.total, b.n_rows, b.clips, b.row0, b.src_dtype) == (ref.total, ref.n_rows, ref.clips, ref.row0, ref.src_dtype)
    assert all(v is w for v, w in zip(b.videos, videos))         # the lists, and with them the frames, stay alive
    # YUV: per-frame pitched surfaces, the geometry of ONE frame in the record
    pool = torch.zeros(4, 150, 160, dtype=torch.uint8)
    nv = TR.FrameList([pool[i, :, :132] for i in (2, 0, 3)])
    b = TR.build_video_batch([nv], _tables((1,), (3,), 8), "NV12", 64, 56, (1,), [8], 3, torch.device("cpu"), lambda t: t, height=98)
    rec = b.sources[0]
    assert (rec.N, rec.Hs, rec.Ws, rec.y_pitch, rec.c_pitch, rec.frame_stride) == (3, 98, 132, 160, 160, 150 * 160)
    assert (rec.u_offset, rec.v_offset) == (100 * 160, 100 * 160 + 1)
    assert b.frame_ptrs.tolist() == [pool[i].data_ptr() for i in (2, 0, 3)]


def test_video_batch_refuses_a_mix_and_bad_frame_lists():
    cpu = torch.device("cpu")
    video = torch.zeros((12, 97, 131, 3), dtype=torch.uint8)
    frames = TR.FrameList(video.unbind(0))
    tables = _tables((2, 2), (12, 12), 4)

    def build(vs, ts=tables, layout="NTHWC", device=cpu, crop=56):
        return TR.build_video_batch(vs, ts, layout, 64, crop, (0, 1, 2), [4], 3, device, lambda t: t)

    assert build([frames, frames]).total == 12
    for mix in ([video, frames], [frames, video]):
        with pytest.raises(ValueError, match="tensors.*FrameLists"):
            build(mix)
    with pytest.raises(RuntimeError, match="is on cpu"):
        build([frames, frames], device=torch.device("cuda", 0))
    with pytest.raises(RuntimeError, match="crop does not fit"):
        build([frames, frames], crop=65)
    with pytest.raises(ValueError, match="leave the video"):
        build([frames, TR.FrameList(video[:5].unbind(0))])        # entries past ITS frame count
    with pytest.raises(RuntimeError, match="one dtype"):
        build([TR.FrameList([torch.zeros(3, 97, 131, dtype=torch.uint8)]), TR.FrameList([torch.zeros(3, 97, 131)])],
              _tables((2, 2), (1, 1), 4), layout="NCTHW")
    with pytest.raises(RuntimeError):
        build([frames, frames], layout="NV12")                   # frames of another form


def test_the_one_tensor_entries_refuse_a_frame_list_and_name_video_batch():
    frames = TR.FrameList([torch.zeros(4, 6, 3, dtype=torch.uint8)])
    for what in ("fill_video", "a clip-at-a-time call"):
        with pytest.raises(RuntimeError, match="video_batch"):
            TR._refuse_frames(frames, what)
    TR._refuse_frames(torch.zeros(1), "fill_video")


# ----------------------------------------------------------------------------- streams
def _rows(windows, clip_frames):
    return [(first + TR.temporal_indices(stop - first, clip_frames)).tolist() for _, _, first, stop in windows]


@pytest.mark.parametrize("fps,d,stride,n,t", [(10, Fraction(8, 10), Fraction(3, 10), n, 4) for n in (8, 14, 21, 23, 24)]
                         + [(Fraction(30000, 1001), Fraction(32, 30), Fraction(16, 30), 100, 16)])
def test_stream_windows_are_the_clips_of_the_uniform_sampler(fps, d, stride, n, t):
    table, infos = clip_frame_table(UniformClipSampler(d, stride), n, fps, t)
    windows = stream_windows(d, stride, fps, n, 0)
    assert _rows(windows, t) == table.tolist()
    assert [(k, start) for k, start, _, _ in windows] == [(i.clip_index, i.clip_start_sec) for i in infos]
    # from a later window on: the tail of the same list; a pure function
    assert stream_windows(d, stride, fps, n, 2) == windows[2:] and stream_windows(d, stride, fps, n, 0) == windows
    assert stream_windows(d, stride, fps, n, len(windows)) == []


def test_a_stream_shorter_than_one_clip_emits_nothing():
    d, stride = Fraction(8, 10), Fraction(3, 10)
    for n in range(8):
        assert stream_windows(d, stride, 10, n, 0) == []
    assert len(stream_windows(d, stride, 10, 8, 0)) == 1
    assert len(clip_frame_table(UniformClipSampler(d, stride), 5, 10, 4)[1]) == 1    # where the sampler cuts a short clip
    for bad in (dict(clip_duration=0), dict(stride=0), dict(fps=0), dict(frames_seen=-1), dict(first_window=-1)):
        args = dict(clip_duration=d, stride=stride, fps=10, frames_seen=8, first_window=0)
        args.update(bad)
        with pytest.raises(ValueError):
            stream_windows(**args)


@pytest.mark.parametrize("pushes", [(7, 7, 7, 2), (1,) * 23, (23,), (3, 11, 1, 8), (2,) * 40])
def test_stream_state_emits_every_window_once_and_holds_a_bounded_number_of_frames(pushes):
    """`StreamState` is all of `StreamPredictor`'s bookkeeping: windows completed per push, then the drop."""
    d, stride, fps = Fraction(8, 10), Fraction(3, 10), 10
    st = INF.StreamState(d, stride, fps)
    assert st.bound == 8
    emitted, counts = [], []
    for n in pushes:
        base = st.base
        windows = st.push(n)
        for k, start, first, stop in windows:
            assert base <= first < stop <= st.seen               # every frame of an emitted window is still held
        emitted.extend(windows)
        counts.append(len(windows))
        dropped = st.drop()
        assert st.base == base + dropped and st.held == st.seen - st.base
        assert st.held <= st.bound + n, (n, st.held)
        # nothing the next window needs is gone
        assert st.base <= -(-fps * st.next_window * stride // 1)
    assert emitted == stream_windows(d, stride, fps, sum(pushes), 0)
    if pushes == (7, 7, 7, 2):
        assert counts == [0, 3, 2, 1]
    # a stream of a million frames: numbers stay exact Python ints
    st = INF.StreamState(Fraction(32, 30), Fraction(16, 30), Fraction(30000, 1001))
    st.push(10 ** 6)
    st.drop()
    assert st.held <= st.bound + 16 and isinstance(st.base, int)


def test_stream_predictor_takes_a_classification_form_only():
    class Detection:
        _pv_load_boxes = staticmethod(lambda b: None)

    with pytest.raises(ValueError, match="classification"):
        INF.StreamPredictor(Detection(), Fraction(8, 10), Fraction(3, 10), 10, None, None, False, 64, 56)
