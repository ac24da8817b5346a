"""Many videos per forward, without a GPU: the descriptor of `pv_batch_views` (include/pv_mi355x.h) -- exported, versioned,
mirrored by ctypes, validated before any launch --, the code-object metadata of its kernels (pytorchvideo_amd/csrc/
pv_batch.hip), and the host logic of `DevicePacker.video_batch`: the item sequence, the concatenated frame tables and the
chunking."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

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
    2 frames of 2 x W and 3 frames of 6 x W scaled to 3 x W, W = 40000 --, a table of 3 rows, 4 items of 1 x W, one view.
    RGB planar uint8, or NV12.  The limit is checked last, so this base returns PV_ERR_UNSUPPORTED -- the positive control of
    every PV_ERR_INVALID case below -- and nothing here is ever launched, on a machine with a GPU or without."""
    src, dst, tab, mat = (C.c_uint8 * 512)(), (C.c_uint8 * 256)(), (C.c_int32 * 8)(), (C.c_float * 12)()
    sources, items = (L.ViewSource * 2)(), (L.ViewItem * 4)()
    keep.extend([src, dst, tab, mat, sources, items])
    base = C.addressof(src) + (-C.addressof(src)) % 16
    _record(sources[0], base, 2, 2, W, 2, W)
    _record(sources[1], base + 64, 3, 6, W, 3, W)
    for i, (s, r) in enumerate(((1, 2), (0, 0), (1, 1), (0, 0))):
        items[i].source, items[i].row, items[i].view = s, r, 0
    d = L.BatchViewsDesc()
    d.sources = d.sources_dev = C.addressof(sources)
    d.items = d.items_dev = C.addressof(items)
    d.t_index, d.dst = C.addressof(tab), C.addressof(dst) + (-C.addressof(dst)) % 16
    d.n_sources, d.n_items, d.n_rows, d.t_stride, d.C, d.T = 2, 4, 3, 1, 3, 1
    d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NCTHW
    d.Ho, d.Wo, d.n_views = 1, W, 1
    d.dst_layout, d.dst_dtype = L.DST_NCTHW, L.PV_BF16
    if yuv:
        d.src_layout, d.c_step, d.yuv2rgb = L.SRC_YUV420, 2, C.addressof(mat)
        sources[0].src += 1                              # nothing needs alignment
        for rec, (hs, ws) in zip(sources, ((2, W), (6, W))):
            rec.y_pitch = rec.c_pitch = ws
            rec.u_offset, rec.v_offset, rec.frame_stride = hs * ws, hs * ws + 1, hs * ws * 3 // 2
    return d, sources, items


def _status(d):
    return L.lib().pv_batch_views(C.byref(d), None)


def _bad(keep, yuv=False, **fields):
    d, _, _ = _desc(keep, yuv)
    for k, v in fields.items():
        setattr(d, k, v)
    return _status(d)


def _bad_record(keep, index, yuv=False, **fields):
    d, sources, _ = _desc(keep, yuv)
    for k, v in fields.items():
        setattr(sources[index], k, v)
    return _status(d)


def test_batch_views_is_exported_and_versioned(pv_lib):
    assert "pv_batch_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_batch_views")
    assert pv_lib.pv_version() == L.ABI_VERSION == 36            # additive: no descriptor changed
    assert L.SRC_YUV420 == 2 and (L.SRC_NCTHW, L.SRC_NTHWC) == (0, 1)


def test_ctypes_mirrors_have_the_size_of_the_c_structs(tmp_path):
    cc = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang")
    cc = next((c for c in (cc, "/opt/rocm/lib/llvm/bin/clang", "/usr/bin/cc", "/usr/bin/gcc") if os.path.exists(c)), None)
    assert cc is not None, "no C compiler beside hipcc"
    assert C.sizeof(L.ViewSource) == 96 and C.sizeof(L.ViewItem) == 16
    src = tmp_path / "size.c"
    text = ('#include "pv_mi355x.h"\n_Static_assert(sizeof(pv_view_source) == %d, "size");\n'
            '_Static_assert(sizeof(pv_view_item) == %d, "size");\n_Static_assert(sizeof(pv_batch_views_desc) == %d, "size");\n'
            '_Static_assert(PV_SRC_YUV420 == 2, "value");\n')
    cmd = [cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)]
    sizes = [C.sizeof(L.ViewSource), C.sizeof(L.ViewItem), C.sizeof(L.BatchViewsDesc)]
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
        d, _, _ = _desc(keep, yuv)
        assert _status(d) == UNS, yuv


def test_batch_views_rejects_invalid_launch_fields(pv_lib):
    keep = []
    assert pv_lib.pv_batch_views(None, None) == INV
    assert _status(L.BatchViewsDesc()) == INV
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
    # whatever pv_resample_crop rejects
    assert _bad(keep, C=5) == INV
    assert _bad(keep, C=0) == INV
    for nv in (0, 4, -1):
        assert _bad(keep, n_views=nv) == INV, nv
    for dtype, ch in ((L.PV_F32, 3), (L.PV_U8, 4)):              # an interleaved video is uint8 with 3 channels
        assert _bad(keep, src_layout=L.SRC_NTHWC, src_dtype=dtype, C=ch) == INV
    assert _bad(keep, src_layout=3) == INV
    assert _bad(keep, Ho=0) == INV
    assert _bad(keep, Wo=-1) == INV
    d, _, _ = _desc(keep)                                        # misaligned channels-last destination
    d.dst_layout, d.c_p, d.ld, d.bs = L.DST_NDHWC, 8, 8, 8
    d.dst += 2
    assert _status(d) == INV
    assert _bad(keep, dst_layout=L.DST_NDHWC, c_p=8, ld=8, bs=4) == INV      # items overlap
    d, _, _ = _desc(keep)
    d.dst += 1                                                   # a bf16 destination at an odd address
    assert _status(d) == INV
    # YUV launches: three channels, a chroma step of 1 or 2
    assert _bad(keep, yuv=True, C=4) == INV
    for step in (0, 3, -1):
        assert _bad(keep, yuv=True, c_step=step) == INV, step


def test_batch_views_rejects_invalid_records(pv_lib):
    keep = []
    for index in (0, 1):
        assert _bad_record(keep, index, src=None) == INV
        for field in ("N", "Hs", "Ws", "Hn", "Wn"):
            for val in (0, -3):
                assert _bad_record(keep, index, **{field: val}) == INV, (index, field, val)
    # sy / sx are the library's own division, bit for bit: one ulp off is refused
    for field in ("sy", "sx"):
        for index in (0, 1):
            d, sources, _ = _desc(keep)
            good = getattr(sources[index], field)
            bits = C.c_uint32.from_buffer_copy(C.c_float(good)).value
            for off in (1, -1):
                setattr(sources[index], field, C.c_float.from_buffer_copy(C.c_uint32(bits + off)).value)
                assert _status(d) == INV, (field, index, off)
            setattr(sources[index], field, good)
            assert _status(d) == UNS
    # a window one pixel outside Hn x Wn of the SECOND source only: source 1 is 3 x W after scaling, the window 1 x W
    for field, val in (("y_off", 3), ("x_off", 1), ("y_off", -1), ("x_off", -1)):
        d, sources, _ = _desc(keep)
        getattr(sources[1], field)[0] = val
        assert _status(d) == INV, (field, val)
        getattr(sources[1], field)[0] = val - 1 if val > 0 else 0   # the last pixel inside
        assert _status(d) == UNS, (field, val)
    d, sources, _ = _desc(keep)
    sources[0].y_off[0] = 2                                      # legal in source 1 (3 rows), not in source 0 (2 rows)
    assert _status(d) == INV
    d, sources, _ = _desc(keep)
    d.Ho = 3                                                     # fits source 1, leaves source 0
    assert _status(d) == INV
    d, sources, _ = _desc(keep)
    d.src_dtype = L.PV_F32                                       # an fp32 source at an address that is no multiple of 4
    assert _status(d) == UNS
    sources[1].src += 2
    assert _status(d) == INV


def test_batch_views_rejects_invalid_items(pv_lib):
    keep = []
    for field, bad in (("source", 2), ("source", -1), ("row", 3), ("row", -1), ("view", 1), ("view", -1)):
        for index in (0, 3):
            d, _, items = _desc(keep)
            setattr(items[index], field, bad)
            assert _status(d) == INV, (field, bad, index)
    d, _, items = _desc(keep)
    d.n_items = 3
    items[3].source = 9                                          # behind the window: never read
    assert _status(d) == UNS


def test_batch_views_rejects_invalid_yuv_planes_per_source(pv_lib):
    keep = []
    # source 1 is 6 x W NV12: y_pitch W, chroma at 6 W / 6 W + 1, frames of 9 W bytes
    assert _bad_record(keep, 1, yuv=True, Hs=5, Hn=5, sy=1.0) == INV                 # odd height
    assert _bad_record(keep, 1, yuv=True, Ws=W + 1, Wn=W + 1, sx=1.0) == INV         # odd width
    assert _bad_record(keep, 1, yuv=True, y_pitch=W - 1) == INV                      # y_pitch < Ws
    assert _bad_record(keep, 1, yuv=True, c_pitch=W - 1) == INV                      # c_pitch < (Ws/2) * c_step
    assert _bad_record(keep, 1, yuv=True, frame_stride=0) == INV
    assert _bad_record(keep, 1, yuv=True, frame_stride=6 * W - 1) == INV             # the luma plane leaves the frame
    assert _bad_record(keep, 1, yuv=True, frame_stride=9 * W - 1) == INV             # the last V sample at byte 9 W - 1
    assert _bad_record(keep, 1, yuv=True, u_offset=-1, v_offset=0) == INV
    assert _bad_record(keep, 1, yuv=True, u_offset=6 * W, v_offset=6 * W + 2) == INV # an interleaved plane holds U and V side by side
    assert _bad_record(keep, 1, yuv=True, u_offset=6 * W, v_offset=6 * W) == INV
    assert _bad_record(keep, 0, yuv=True, frame_stride=5) == INV                     # the first source is checked as well
    assert _bad_record(keep, 1, yuv=True, u_offset=6 * W + 1, v_offset=6 * W) == UNS # NV21 beside NV12 in one launch
    # planar chroma (c_step 1): I420 and YV12 side by side, and a V plane behind the frame
    d, sources, _ = _desc(keep, yuv=True)
    d.c_step = 1
    for rec, (hs, ws) in zip(sources, ((2, W), (6, W))):
        rec.c_pitch = ws // 2
        rec.u_offset, rec.v_offset = hs * ws, hs * ws + (hs // 2) * (ws // 2)
    sources[1].u_offset, sources[1].v_offset = sources[1].v_offset, sources[1].u_offset
    assert _status(d) == UNS
    sources[1].u_offset += 1
    assert _status(d) == INV


def test_batch_views_reports_unsupported_forms(pv_lib):
    keep = []
    assert _bad(keep, src_dtype=L.PV_BF16) == UNS
    assert _bad(keep, yuv=True, src_dtype=L.PV_F32) == UNS
    assert _bad(keep, dst_dtype=L.PV_U8) == UNS
    assert _bad(keep, dst_layout=L.DST_NDHWC, dst_dtype=L.PV_F32, c_p=4, ld=4, bs=4) == UNS
    assert _bad(keep, dst_layout=L.DST_NDHWC, c_p=6, ld=8, bs=8) == UNS
    assert _bad(keep, dst_layout=7) == UNS
    # a staged strip beyond the LDS limit: one output row of W columns of three uint8 planes needs 2 * 3 * (W + 15) bytes
    d, _, _ = _desc(keep)
    assert _status(d) == UNS


# ----------------------------------------------------------------------------- code object metadata
@pytest.fixture(scope="module")
def batch_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("isa_batch") / "pv_batch.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_batch.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_every_batch_instantiation_is_free_of_scratch_and_spills(batch_asm):
    """The per-item record is read through a pointer, field by field, and the view is selected, never indexed: 3 source forms
    x 5 destination forms of the RGB / planar kernel with no private segment, no spilled register and at most 72 VGPRs
    (seven waves per SIMD, the bar of resample_crop_kernel); 2 chroma forms x 5 of the YUV kernel with no private segment and
    no spill, their VGPR counts printed (DESIGN.md 4.6 records them; pv_yuv_views' are not gated either)."""
    kernels = re.findall(r"\.name:\s+(\S*batch_(?:views|yuv)_kernel\S*)\n(.*?)\.wavefront_size", batch_asm, re.S)
    rgb = [k for k in kernels if "batch_views_kernel" in k[0]]
    yuv = [k for k in kernels if "batch_yuv_kernel" in k[0]]
    assert len(rgb) == 15 and len(yuv) == 10, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
        if "batch_views_kernel" in name:
            assert meta["vgpr_count"] <= 72, (name, meta["vgpr_count"])
    # the one-source kernels keep their names to themselves: the patterns of their own code-shape tests match nothing here
    assert "resample_crop_kernel" not in batch_asm and "yuv_views_kernel" not in batch_asm


# ----------------------------------------------------------------------------- host logic of video_batch
def _tables(counts, frames, t):
    """Per video a [n_clips, t] table whose entries name frames of THAT video (the last entry of every table is its last frame)."""
    out = []
    for j, (c, n) in enumerate(zip(counts, frames)):
        tab = (torch.arange(c * t).view(c, t) * 3 + j) % n
        tab[-1, -1] = n - 1
        out.append(tab.to(torch.int32))
    return out


def test_item_sequence_is_video_major_then_clip_then_view():
    items, video_of, clip_of, row0 = TR.batch_items([4, 1, 3], 3)
    assert items.dtype == torch.int32 and tuple(items.shape) == (24, 4)
    want = [(j, r0 + c, v, 0) for j, (n, r0) in enumerate(zip((4, 1, 3), (0, 4, 5))) for c in range(n) for v in range(3)]
    assert [tuple(r) for r in items.tolist()] == want
    assert row0 == [0, 4, 5]
    assert video_of.tolist() == [0] * 12 + [1] * 3 + [2] * 9 and video_of.dtype == torch.int32
    assert clip_of.tolist() == [r for r in range(8) for _ in range(3)] and clip_of.dtype == torch.int32
    # batch 6: 24 items = 4 forwards, none of them short; 25 would add a short one
    assert TR.batch_chunks(24, 6) == [(0, 6), (6, 6), (12, 6), (18, 6)]
    assert TR.batch_chunks(25, 6)[-1] == (24, 1) and TR.batch_chunks(5, 6) == [(0, 5)]
    for bad in ([], [2, 0], [1, -1]):
        with pytest.raises(ValueError):
            TR.batch_items(bad, 3)


def test_video_batch_builds_records_items_and_concatenated_tables_on_the_host():
    """`build_video_batch` -- everything `DevicePacker.video_batch` does -- on plain tensors, the upload stubbed out: three
    NTHWC videos of 4, 1 and 3 clips x 3 views for a two-pathway (4, 1) packer of 2 + 8 frames."""
    frames, sizes, counts = (12, 9, 5), ((97, 131), (131, 97), (40, 53)), (4, 1, 3)
    videos = [torch.zeros((n, h, w, 3), dtype=torch.uint8) for n, (h, w) in zip(frames, sizes)]
    tables = _tables(counts, frames, 8)
    uploads = []

    def upload(t):
        uploads.append(t)
        return t

    b = TR.build_video_batch(videos, tables, "NTHWC", 64, 56, (0, 1, 2), [2, 8], 3, torch.device("cpu"), upload)
    assert len(uploads) == 6                                     # records, items, two tables, video_of, clip_of: once each
    assert b.total == 24 and b.n_rows == 8 and b.clips == [4, 1, 3] and b.row0 == [0, 4, 5] and b.n_views == 3
    assert b.src_dtype == L.PV_U8 and all(v is w for v, w in zip(b.videos, videos))
    # the item sequence, as the C struct holds it and as the device copy holds it
    seq, video_of, clip_of, _ = TR.batch_items(counts, 3)
    assert [(i.source, i.row, i.view, i.reserved) for i in b.items] == [tuple(r) for r in seq.tolist()]
    assert torch.equal(b.items_dev.view(torch.int32).view(-1, 4), seq)
    assert torch.equal(b.video_of, video_of) and torch.equal(b.clip_of, clip_of)
    assert bytes(b.sources_dev.numpy().tobytes()) == bytes(b.sources)        # the very buffer that is passed
    # the concatenated tables: fast = the tables one after another, slow = its columns temporal_indices(8, 2); the rows of
    # video j start at row0[j]
    slow, fast = b.tables
    assert fast.dtype == slow.dtype == torch.int32 and tuple(fast.shape) == (8, 8) and tuple(slow.shape) == (8, 2)
    assert torch.equal(fast, torch.cat(tables)) and torch.equal(slow, fast[:, TR.temporal_indices(8, 2)])
    for j, r0 in enumerate(b.row0):
        assert torch.equal(fast[r0:r0 + counts[j]], tables[j])
    # the records: geometry of every video by the host mirrors, sy / sx the fp32 quotient
    for rec, video, (h, w), n in zip(b.sources, videos, sizes, frames):
        hn, wn = TR.scaled_size(h, w, 64)
        assert (rec.src, rec.N, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (video.data_ptr(), n, h, w, hn, wn)
        assert [(rec.y_off[k], rec.x_off[k]) for k in range(3)] == [TR.crop_offsets(hn, wn, 56, v) for v in (0, 1, 2)]
        assert rec.sy == _f32(h, hn) and rec.sx == _f32(w, wn)


def test_video_batch_refuses_bad_videos_and_tables_on_the_host():
    cpu = torch.device("cpu")
    videos = [torch.zeros((12, 97, 131, 3), dtype=torch.uint8), torch.zeros((5, 40, 53, 3), dtype=torch.uint8)]
    tables = _tables((2, 2), (12, 5), 4)

    def build(vs, ts, layout="NTHWC", device=cpu, crop=56, **kw):
        return TR.build_video_batch(vs, ts, layout, 64, crop, (0, 1, 2), [4], 3, device, lambda t: t, **kw)

    assert build(videos, tables).total == 12
    with pytest.raises(RuntimeError, match="is on cpu"):
        build(videos, tables, device=torch.device("cuda", 0))    # the deploy form is elsewhere
    with pytest.raises(RuntimeError, match="crop does not fit"):
        build(videos, tables, crop=65)
    # an entry outside ITS video, though inside the longer neighbour
    bad = [tables[0], tables[1].clone()]
    bad[1][0, 0] = 7
    with pytest.raises(ValueError, match="leave the video"):
        build(videos, bad)
    assert build(videos, [bad[1], tables[1]]).total == 12         # frame 7 exists in the 12-frame video
    with pytest.raises(ValueError):
        build(videos, tables[:1])
    with pytest.raises(ValueError):
        build(videos, [tables[0], tables[1][:, :3]])             # tables of one batch have one row length
    with pytest.raises(RuntimeError, match="contiguous"):
        build([videos[0].transpose(1, 2), videos[1]], tables)
    with pytest.raises(RuntimeError, match="one dtype"):
        build([videos[0].permute(3, 0, 1, 2).contiguous(), videos[1].permute(3, 0, 1, 2).float().contiguous()], tables, layout="NCTHW")
    with pytest.raises(RuntimeError):
        build([videos[0][..., :2].contiguous(), videos[1]], tables)          # two channels
    with pytest.raises(RuntimeError):
        build([videos[0][0], videos[1]], tables)                             # not a video
    # YUV: geometry per video, heights one per video
    nv = [torch.zeros((4, 150, 132), dtype=torch.uint8), torch.zeros((3, 96, 64), dtype=torch.uint8)]
    tabs = _tables((1, 2), (4, 3), 4)
    b = build(nv, tabs, layout="NV12", height=[98, None])
    assert (b.sources[0].Hs, b.sources[0].u_offset, b.sources[0].v_offset) == (98, 100 * 132, 100 * 132 + 1)
    assert (b.sources[1].Hs, b.sources[1].Ws, b.sources[1].frame_stride) == (64, 64, 96 * 64)
    with pytest.raises(ValueError):
        build(nv, tabs, layout="NV12", height=[98])
    with pytest.raises(RuntimeError):
        build(nv, tabs, layout="NV12", height=99)                            # odd display height
