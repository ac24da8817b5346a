"""Rotated and mirrored videos read in place, without a GPU: the orientation rule of include/pv_mi355x.h (`pv_view_source.orient`,
the field that was `reserved`), the library's validation of oriented records before any launch, the host mirrors
(`transforms.orientation_code`, `oriented`, `orient_boxes`, `boxes_to_view(..., orientation=)`) and the records
`build_video_batch` builds for videos with a code each."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch

import orient_util as OU
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR
from test_batch_views import _desc, _f32, _status

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIX = json.load(open(os.path.join(HERE, "golden", "orient_boxes.json")))
INV, UNS = L.PV_ERR_INVALID, L.PV_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- the ABI is the one it was
def test_the_abi_is_unchanged_and_orient_lies_where_reserved_lay(pv_lib):
    assert pv_lib.pv_version() == L.ABI_VERSION == 36
    assert C.sizeof(L.ViewSource) == 96 and L.ViewSource.reserved.offset == 92 and L.ViewSource.reserved.size == 4
    rec = L.ViewSource()
    assert rec.orient == 0 and rec.reserved == 0
    rec.orient = 5
    assert rec.reserved == 5 and rec.orient == 5
    rec.reserved = 2
    assert rec.orient == 2


# ----------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("orient", OU.CODES)
def test_the_index_formulas_are_rot90_then_flip(orient):
    """D(y, x) of the header's table on a 4 x 6 frame = torch.rot90(S, -rot, (h, w)), then .flip(w) for the mirror bit, which
    is also what `transforms.oriented` returns -- over any pair of dimensions."""
    s = torch.arange(24, dtype=torch.int32).view(4, 6)
    want = OU.by_index(s, orient)
    assert tuple(want.shape) == OU.displayed_size(4, 6, orient) == TR.displayed_size(4, 6, orient)
    ref = torch.rot90(s, -(orient & 3), (0, 1))
    ref = ref.flip(1) if orient & 4 else ref
    assert torch.equal(want, ref) and torch.equal(want, OU.turned(s, orient)) and torch.equal(want, TR.oriented(s, orient))
    video = torch.arange(2 * 4 * 6 * 3, dtype=torch.int32).view(2, 4, 6, 3)                    # NTHWC
    got = TR.oriented(video, orient, 1, 2)
    for n in range(2):
        for c in range(3):
            assert torch.equal(got[n, :, :, c], OU.by_index(video[n, :, :, c], orient))
    if orient:
        assert not torch.equal(want.reshape(-1), s.reshape(-1))


@pytest.mark.parametrize("orient", OU.CODES)
def test_chroma_then_orient_equals_orient_then_chroma(orient):
    """4:2:0 chroma of displayed pixel (y, x) = the chroma sample of the stored pixel it shows; with even sizes that is the
    chroma plane oriented on its own and replicated."""
    g = torch.Generator().manual_seed(40 + orient)
    u = torch.randint(0, 256, (3, 5), generator=g, dtype=torch.int32)                           # of a 6 x 10 frame
    through_the_map = OU.by_index(OU.upsampled(u), orient)
    assert torch.equal(through_the_map, OU.upsampled(OU.by_index(u, orient)))
    assert torch.equal(through_the_map, OU.upsampled(OU.turned(u, orient)))


def test_orientation_code():
    assert [TR.orientation_code(r) for r in (0, 90, 180, 270)] == [0, 1, 2, 3]
    assert [TR.orientation_code(r, True) for r in (0, 90, 180, 270)] == [4, 5, 6, 7]
    assert TR.orientation_code() == 0 and TR.orientation_code(mirror=True) == 4
    for bad in (45, 360, -90, 1, None, "90", True):
        with pytest.raises(ValueError):
            TR.orientation_code(bad)
    for bad in (8, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            TR.oriented(torch.zeros(2, 2), bad)


# ----------------------------------------------------------------------------- validation, before any launch
def _oriented_base(keep):
    """The base of tests/test_batch_views.py (it passes every check but the LDS limit of its 40000-column strips) with source 0
    replaced by a valid TRANSPOSING record: stored 6 x 4, code 1 -> displayed 4 x 6, scaled to 2 x 3, a 1 x 3 window.  The
    launch is mixed: items 1 and 3 name it, items 0 and 2 the upright 6 x W source."""
    d, sources, items = _desc(keep)
    d.Wo = 3
    rec = sources[0]
    rec.Hs, rec.Ws, rec.Hn, rec.Wn, rec.orient = 6, 4, 2, 3, 1
    rec.sy, rec.sx = _f32(4, 2), _f32(6, 3)
    up = sources[1]                                              # upright, far wider than the limit: 3 of 40000 scaled columns
    up.Hn, up.Wn, up.sy, up.sx = 3, 3, _f32(6, 3), _f32(40000, 3)
    return d, sources, items


def test_a_valid_mixed_launch_passes_validation(pv_lib):
    """Every check passes; what stops the call short of the first HIP call is the LDS limit, checked last: the upright items'
    strip spans 26000 columns of three planes."""
    keep = []
    d, sources, _ = _oriented_base(keep)
    assert _status(d) == UNS
    for code in range(8):                                        # every code is valid with the sizes that belong to it
        d, sources, _ = _oriented_base(keep)
        hd, wd = OU.displayed_size(6, 4, code)
        sources[0].orient, sources[0].Hn, sources[0].Wn = code, 2, 3
        sources[0].sy, sources[0].sx = _f32(hd, 2), _f32(wd, 3)
        assert _status(d) == UNS, code


def test_orient_outside_0_to_7_is_invalid(pv_lib):
    keep = []
    for code in (8, -1, 16, 255):
        d, sources, _ = _oriented_base(keep)
        sources[0].orient = code
        assert _status(d) == INV, code


def test_a_transposing_record_divides_the_displayed_size(pv_lib):
    keep = []
    d, sources, _ = _oriented_base(keep)
    sources[0].sy, sources[0].sx = _f32(6, 2), _f32(4, 3)       # the stored size divided: not the displayed quotient
    assert _status(d) == INV
    d, sources, _ = _oriented_base(keep)
    sources[0].orient = 2                                        # the same numbers ARE valid for a half turn: 6 x 4 stays 6 x 4
    sources[0].sy, sources[0].sx = _f32(6, 2), _f32(4, 3)
    assert _status(d) == UNS
    d, sources, _ = _oriented_base(keep)
    sources[0].orient = 0                                        # and an upright record must not carry the turned quotient
    assert _status(d) == INV


def test_a_window_must_fit_the_turned_frame(pv_lib):
    """A 3 x 2 window in a frame scaled to 3 x 2: fine while the 6 x 4 frame lies as stored, but turned it is 4 x 6 -> 2 x 3 and
    the window leaves it."""
    keep = []

    def case(code, hn, wn):
        d, sources, _ = _oriented_base(keep)
        d.Ho, d.Wo = 3, 2
        hd, wd = OU.displayed_size(6, 4, code)
        sources[0].orient, sources[0].Hn, sources[0].Wn = code, hn, wn
        sources[0].sy, sources[0].sx = _f32(hd, hn), _f32(wd, wn)
        sources[1].Hn, sources[1].Wn, sources[1].sy, sources[1].sx = 3, 2, _f32(6, 3), _f32(40000, 2)
        return _status(d)

    assert case(0, 3, 2) == UNS and case(2, 3, 2) == UNS         # not turned: the window is the whole scaled frame
    assert case(1, 2, 3) == INV and case(3, 2, 3) == INV and case(5, 2, 3) == INV


def test_a_tile_footprint_beyond_the_lds_limit_is_unsupported(pv_lib):
    """Only oriented items: a 40000 x 40000 stored frame scaled to 8 x 8 -- one output row or column spans 5000 source pixels,
    the smallest tile's footprint is far beyond 64 KiB."""
    keep = []
    d, sources, items = _desc(keep)
    d.Ho = d.Wo = 8
    for rec in sources:
        rec.Hs, rec.Ws, rec.Hn, rec.Wn, rec.orient = 40000, 40000, 8, 8, 3
        rec.sy = rec.sx = _f32(40000, 8)
    assert _status(d) == UNS
    sources[1].orient = 9
    assert _status(d) == INV


# ----------------------------------------------------------------------------- code object metadata
def test_every_tile_kernel_is_free_of_scratch_and_spills(tmp_path):
    """3 RGB / planar source forms and 2 chroma forms x 2 sample widths, x 5 destination forms: no private segment and no
    spilled register.  The register counts are printed (profiles/r17/orient_isa_vs_parent.md records them); not gated."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    path = str(tmp_path / "pv_orient.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", path,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", "pv_orient.hip")], stderr=subprocess.DEVNULL)
    kernels = re.findall(r"\.name:\s+(\S*orient_\w+_kernel\S*)\n(.*?)\.wavefront_size", open(path).read(), re.S)
    assert len(kernels) == 35 and sum("orient_yuv_kernel" in k for k, _ in kernels) == 20, [k for k, _ in kernels]
    for name, body in kernels:
        meta = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        print("%s: %d VGPRs, %d SGPRs" % (name, meta["vgpr_count"], meta["sgpr_count"]))
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name


# ----------------------------------------------------------------------------- boxes
def _t(rows):
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: "%dx%d" % (c["height"], c["width"]))
def test_code_4_is_the_reference_horizontal_flip_with_boxes(case):
    h, w, boxes = case["height"], case["width"], _t(case["boxes"])
    before = boxes.clone()
    assert torch.equal(TR.orient_boxes(boxes, h, w, 4), _t(case["flipped"]))
    assert torch.equal(boxes, before)                            # the input is not modified
    for view in case["views"]:
        got = TR.boxes_to_view(boxes, h, w, case["short_side"], case["crop_size"], view["spatial_idx"], orientation=4)
        assert torch.equal(got, _t(view["expected"])), view["spatial_idx"]
    assert torch.equal(TR.orient_boxes(boxes, h, w, 0), boxes)


def test_codes_1_and_7_by_hand():
    """A 40 x 100 stored frame (H x W), one box (x1, y1, x2, y2) = (10, 4, 30, 9).
    Code 1, a quarter turn clockwise, D is 100 x 40: the stored top-left corner goes to the top-RIGHT.  A point (x, y) lands at
    (Hs-1-y, x): (10, 4) -> (35, 10), (30, 9) -> (30, 30); re-ordered: (30, 10, 35, 30).
    Code 7 = three quarter turns, then mirrored: (x, y) -> (y, Ws-1-x), then x -> Wd-1-x with Wd = 40:
    (10, 4) -> (4, 89) -> (35, 89); (30, 9) -> (9, 69) -> (30, 69); re-ordered: (30, 69, 35, 89)."""
    box = _t([[10, 4, 30, 9]])
    assert TR.orient_boxes(box, 40, 100, 1).tolist() == [[30, 10, 35, 30]]
    assert TR.orient_boxes(box, 40, 100, 7).tolist() == [[30, 69, 35, 89]]
    # the same through the pixels: a frame that is 1 inside the box lights up exactly the mapped box
    frame = torch.zeros(40, 100)
    frame[4:10, 10:31] = 1
    for code in OU.CODES:
        x1, y1, x2, y2 = (int(v) for v in TR.orient_boxes(box, 40, 100, code)[0])
        shown = TR.oriented(frame, code)
        assert shown.sum() == 6 * 21 and bool(shown[y1:y2 + 1, x1:x2 + 1].all()), code
    # boxes_to_view: displayed 100 x 40 scales by 2 to 200 x 80 (short side 80), the centre 80 x 80 crop starts at y = 60
    got = TR.boxes_to_view(box, 40, 100, 80, 80, 1, orientation=1)
    assert got.tolist() == [[60, 0, 70, 0]]
    got = TR.boxes_to_view(box, 40, 100, 80, 80, 1, orientation=7)
    assert got.tolist() == [[60, 78, 70, 79]]                    # y: 138 - 60 = 78, and 178 - 60 clipped to 79
    with pytest.raises(ValueError):
        TR.orient_boxes(box, 40, 100, 8)


# ----------------------------------------------------------------------------- records
def _upload(t):
    return t


def test_build_video_batch_carries_a_code_per_video():
    cpu = torch.device("cpu")
    videos = [torch.zeros((5, 40, 100, 3), dtype=torch.uint8), torch.zeros((4, 60, 50, 3), dtype=torch.uint8),
              torch.zeros((3, 48, 64, 3), dtype=torch.uint8)]
    tables = [torch.zeros((1, 4), dtype=torch.int32)] * 3
    batch = TR.build_video_batch(videos, tables, "NTHWC", 32, 32, (0, 1, 2), [4], 3, cpu, _upload, orientation=[1, 0, 6])
    a, b, c = batch.sources
    assert (a.orient, b.orient, c.orient) == (1, 0, 6) and b.reserved == 0
    assert (a.Hs, a.Ws, b.Hs, b.Ws, c.Hs, c.Ws) == (40, 100, 60, 50, 48, 64)                    # stored sizes
    assert (a.Hn, a.Wn) == TR.scaled_size(100, 40, 32) == (80, 32)                              # displayed 100 x 40
    assert (b.Hn, b.Wn) == TR.scaled_size(60, 50, 32) and (c.Hn, c.Wn) == TR.scaled_size(48, 64, 32)
    assert a.sy == _f32(100, 80) and a.sx == _f32(40, 32)
    assert [(a.y_off[k], a.x_off[k]) for k in range(3)] == [TR.crop_offsets(80, 32, 32, v) for v in (0, 1, 2)]
    # one code for all, any integer type; the default leaves the field as it was built
    same = TR.build_video_batch(videos, tables, "NTHWC", 32, 32, (1,), [4], 3, cpu, _upload, orientation=torch.tensor(5))
    assert [r.orient for r in same.sources] == [5, 5, 5]
    plain = TR.build_video_batch(videos, tables, "NTHWC", 32, 32, (1,), [4], 3, cpu, _upload)
    assert [r.reserved for r in plain.sources] == [0, 0, 0]
    # the library accepts the records as they are (the strips and tiles of these small frames fit, so validation ends at the
    # first HIP call on a machine without a GPU: not called here), and refuses a list of the wrong length or a bad code
    with pytest.raises(ValueError, match="one per video"):
        TR.build_video_batch(videos, tables, "NTHWC", 32, 32, (1,), [4], 3, cpu, _upload, orientation=[1, 2])
    with pytest.raises(ValueError, match="0..7"):
        TR.build_video_batch(videos, tables, "NTHWC", 32, 32, (1,), [4], 3, cpu, _upload, orientation=[1, 2, 8])
    # the crop must fit the DISPLAYED frame scaled: 40 x 100 turned is 100 x 40; no crop: the window is the displayed frame's
    nocrop = TR.build_video_batch(videos[:1], tables[:1], "NTHWC", 32, (80, 32), (1,), [4], 3, cpu, _upload, orientation=3)
    assert (nocrop.sources[0].Hn, nocrop.sources[0].Wn) == (80, 32)
    with pytest.raises(RuntimeError, match="nothing is cropped"):
        TR.build_video_batch(videos[:1], tables[:1], "NTHWC", 32, (80, 32), (1,), [4], 3, cpu, _upload, orientation=2)


def test_frame_lists_and_yuv_videos_take_a_code():
    cpu = torch.device("cpu")
    nv12 = torch.zeros((5, 72, 60), dtype=torch.uint8)           # 48 x 60 frames
    tables = [torch.zeros((1, 4), dtype=torch.int32)]
    batch = TR.build_video_batch([nv12], tables, "NV12", 24, 24, (0, 1, 2), [4], 3, cpu, _upload, orientation=7)
    rec = batch.sources[0]
    assert (rec.orient, rec.Hs, rec.Ws, rec.y_pitch, rec.u_offset) == (7, 48, 60, 60, 48 * 60)
    assert (rec.Hn, rec.Wn) == TR.scaled_size(60, 48, 24) == (30, 24) and rec.sy == _f32(60, 30) and rec.sx == _f32(48, 24)
    frames = TR.FrameList(list(torch.zeros((4, 20, 30, 3), dtype=torch.uint8).unbind(0)))
    fl = TR.build_video_batch([frames], tables, "NTHWC", 16, 16, (1,), [4], 3, cpu, _upload, orientation=1)
    rec = fl.sources[0]
    assert (rec.orient, rec.Hs, rec.Ws, rec.Hn, rec.Wn) == (1, 20, 30, 24, 16) and fl.frame_ptrs.numel() == 4


def test_the_one_source_paths_refuse_an_orientation():
    clip = torch.zeros((1, 3, 4, 20, 30), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="video_batch"):
        TR.device_scale_crop(clip, 16, 16, orientation=1)
    with pytest.raises(ValueError, match="0..7"):
        TR.device_scale_crop(clip, 16, 16, orientation=9)
