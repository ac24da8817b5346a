"""Key-frame action detection over whole videos, the parts that need no GPU: the box mirror `transforms.boxes_to_view` against
the reference's own box transforms (tests/golden/keyframe_boxes.json, written by tests/golden/make_keyframe_golden.py), the
key-frame windows, the chunking of a key-frame sequence into forwards, the host-side validation of `pv_box_views` and the
constructor refusals."""
import ctypes as C
import json
import math
import os
from fractions import Fraction

import pytest
import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import KeyframeDetector, keyframe_chunks

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_boxes.json")))


# ----------------------------------------------------------------------------- the box mirror
def test_fixture_covers_the_cases_that_matter():
    frames = {(c["height"], c["width"], c["crop_size"]) for c in GOLD["cases"]}
    assert {(60, 90, None), (90, 60, None), (53, 53, None), (720, 1280, None), (60, 90, 48), (90, 60, 48)} <= frames
    c = GOLD["cases"][0]                                        # 60 x 90 -> 48 x 72, no crop
    assert (c["height"], c["width"], c["scaled"]) == (60, 90, [48, 72])
    # x2 = 95 is clipped to 89, scaled to 71.2 and clipped again to 71: the second clip fires
    row = [r for r in c["boxes"] if r[2] == 95.0][0]
    i = c["boxes"].index(row)
    assert c["clipped"][i][2] == 89.0 and c["expected"][i][2] == 71.0
    assert 89.0 * (72.0 / 90.0) > 71.0


@pytest.mark.parametrize("i", range(len(GOLD["cases"])))
def test_boxes_to_view_equals_the_reference_bit_for_bit(i):
    c = GOLD["cases"][i]
    boxes = torch.tensor(c["boxes"], dtype=torch.float32)
    keep = boxes.clone()
    got = TR.boxes_to_view(boxes, c["height"], c["width"], c["short_side"], c["crop_size"], c["spatial_idx"], c["clip_to_source"])
    want = torch.tensor(c["expected"], dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(boxes, keep)                            # the input is not modified
    if c["crop_size"] is None:
        assert TR.scaled_size(c["height"], c["width"], c["short_side"]) == tuple(c["scaled"])


def test_boxes_to_view_is_the_composition_of_the_existing_mirrors():
    h, w, size, crop, v = 60, 90, 56, 48, 2
    b = torch.tensor(GOLD["cases"][0]["boxes"], dtype=torch.float32)
    _, scaled = TR.short_side_scale_with_boxes(torch.zeros(1, 1, h, w), b.clone(), size)
    _, want = TR.uniform_crop_with_boxes(torch.zeros(1, 1, *TR.scaled_size(h, w, size)), crop, v, scaled)
    assert torch.equal(TR.boxes_to_view(b, h, w, size, crop, v), want)
    with pytest.raises(RuntimeError, match="does not fit"):
        TR.boxes_to_view(b, h, w, 40, 48, 1)


# ----------------------------------------------------------------------------- key-frame windows
def _rule(t, d, n, fps, frames):
    """The frame rule of clip_frame_table restated for the window [t - d/2, t - d/2 + d)."""
    fps = Fraction(fps)
    start = Fraction(t) - Fraction(d) / 2
    end = min(start + Fraction(d), Fraction(n) / fps)
    first, stop = math.ceil(fps * start), min(math.ceil(fps * end), n)
    return first + TR.temporal_indices(stop - first, frames), first, stop


def test_keyframe_frame_table_follows_the_sampler_and_the_frame_rule():
    for w in GOLD["windows"]:                                  # the reference's TimeStampClipSampler, where it was recorded
        d, t = Fraction(*w["duration"]), Fraction(*w["stamp"])
        info = D.TimeStampClipSampler(D.UniformClipSampler(d))(None, None, {"clip_index": t})
        assert [Fraction(info.clip_start_sec), Fraction(info.clip_end_sec)] == [Fraction(*w["start"]), Fraction(*w["end"])]
        assert [info.clip_index, info.aug_index, info.is_last_clip] == w["tail"]
    info = D.TimeStampClipSampler(D.UniformClipSampler(Fraction(16, 30)))(None, None, {"clip_index": Fraction(3, 2)})
    start = Fraction(3, 2) - Fraction(16, 30) / 2.0             # ava.py:311 halves by a float
    assert (info.clip_start_sec, info.clip_end_sec) == (start, start + Fraction(16, 30))
    assert abs(info.clip_start_sec - 37 / 30) < 1e-12 and abs(info.clip_end_sec - 53 / 30) < 1e-12
    assert (info.clip_index, info.aug_index, info.is_last_clip) == (0, 0, True)
    for n, fps, d, frames, stamps in ((40, 20, Fraction(16, 20), 16, [0.4, 0.7, 1.0, 1.3, 1.6]),
                                      (90, 30, Fraction(16, 30), 8, [Fraction(1), Fraction(3, 2), 0.9, 2.9]),
                                      (25, Fraction(30000, 1001), 0.8, 4, [0.4, 0.5])):
        table, centres = D.keyframe_frame_table(stamps, d, n, fps, frames)
        assert table.dtype == torch.int32 and tuple(table.shape) == (len(stamps), frames) and len(centres) == len(stamps)
        for k, t in enumerate(stamps):
            row, first, stop = _rule(t, d, n, fps, frames)
            assert table[k].tolist() == row.tolist()
            assert centres[k] == list(range(first, stop))[(stop - first) // 2]
        assert int(table.min()) >= 0 and int(table.max()) < n
    # a window that ends past the video is cut, as clip_frame_table cuts it
    table, centres = D.keyframe_frame_table([1.9], 1, 40, 20, 4)
    assert table[0].tolist() == (28 + TR.temporal_indices(12, 4)).tolist() and centres == [34]
    # windows that tile the video are the clips of a UniformClipSampler
    table, _ = D.keyframe_frame_table([0.5, 1.5, 2.5], 1, 60, 20, 8)
    want, _ = D.clip_frame_table(D.UniformClipSampler(1), 60, 20, 8)
    assert torch.equal(table, want)


def test_keyframe_frame_table_errors():
    with pytest.raises(ValueError, match="holds no frame"):
        D.keyframe_frame_table([0.2], 1, 40, 20, 4)           # the window starts before 0
    with pytest.raises(ValueError, match="holds no frame"):
        D.keyframe_frame_table([1.0, 2.5], 1, 40, 20, 4)      # [2, 3) s of a 2 s video: no frame
    with pytest.raises(ValueError, match="holds no frame"):
        D.keyframe_frame_table([5.0], 1, 40, 20, 4)
    with pytest.raises(ValueError):
        D.keyframe_frame_table([], 1, 40, 20, 4)
    with pytest.raises(ValueError):
        D.keyframe_frame_table([1.0], 1, 0, 20, 4)


# ----------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("counts", [[2, 0, 3, 1, 4, 5, 0, 1], [2, 0, 3, 1, 4], [0, 0], [5, 5, 5], [1] * 9, [0, 3]])
@pytest.mark.parametrize("batch,capacity", [(2, 5), (4, 5), (1, 5), (8, 16)])
def test_keyframe_chunks_properties(counts, batch, capacity):
    chunks = keyframe_chunks(counts, batch, capacity)
    flat = [k for c in chunks for k in c]
    assert flat == [k for k, c in enumerate(counts) if c > 0]              # every non-empty key frame once, in order
    for i, c in enumerate(chunks):
        assert 1 <= len(c) <= batch and sum(counts[k] for k in c) <= capacity
        if i + 1 < len(chunks):                                            # closed only because the next would not fit
            nxt = chunks[i + 1][0]
            assert len(c) == batch or sum(counts[k] for k in c) + counts[nxt] > capacity


def test_keyframe_chunks_examples_and_errors():
    assert keyframe_chunks([2, 0, 3, 1, 4], 2, 5) == [[0, 2], [3, 4]]
    assert keyframe_chunks([2, 0, 3, 1, 4, 5, 0, 1], 4, 5) == [[0, 2], [3, 4], [5], [7]]
    assert keyframe_chunks([2, 0, 3, 1, 4, 5, 0, 1], 8, 16) == [[0, 2, 3, 4, 5, 7]]
    assert keyframe_chunks([], 2, 5) == []
    with pytest.raises(ValueError, match="6 boxes"):
        keyframe_chunks([2, 6, 1], 2, 5)
    with pytest.raises(ValueError):
        keyframe_chunks([1], 0, 5)


# ----------------------------------------------------------------------------- the C ABI, without a GPU
def _valid_box_desc():
    d = L.BoxViewsDesc()
    d.boxes = d.box_item = d.sources_dev = d.items_dev = d.dst = 4096          # never dereferenced: validation comes first
    d.n_boxes, d.n_seq, d.n_sources, d.n_views = 10, 4, 2, 1
    d.box0, d.n_launch, d.item0, d.n_items = 2, 5, 1, 2
    d.Ho, d.Wo, d.capacity, d.clip_to_source = 48, 72, 5, 1
    return d


def test_box_views_symbol_binding_and_version(pv_lib):
    assert "pv_box_views" in L.EXPORTED_SYMBOLS and hasattr(pv_lib, "pv_box_views")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pv_mi355x.h")).read()
    assert "int pv_box_views(const pv_box_views_desc* d, pv_stream_t stream);" in header
    assert pv_lib.pv_version() == 36 == L.ABI_VERSION           # additive: no existing descriptor changed
    assert C.sizeof(L.BoxViewsDesc) == 6 * 8 + 12 * 4


@pytest.mark.parametrize("field,value", [
    ("boxes", None), ("box_item", None), ("sources_dev", None), ("items_dev", None), ("dst", None),
    ("capacity", 0), ("capacity", -3), ("n_items", 0), ("n_items", -1), ("Ho", 0), ("Wo", 0), ("Ho", -48), ("Wo", -1),
    ("n_launch", -1), ("n_launch", 6), ("box0", -1), ("box0", 6), ("item0", -1), ("item0", 3), ("n_sources", 0),
    ("n_views", 0), ("n_views", 4)])
def test_box_views_rejects_invalid_descriptors_without_a_gpu(pv_lib, field, value):
    d = _valid_box_desc()
    setattr(d, field, value)
    assert pv_lib.pv_box_views(C.byref(d), None) == L.PV_ERR_INVALID
    assert pv_lib.pv_box_views(None, None) == L.PV_ERR_INVALID


# ----------------------------------------------------------------------------- constructor refusals
class _Ref:
    def __init__(self, B, C, T, H, W):
        self.B, self.C, self.T, self.H, self.W = B, C, T, H, W


class _Sess:
    device = "cpu"


def _fake_detection_form(h, w, capacity=5):
    m = torch.nn.Identity()
    m.__dict__.update(_pv_inputs=_Ref(2, 3, 4, h, w), _pv_session=_Sess(), _pv_load_boxes=lambda b: None,
                      _pv_box_capacity=capacity, _pv_box_ptr=None)
    return m


def test_device_packer_modes_and_refusals():
    dm = _fake_detection_form(48, 72)
    with pytest.raises(ValueError, match="given together"):
        TR.DevicePacker(dm, crop_size=48)
    p = TR.DevicePacker(dm, short_side=48, src_layout="NTHWC", keyframes=True)         # no crop: the tutorial's protocol
    assert p.no_crop and p.window == (48, 72) and p.views == (1,) and p.box_capacity == 5
    with pytest.raises(RuntimeError, match="no-crop mode"):
        p(torch.zeros(2, 4, 60, 90, 3, dtype=torch.uint8), torch.zeros(5, 5))
    with pytest.raises(ValueError, match="crop_size 48 is not the 48 x 72 input"):
        TR.DevicePacker(dm, short_side=56, crop_size=48, src_layout="NTHWC", keyframes=True)
    # YUV frames are legal for a detection form on the key-frame path only
    with pytest.raises(ValueError, match="detection model does not take NV12 frames: its boxes"):
        TR.DevicePacker(dm, short_side=56, crop_size=48, src_layout="NV12")
    with pytest.raises(ValueError, match="given together"):
        TR.DevicePacker(dm, short_side=48, src_layout="NTHWC")                         # no crop is a mode of the key-frame path
    p = TR.DevicePacker(dm, short_side=48, src_layout="NV12", keyframes=True)
    with pytest.raises(ValueError, match="does not take NV12 frames a clip at a time"):
        p(torch.zeros(2, 4, 90, 90, dtype=torch.uint8), torch.zeros(5, 5))
    # without keyframes=True a detection form still takes no videos
    with pytest.raises(RuntimeError, match="boxes of key frames"):
        TR.DevicePacker(_fake_detection_form(48, 48), short_side=56, crop_size=48, src_layout="NTHWC").video_batch([torch.zeros(8, 60, 90, 3, dtype=torch.uint8)], [torch.zeros(1, 4)])
    with pytest.raises(ValueError, match="one view"):
        TR.DevicePacker(_fake_detection_form(48, 48), short_side=56, crop_size=48, spatial_idx=(0, 1), src_layout="NTHWC")


def test_no_crop_batches_name_both_sizes():
    up = lambda t: t
    video = torch.zeros(8, 60, 90, 3, dtype=torch.uint8)
    table = torch.zeros(1, 4, dtype=torch.int32)
    b = TR.build_video_batch([video], [table], "NTHWC", 48, (48, 72), (1,), [4], 3, torch.device("cpu"), up)
    rec = b.sources[0]
    assert (rec.Hn, rec.Wn, rec.y_off[0], rec.x_off[0]) == (48, 72, 0, 0)
    with pytest.raises(RuntimeError, match="60 x 80 frame scales to 48 x 64, the deploy form takes 48 x 72"):
        TR.build_video_batch([video, torch.zeros(8, 60, 80, 3, dtype=torch.uint8)], [table, table], "NTHWC", 48, (48, 72), (1,),
                             [4], 3, torch.device("cpu"), up)


def test_keyframe_detector_refuses_what_it_cannot_score():
    with pytest.raises(ValueError, match="VideoPredictor"):
        KeyframeDetector(torch.nn.Identity(), 1.0, None, None, False, 48)
    cls = torch.nn.Identity()
    cls.__dict__.update(_pv_inputs=_Ref(2, 3, 4, 48, 48), _pv_session=_Sess())
    with pytest.raises(ValueError, match="VideoPredictor"):
        KeyframeDetector(cls, 1.0, None, None, False, 56, 48)
    dm = _fake_detection_form(48, 72)
    with pytest.raises(ValueError, match="short_side"):
        KeyframeDetector(dm, 1.0, None, None, False, None)
    with pytest.raises(ValueError, match="one view"):
        KeyframeDetector(dm, 1.0, None, None, False, 48, None, (0, 1))
    det = KeyframeDetector(dm, 1.0, None, None, False, 48)
    assert det.packer.keyframes and det.packer.no_crop and det.forwards == 0
