"""Record the REAL reference's box transforms of the key-frame detection protocol -> tests/golden/keyframe_boxes.json
(numbers only).  pytorchvideo/transforms/functional.py is loaded by file path, as make_spatial_golden.py loads it:
`clip_boxes_to_image`, `short_side_scale_with_boxes`, `uniform_crop_with_boxes`, chained as the detection tutorial chains
them (clip, scale, clip: no crop) and as the eval pipeline does (scale, crop + clip).  Runs only where the reference tree
exists.

`TimeStampClipSampler.__call__` is recorded too when pytorchvideo/data/ava.py imports under the shim (oracle/ref_shim.py);
it needs iopath and the decoders behind `LabeledVideoDataset`, so where those are missing only the transform cases are
recorded and "windows" is an empty list -- tests/test_keyframe_detection.py then checks the windows against the rule of
`clip_frame_table` alone.

fp32 values are stored as the Python floats they convert to exactly, so the fixture compares bit for bit.

    python tests/golden/make_keyframe_golden.py
"""
import importlib.util
import json
import os
import sys
from fractions import Fraction

import torch

from make_transforms_golden import REFERENCE   # the reference checkout (PV_REFERENCE_ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))

# (frame (H, W), short side): landscape, portrait, square, 720p
FRAMES = [((60, 90), 48), ((90, 60), 48), ((53, 53), 48), ((720, 1280), 256)]
# crop mode: (frame, short side, crop, spatial indices)
CROPS = [((60, 90), 56, 48, (0, 1, 2)), ((90, 60), 56, 48, (0, 1, 2)), ((53, 53), 56, 48, (1,)), ((720, 1280), 256, 224, (0, 2))]
# (clip duration, time stamps) for the sampler
WINDOWS = [(Fraction(16, 30), [Fraction(1), Fraction(3, 2), 0.9, 2.0]), (0.8, [0.4, 1.0, 1.25]), (2.0, [1.0, 902.0])]


def box_set(h, w):
    """[N,4] fp32 (x1, y1, x2, y2) on an h x w frame: inside, partly outside on every side, wholly outside, negative, on the
    border, zero-area, fractional, and one whose x2 (y2) lies 5 pixels beyond the frame, so that after the first clip its scaled
    corner still exceeds the scaled frame's last pixel and the second clip fires (60 x 90 -> 48: 95 -> 89 -> 71.2 -> 71)."""
    rows = [
        [0.25 * w, 0.25 * h, 0.75 * w, 0.5 * h],            # inside
        [3.5, 7.25, w - 10.75, h - 3.125],                  # inside, fractional
        [-12.0, 5.0, 0.5 * w, 0.5 * h],                     # partly outside: left
        [0.5 * w, -8.0, w + 20.0, 0.75 * h],                # top and right
        [10.0, 0.5 * h, 0.6 * w, h + 14.0],                 # bottom
        [w + 5.0, h + 5.0, w + 40.0, h + 30.0],             # wholly outside
        [-50.0, -40.0, -5.0, -2.0],                         # negative
        [0.0, 0.0, w - 1.0, h - 1.0],                       # the border
        [0.0, 0.0, float(w), float(h)],                     # one past the border
        [0.3 * w, 0.4 * h, 0.3 * w, 0.4 * h],               # zero area
        [0.5 * w, 0.2 * h, 0.5 * w, 0.9 * h],               # zero width
        [20.0, 10.0, w + 5.0, h + 5.0],                     # the second clip fires
        [1.0 / 3.0, 2.0 / 3.0, w - 1.0 / 3.0, h - 2.0 / 3.0],
    ]
    return torch.tensor(rows, dtype=torch.float32)


def listed(t):
    return [[float(v) for v in row] for row in torch.as_tensor(t).to(torch.float32).tolist()]


def load_functional():
    spec = importlib.util.spec_from_file_location("pv_ref_functional", os.path.join(REFERENCE, "pytorchvideo/transforms/functional.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    return F


def windows():
    """[{duration, stamp, start, end}] from the reference's TimeStampClipSampler, or [] where ava.py does not import."""
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from oracle import ref_shim
        ref_shim.install()
        from pytorchvideo.data.ava import TimeStampClipSampler
        from pytorchvideo.data.clip_sampling import UniformClipSampler
    except Exception as e:                                   # iopath / decoders missing
        print("TimeStampClipSampler not recorded: %s: %s" % (type(e).__name__, e))
        return []

    def frac(x):
        x = Fraction(x)
        return [x.numerator, x.denominator]

    out = []
    for duration, stamps in WINDOWS:
        sampler = TimeStampClipSampler(UniformClipSampler(duration))
        for t in stamps:
            info = sampler(None, None, {"clip_index": t})
            out.append({"duration": frac(duration), "stamp": frac(t), "start": frac(info.clip_start_sec), "end": frac(info.clip_end_sec),
                        "tail": [info.clip_index, info.aug_index, bool(info.is_last_clip)]})
    return out


def main():
    F = load_functional()
    cases = []
    for (h, w), size in FRAMES:                             # the tutorial: clip, scale, clip; no crop
        b0 = box_set(h, w)
        img = torch.zeros(3, 1, h, w)
        b1 = torch.as_tensor(F.clip_boxes_to_image(b0.clone(), h, w))
        scaled, b2 = F.short_side_scale_with_boxes(img, b1.clone(), size)
        b3 = torch.as_tensor(F.clip_boxes_to_image(b2.clone(), scaled.shape[-2], scaled.shape[-1]))
        cases.append({"height": h, "width": w, "short_side": size, "crop_size": None, "spatial_idx": 1, "clip_to_source": True,
                      "scaled": [int(scaled.shape[-2]), int(scaled.shape[-1])], "boxes": listed(b0), "clipped": listed(b1),
                      "expected": listed(b3)})
    for (h, w), size, crop, idxs in CROPS:                  # the eval pipeline: scale, then crop + clip
        b0 = box_set(h, w)
        img = torch.zeros(3, 1, h, w)
        scaled, b1 = F.short_side_scale_with_boxes(img, b0.clone(), size)
        for v in idxs:
            cropped, b2 = F.uniform_crop_with_boxes(scaled, crop, v, b1.clone())
            assert tuple(cropped.shape[-2:]) == (crop, crop)
            cases.append({"height": h, "width": w, "short_side": size, "crop_size": crop, "spatial_idx": v, "clip_to_source": False,
                          "scaled": [int(scaled.shape[-2]), int(scaled.shape[-1])], "boxes": listed(b0),
                          "expected": listed(torch.as_tensor(b2))})
    path = os.path.join(HERE, "keyframe_boxes.json")
    with open(path, "w") as f:
        json.dump({"source": "pytorchvideo/transforms/functional.py, pytorchvideo/data/ava.py", "cases": cases, "windows": windows()},
                  f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(cases), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
