"""Record the REAL reference's `horizontal_flip_with_boxes` (pytorchvideo/transforms/functional.py:380-404) ->
tests/golden/orient_boxes.json (numbers only): the boxes of a mirrored frame, alone and followed by the eval pipeline's
`short_side_scale_with_boxes` and `uniform_crop_with_boxes`.  It is what orientation code 4 (mirror, no turn) of
`transforms.orient_boxes` / `boxes_to_view(..., orientation=4)` must equal.  functional.py is loaded by file path, as
make_keyframe_golden.py loads it, and the box sets are that generator's.  Runs only where the reference tree exists.

fp32 values are stored as the Python floats they convert to exactly, so the fixture compares bit for bit.

    python tests/golden/make_orient_golden.py
"""
import json
import os

import torch

from make_keyframe_golden import box_set, listed, load_functional

HERE = os.path.dirname(os.path.abspath(__file__))

# (frame (H, W), short side, crop, spatial indices): landscape, portrait, square
CASES = [((60, 90), 56, 48, (0, 1, 2)), ((90, 60), 56, 48, (0, 2)), ((53, 53), 56, 48, (1,)), ((45, 71), 24, 24, (0, 1, 2))]


def main():
    F = load_functional()
    cases = []
    for (h, w), size, crop, idxs in CASES:
        b0 = box_set(h, w)
        img = torch.zeros(3, 1, h, w)
        flipped_img, b1 = F.horizontal_flip_with_boxes(1.0, img, b0.clone())        # prob 1: always flipped
        assert tuple(flipped_img.shape) == tuple(img.shape)
        scaled, b2 = F.short_side_scale_with_boxes(flipped_img, torch.as_tensor(b1).clone(), size)
        views = []
        for v in idxs:
            _, b3 = F.uniform_crop_with_boxes(scaled, crop, v, b2.clone())
            views.append({"spatial_idx": v, "expected": listed(b3)})
        cases.append({"height": h, "width": w, "short_side": size, "crop_size": crop, "boxes": listed(b0), "flipped": listed(b1),
                      "views": views})
    path = os.path.join(HERE, "orient_boxes.json")
    with open(path, "w") as f:
        json.dump({"source": "pytorchvideo/transforms/functional.py: horizontal_flip_with_boxes", "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, len(cases), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
