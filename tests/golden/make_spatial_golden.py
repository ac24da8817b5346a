"""Record the REAL reference's spatial eval transforms (pytorchvideo/transforms/functional.py, loaded by file path: the
package __init__ pulls in torchvision): short_side_scale, uniform_crop and the four box functions
-> tests/golden/spatial_transforms.pt.  Inputs are regenerated from seeds by the tests; only expected outputs are stored.
Runs only where the reference tree exists.

    python tests/golden/make_spatial_golden.py
"""
import importlib.util
import os

import torch

from make_transforms_golden import REFERENCE   # the reference checkout (PV_REFERENCE_ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD = (0.45, 0.40, 0.50), (0.225, 0.25, 0.2)

# (clip shape (C,T,H,W), short side, crop, spatial indices): landscape, portrait and square sources, up- and down-scaling,
# odd sizes; every spatial index on both orientations
CASES = [
    ((3, 2, 97, 131), 64, 56, (1,)),
    ((3, 2, 131, 97), 32, 28, (0, 1, 2)),
    ((3, 2, 40, 40), 64, 48, (1,)),
    ((3, 2, 90, 160), 48, 48, (2,)),
    ((3, 2, 49, 67), 32, 28, (0, 1, 2)),
    ((3, 2, 150, 200), 32, 32, (1,)),
    ((3, 2, 30, 23), 41, 37, (0, 2)),
]
# (frame (H,W), number of boxes, short side, crop, spatial index)
BOX_CASES = [((97, 131), 5, 64, 56, 0), ((131, 97), 4, 64, 56, 2), ((90, 160), 6, 48, 48, 1), ((40, 40), 3, 64, 48, 1)]


def clip(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def boxes(n, h, w, seed):
    """[n,4] (x1, y1, x2, y2) float32, some of them reaching outside the frame so that clipping has work to do."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 4, generator=g) * torch.tensor([w, h, w, h], dtype=torch.float32) * 1.2 - 0.1 * max(h, w)
    x = torch.stack([torch.minimum(p[:, 0], p[:, 2]), torch.minimum(p[:, 1], p[:, 3]),
                     torch.maximum(p[:, 0], p[:, 2]), torch.maximum(p[:, 1], p[:, 3])], 1)
    return x.contiguous()


def normalised(u8):
    """Normalize(Div255(x)) of a (C,T,H,W) uint8 clip, as the reference pipelines compose it (fp32)."""
    x = u8.float() / 255.0
    return (x - torch.tensor(MEAN).view(3, 1, 1, 1)) / torch.tensor(STD).view(3, 1, 1, 1)


def main():
    spec = importlib.util.spec_from_file_location("pv_ref_functional", os.path.join(REFERENCE, "pytorchvideo/transforms/functional.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    out = {"chain": [], "scaled_shape": [], "boxes": []}
    for i, (shape, size, crop, idxs) in enumerate(CASES):
        scaled = F.short_side_scale(normalised(clip(shape, 300 + i)), size)
        out["scaled_shape"].append(tuple(scaled.shape))
        out["chain"].append({v: F.uniform_crop(scaled, crop, v).clone() for v in idxs})
    for i, ((h, w), n, size, crop, v) in enumerate(BOX_CASES):
        img = clip((3, 1, h, w), 400 + i).float()
        b0 = boxes(n, h, w, 500 + i)
        scaled, b1 = F.short_side_scale_with_boxes(img, b0.clone(), size)
        cropped, b2 = F.uniform_crop_with_boxes(scaled, crop, v, b1.clone())
        out["boxes"].append({
            "scaled": torch.as_tensor(b1).clone(), "cropped": torch.as_tensor(b2).clone(), "cropped_shape": tuple(cropped.shape),
            "clip_only": torch.as_tensor(F.clip_boxes_to_image(b0.clone(), h // 2, w // 2)).clone(),
            "crop_only": torch.as_tensor(F.crop_boxes(b0.clone(), 7, 3)).clone(),
        })
    path = os.path.join(HERE, "spatial_transforms.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
