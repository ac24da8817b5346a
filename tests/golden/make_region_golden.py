"""Record the REAL reference's crop-and-resize (pytorchvideo/transforms/functional.py `random_resized_crop`, loaded by file
path: the package __init__ pulls in torchvision) on CHOSEN rectangles -> tests/golden/region_transforms.pt.  The function
draws its rectangles from `_get_param_spatial_crop`; that one name is replaced by an iterator over the rectangles below, and
everything behind it -- the crop, `interpolate`, and with `shift=True` the per-frame rectangles (`torch.linspace` + `int()`)
-- is the reference's own code.  Inputs are regenerated from seeds by the tests; only expected outputs are stored.  Runs only
where the reference tree exists.

    python tests/golden/make_region_golden.py
"""
import importlib.util
import os

import torch

from make_transforms_golden import REFERENCE   # the reference checkout (PV_REFERENCE_ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (3, 5, 37, 53)                          # (C, T, H, W): odd sizes
# ([rectangle (top, left, h, w)] -- one: shift=False; two: shift=True, first and last frame --, (Ho, Wo))
CASES = [
    ([(3, 5, 20, 9)], (16, 16)),                # an upscale of a narrow rectangle
    ([(0, 0, 37, 53)], (16, 24)),               # the full frame, downscaled
    ([(36, 52, 1, 1)], (8, 8)),                 # one pixel, the bottom-right one
    ([(1, 2, 35, 50)], (7, 9)),                 # a downscale by 5: taps far apart
    ([(10, 11, 13, 17)], (13, 17)),             # the identity size
    ([(3, 5, 20, 9), (10, 30, 11, 21)], (12, 14)),   # a rectangle that moves and changes size over the clip
]


def clip(seed):
    return torch.randint(0, 256, SHAPE, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def main():
    spec = importlib.util.spec_from_file_location("pv_ref_functional", os.path.join(REFERENCE, "pytorchvideo/transforms/functional.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    out = []
    for i, (rects, (ho, wo)) in enumerate(CASES):
        chosen = iter(rects)
        F._get_param_spatial_crop = lambda *a, **k: next(chosen)
        got = F.random_resized_crop(clip(600 + i).float(), ho, wo, (0.5, 1.0), (0.75, 1.33), shift=len(rects) == 2)
        assert next(chosen, None) is None and tuple(got.shape) == (SHAPE[0], SHAPE[1], ho, wo)
        out.append(got.clone())
    path = os.path.join(HERE, "region_transforms.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
