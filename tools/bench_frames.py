"""Whole-video rate on a decoder's surface pool: `VideoPredictor` on a `FrameList` against stacking the surfaces first
(dev tool; needs the MI355X).

    timeout -k 10 900 python tools/bench_frames.py [--batch 32] [--rounds 3] [--out FILE]

Workload: X3D-M (16 x 224 x 224), bf16, deploy batch `--batch`; one 300-frame 720 x 1280 NV12 video held as 300 separate
surfaces on the device (one allocation each, allocated in a shuffled order); the model-zoo test protocol, 10 clips x 3
crops = 30 views, short side 256, crop 224.
A: `VideoPredictor` on the `FrameList`: one table of 300 frame addresses uploaded with the records, the ingest reads every
   surface where it lies (`pv_frame_views`).
B: what a user does without it: `torch.stack` of the 300 surfaces into one [N, Hc*3/2, W] tensor on EVERY call (414 MB
   written, as much read), then `VideoPredictor` on that tensor (`pv_yuv_views`).
Both in this process on the same GPU.  Asserted: the scores of A and B are `torch.equal` (the same items at the same batch
positions).  Measured: interleaved windows A B A' of about 1 s each, every window warmed up, host clock around work that
ends in a device synchronise; |A - A'| is the spread a difference has to beat.  No speed-up is asserted.
"""
import argparse
import os
import statistics
import sys
import time
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pytorchvideo_amd import data as D
from pytorchvideo_amd import transforms as TR
from pytorchvideo_amd.inference import VideoPredictor

MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
FRAMES, FPS, HS, WS = 300, 30, 720, 1280
KW = dict(mean=MEAN, std=STD, div255=True, short_side=256, crop_size=224, src_layout="NV12")


def deploy(batch):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_x3d
    from pytorchvideo_amd.utils import randomize_norm_stats
    torch.manual_seed(0)
    m = randomize_norm_stats(create_x3d(input_clip_length=16, input_crop_size=224, model_num_class=400), 0).eval()
    transmute_model(m, "mi355x")
    x = torch.zeros(batch, 3, 16, 224, 224, device="cuda", dtype=torch.bfloat16)
    return convert_to_deployable_form(m, x, dtype=torch.bfloat16)


def window(fn, calls):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return calls / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_frames.py measures on the GPU; there is none here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    g = torch.Generator("cuda").manual_seed(3)
    surfaces = [None] * FRAMES
    for i in torch.randperm(FRAMES, generator=torch.Generator().manual_seed(4)).tolist():
        surfaces[i] = torch.randint(0, 256, (HS * 3 // 2, WS), dtype=torch.uint8, device="cuda", generator=g)
    frames = TR.FrameList(surfaces, "NV12")
    pred = VideoPredictor(deploy(a.batch), D.ConstantClipsPerVideoSampler(Fraction(80, FPS), 10), **KW)

    def route_a():
        return pred(frames, FPS)

    def route_b():
        return pred(torch.stack(surfaces), FPS)

    s_a, s_b = route_a().clone(), route_b().clone()
    say("X3D-M bf16, deploy batch %d, one %d-frame %d x %d NV12 video as %d separate surfaces, 10 clips x 3 crops, short side 256, "
        "crop 224: A = VideoPredictor on the FrameList (pv_frame_views); B = torch.stack of the surfaces on every call, then "
        "VideoPredictor on the tensor (pv_yuv_views); scores torch.equal: %s; top score %.4f"
        % (a.batch, FRAMES, HS, WS, FRAMES, torch.equal(s_a, s_b), s_a.max().item()))
    assert torch.equal(s_a, s_b), "A and B disagree by %.3e" % (s_a - s_b).abs().max().item()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    route_a()
    torch.cuda.synchronize()
    calls = max(1, round(1.0 / (time.perf_counter() - t0)))     # ~1 s per timed window
    res = []
    for r in range(a.rounds):
        va, vb, va2 = window(route_a, calls), window(route_b, calls), window(route_a, calls)
        res.append((va, vb, va2))
        say("  round %d: FrameList %8.2f videos/s | stack first %8.2f | FrameList again %8.2f" % (r, va, vb, va2))
    med_a = statistics.median([x for va, _, va2 in res for x in (va, va2)])
    med_b = statistics.median([vb for _, vb, _ in res])
    spread = max(abs(va - va2) / max(va, va2) for va, _, va2 in res)
    say("  median: A %.2f videos/s, B %.2f videos/s; A / B = %.3f; A/A' spread (max over rounds) %.1f %%"
        % (med_a, med_b, med_a / med_b, 100 * spread))
    return 0


if __name__ == "__main__":
    sys.exit(main())
