"""Key-frame action detection rate, `inference.KeyframeDetector` against one call per key frame (dev tool; needs the MI355X).

    timeout -k 10 900 python tools/bench_keyframes.py [--batch 8] [--keyframes 16] [--rounds 3] [--out FILE]

Workload: slowfast_r50_detection, bf16, one 720 x 1280 uint8 [N,H,W,3] video resident on the device, short side 256 and the
centre 256 x 256 crop, a clip of 32 frames around every key frame, 3 / 5 / 8 person boxes per key frame (cycled).
A: `KeyframeDetector` on a deploy form of `--batch` key frames and 8 boxes per key frame of capacity: frame table, boxes and
   their key-frame index uploaded once per call; per forward the ingest reads the video through the table
   (`pv_batch_views`), `pv_box_views` maps the boxes on the device, one replay.
B: the same key frames one by one through `DevicePacker(dm)(clip, bboxes)`, the route before: the clip of every key frame
   is gathered from the video on the device, its boxes are mapped on the host and copied to the device, and the forward runs
   on a deploy form converted for batch 1 and EXACTLY that key frame's box count (one form per distinct count).
Both in this process on the same GPU.  Asserted: the scores of A and B agree within the bf16 bound on sigmoid scores the
detection tests use (2.5e-2; an item sits at another batch position, so they are not bit-equal -- the largest difference is
printed).  Measured: interleaved windows A B A' of about 1 s each, every window warmed up, host clock around work that ends
in a device synchronise; |A - A'| is the spread a difference has to beat.  No speed-up is asserted.
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
from pytorchvideo_amd.inference import KeyframeDetector, keyframe_chunks

MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
FPS, FRAMES, HS, WS = 30, 150, 720, 1280
SHORT, CROP, CLIP = 256, 256, 32
BOXES_PER_KEYFRAME = (3, 5, 8)


def deploy(batch, n_boxes):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import hub
    torch.manual_seed(0)
    model = hub.slowfast_r50_detection().eval()
    transmute_model(model, "mi355x")
    x = [torch.zeros((batch, 3, CLIP // 4, CROP, CROP), device="cuda", dtype=torch.bfloat16),
         torch.zeros((batch, 3, CLIP, CROP, CROP), device="cuda", dtype=torch.bfloat16)]
    boxes = torch.zeros(n_boxes, 5)
    boxes[:, 3:] = 32.0
    return convert_to_deployable_form(model, (x, boxes), dtype=torch.bfloat16)


def person_boxes(counts):
    g = torch.Generator().manual_seed(1)
    out = []
    for c in counts:
        xy = torch.rand((c, 2), generator=g) * torch.tensor([WS * 0.7, HS * 0.6])
        wh = torch.rand((c, 2), generator=g) * torch.tensor([WS * 0.2, HS * 0.35]) + 40.0
        out.append(torch.cat([xy, xy + wh], 1))
    return out


def window(fn, calls, keyframes):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return calls * keyframes / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_keyframes.py measures on the GPU; there is none here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    kw = dict(mean=MEAN, std=STD, div255=True, short_side=SHORT, crop_size=CROP, spatial_idx=1, frame_ratios=(4, 1), src_layout="NTHWC")
    video = torch.randint(0, 256, (FRAMES, HS, WS, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    duration = Fraction(CLIP, FPS)
    first, last = duration / 2, Fraction(FRAMES, FPS) - duration / 2
    stamps = [first + (last - first) * k / max(a.keyframes - 1, 1) for k in range(a.keyframes)]
    counts = [BOXES_PER_KEYFRAME[k % len(BOXES_PER_KEYFRAME)] for k in range(a.keyframes)]
    boxes = person_boxes(counts)
    capacity = a.batch * max(BOXES_PER_KEYFRAME)
    det = KeyframeDetector(deploy(a.batch, capacity), duration, **kw)
    singles = {c: TR.DevicePacker(deploy(1, c), **kw) for c in sorted(set(counts))}
    table, _ = D.keyframe_frame_table(stamps, duration, FRAMES, FPS, CLIP)
    rows = [r.long().cuda() for r in table]
    host_boxes = [torch.cat([torch.zeros(c, 1), b], 1) for c, b in zip(counts, boxes)]

    def route_a():
        return det(video, FPS, stamps, boxes)

    def route_b():
        out = []
        for k, c in enumerate(counts):
            clip = video[rows[k]][None]                      # the materialised clip of this key frame, [1,T,H,W,3]
            out.append(singles[c](clip, host_boxes[k]).clone())
        return torch.cat(out)

    s_a, s_b = route_a().clone(), route_b()
    diff = (s_a - s_b).abs().max().item()
    chunks = keyframe_chunks(counts, a.batch, capacity)
    say("slowfast_r50_detection bf16, %d x %d video of %d frames, short side %d, crop %d, %d key frames with %s boxes (%d in all): "
        "A = KeyframeDetector, deploy batch %d, capacity %d: %d forwards; B = one DevicePacker call per key frame on forms of batch 1 "
        "and %s boxes: %d forwards; max |score A - score B| %.3e; scores %.3f..%.3f, std over the boxes (mean over classes) %.3e"
        % (HS, WS, FRAMES, SHORT, CROP, a.keyframes, "/".join(map(str, BOXES_PER_KEYFRAME)), sum(counts), a.batch, capacity, det.forwards,
           "/".join(map(str, sorted(singles))), a.keyframes, diff, s_a.min().item(), s_a.max().item(), s_a.std(0).mean().item()))
    assert det.forwards == len(chunks) and tuple(s_a.shape) == tuple(s_b.shape) == (sum(counts), s_a.shape[1])
    assert diff <= 2.5e-2, "A and B disagree by %.3e" % diff
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    route_a()
    torch.cuda.synchronize()
    calls = max(1, round(1.0 / (time.perf_counter() - t0)))     # ~1 s per timed window
    res = []
    for r in range(a.rounds):
        va, vb, va2 = window(route_a, calls, a.keyframes), window(route_b, calls, a.keyframes), window(route_a, calls, a.keyframes)
        res.append((va, vb, va2))
        say("  round %d: KeyframeDetector %8.2f key frames/s | per key frame %8.2f | KeyframeDetector again %8.2f" % (r, va, vb, va2))
    med_a = statistics.median([x for va, _, va2 in res for x in (va, va2)])
    med_b = statistics.median([vb for _, vb, _ in res])
    spread = max(abs(va - va2) / max(va, va2) for va, _, va2 in res)
    say("  median: A %.2f key frames/s, B %.2f key frames/s; A / B = %.3f; A/A' spread (max over rounds) %.1f %%"
        % (med_a, med_b, med_a / med_b, 100 * spread))
    return 0


if __name__ == "__main__":
    sys.exit(main())
