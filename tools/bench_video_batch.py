"""Dataset-evaluation rate, many videos per forward against one video per call (dev tool; needs the MI355X).

    timeout -k 10 900 python tools/bench_video_batch.py [--config mvit_b x3d_m slowfast_r50] [--rounds 3] [--out FILE]

A: `inference.VideoBatchPredictor` over 16 videos per call -- every forward filled with views of as many videos as it takes
   (`pv_batch_views`), one table upload per call.
B: a loop of `inference.VideoPredictor`, one call per video: every video ends in its own short forward and uploads its own
   table.  This is the route a dataset evaluation took before.
Both on the SAME deploy form, in this process, on the same GPU, the 16 videos (uint8 [N,H,W,3], lengths and frame sizes that
differ) resident on the device.  Configurations, the model zoo's test protocols at the bench batches:
   mvit_b        MViT-B 32x3, batch 8,  5 clips x 1 crop  = 5 views:   80 items = 10 forwards against 16
   x3d_m         X3D-M,       batch 32, 10 clips x 3 crops = 30 views: 480 items = 15 forwards against 16
   slowfast_r50  SlowFast-R50, batch 16, 10 x 3 = 30 views:            480 items = 30 forwards against 32

Asserted: the forwards per 16 videos, and that A and B agree in the top-1 class of every video (their scores are not
bit-equal: an item sits at another batch position; the largest difference is printed).  Measured: interleaved windows
A B A' of about 1 s each, every window warmed up, host clock around work that ends in a device synchronise; |A - A'| is the
spread a difference has to beat.  Prints videos/s per window, the medians, the ratio and the spread.
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
from pytorchvideo_amd.inference import VideoBatchPredictor, VideoPredictor

MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
FPS, VIDEOS = 30, 16
# lengths and frame sizes of the 16 videos (cycled): what a dataset looks like to the ingest
SHAPES = [(300, 256, 340), (240, 240, 320), (180, 360, 480), (270, 256, 256), (210, 340, 256), (300, 288, 352), (150, 256, 454),
          (260, 270, 480)]


def _x3d_m():
    from pytorchvideo_amd.models import create_x3d
    return create_x3d(input_clip_length=16, input_crop_size=224, model_num_class=400), [(3, 16, 224, 224)]


def _slowfast_r50():
    from pytorchvideo_amd.models import create_slowfast
    return create_slowfast(model_depth=50), [(3, 8, 256, 256), (3, 32, 256, 256)]


def _mvit_b():
    from pytorchvideo_amd.models import create_multiscale_vision_transformers
    from pytorchvideo_amd.models.hub import mvit_video_base_32x3_config as cfg
    return create_multiscale_vision_transformers(**cfg), [(3, 32, 224, 224)]


# name: (builder, deploy batch, clip duration in frames, clips, crops, short side, crop, frame_ratios, forwards A, forwards B)
CONFIGS = {
    "mvit_b": (_mvit_b, 8, 96, 5, (1,), 256, 224, None, 10, 16),
    "x3d_m": (_x3d_m, 32, 80, 10, (0, 1, 2), 256, 224, None, 15, 16),
    "slowfast_r50": (_slowfast_r50, 16, 64, 10, (0, 1, 2), 256, 256, (4, 1), 30, 32),
}


def deploy(builder, batch, streams):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.utils import randomize_norm_stats
    torch.manual_seed(0)
    model, shapes = builder()
    model = randomize_norm_stats(model, 0).eval()
    transmute_model(model, "mi355x")
    x = [torch.zeros((batch,) + s, device="cuda", dtype=torch.bfloat16) for s in shapes]
    return convert_to_deployable_form(model, x if len(x) > 1 else x[0], dtype=torch.bfloat16, streams=streams)


def videos():
    g = torch.Generator().manual_seed(3)
    out = []
    for i in range(VIDEOS):
        n, h, w = SHAPES[i % len(SHAPES)]
        out.append(torch.randint(0, 256, (n - i, h, w, 3), dtype=torch.uint8, generator=g).cuda())
    return out


def window(fn, calls):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return calls * VIDEOS / (time.perf_counter() - t0)


def run(name, vids, rounds, streams, say):
    builder, batch, clip, clips, crops, short, crop, ratios, want_a, want_b = CONFIGS[name]
    kw = dict(mean=MEAN, std=STD, div255=True, short_side=short, crop_size=crop, spatial_idx=crops, frame_ratios=ratios)
    dep = deploy(builder, batch, streams)

    def sampler():
        return D.ConstantClipsPerVideoSampler(Fraction(clip, FPS), clips, len(crops))

    many, one = VideoBatchPredictor(dep, sampler(), **kw), VideoPredictor(dep, sampler(), **kw)
    state = {"forwards": 0}
    launch = one.packer.launch

    def counted():
        state["forwards"] += 1
        return launch()
    one.packer.launch = counted

    def route_a():
        return many(vids, FPS)

    def route_b():
        return torch.stack([one(v, FPS) for v in vids])

    s_a = route_a().clone()
    state["forwards"] = 0
    s_b = route_b().clone()
    fa, fb = many.forwards, state["forwards"]
    views = many.video_ensembler.counts.tolist()
    top_a, top_b = s_a.argmax(1).tolist(), s_b.argmax(1).tolist()
    say("%s bf16, deploy batch %d (streams=%d), %d videos of %d..%d frames, %d clips x %d crops: forwards per %d videos A %d, B %d; "
        "views folded per video %s; top-1 agree: %s; max |score A - score B| %.3e"
        % (name, batch, streams, VIDEOS, min(v.shape[0] for v in vids), max(v.shape[0] for v in vids), clips, len(crops), VIDEOS, fa, fb,
           sorted(set(views)), top_a == top_b, (s_a - s_b).abs().max().item()))
    assert (fa, fb) == (want_a, want_b), "forwards per %d videos: A %d (want %d), B %d (want %d)" % (VIDEOS, fa, want_a, fb, want_b)
    assert views == [clips * len(crops)] * VIDEOS
    assert top_a == top_b, "top-1 differs: A %s, B %s" % (top_a, top_b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    route_a()
    torch.cuda.synchronize()
    calls = max(1, round(1.0 / (time.perf_counter() - t0)))     # ~1 s per timed window
    rows = []
    for r in range(rounds):
        va, vb, va2 = window(route_a, calls), window(route_b, calls), window(route_a, calls)
        rows.append((va, vb, va2))
        say("  round %d: VideoBatchPredictor %8.2f videos/s | VideoPredictor per video %8.2f | VideoBatchPredictor again %8.2f" % (r, va, vb, va2))
    med_a = statistics.median([x for va, _, va2 in rows for x in (va, va2)])
    med_b = statistics.median([vb for _, vb, _ in rows])
    spread = max(abs(va - va2) / max(va, va2) for va, _, va2 in rows)
    ok = med_a >= med_b * (1 - spread)
    say("  median: A %.2f videos/s, B %.2f videos/s; A / B = %.3f; A/A' spread (max over rounds) %.1f %%; A not slower than B by more "
        "than the spread: %s" % (med_a, med_b, med_a / med_b, 100 * spread, ok))
    one.packer.launch = launch
    del many, one, dep
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_video_batch.py measures on the GPU; there is none here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                        # written as it goes: a later configuration's failure keeps the earlier ones
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    vids = videos()
    ok = [run(name, vids, a.rounds, a.streams, say) for name in a.config]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
