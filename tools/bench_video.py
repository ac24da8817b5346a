"""Whole-video inference rate of X3D-M (16 x 224 x 224, bf16): `inference.VideoPredictor` (the clip sampler's frame table
read by the ingest kernel, `pv_video_views`) against the route the same job took before it -- clips materialised by
index_select, `DevicePacker.__call__`, `VideoEnsembler` -- on the SAME deploy form, in this process, on the same GPU
(dev tool; needs the MI355X).

    timeout -k 10 900 python tools/bench_video.py [--videos 300] [--rounds 5] [--out FILE]

One video = 300 frames of 256 x 340 uint8 [N,H,W,3] resident on the device, 30 fps; the model zoo's protocol:
ConstantClipsPerVideoSampler(80 frames, 10 clips) x 3 crops = 30 views, 16 of every 80 frames.  Both routes build the frame
table on the host and upload it per video.  The old route copies the 10 x 16 selected frames into clip tensors (the cheapest
form of it: `DevicePacker.__call__` takes clips that already have the pathway's frame count) and can only run a deploy form
whose batch is a multiple of the 3 views, so the A/B is at batch 30 = one forward per video; the new route is also timed at
the bench batch of 32, which the old route cannot run at all (30 of 32 items: the ragged tail).

Method: the two routes give bit-equal scores (checked first); `rounds` interleaved windows A B A' of `videos` videos each,
host clock around work that ends in a device synchronise, every window warmed up; A' is the new route again, so |A - A'| is
the spread a difference has to beat.  Prints videos/s per window, the medians and the spread.
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
from pytorchvideo_amd.ensemble import VideoEnsembler
from pytorchvideo_amd.inference import VideoPredictor

MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
FRAMES, FPS, HS, WS = 300, 30, 256, 340
KW = dict(mean=MEAN, std=STD, div255=True, short_side=256, crop_size=224)


def sampler():
    return D.ConstantClipsPerVideoSampler(Fraction(80, FPS), 10, 3)


def deploy(batch, streams):
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_x3d
    from pytorchvideo_amd.utils import randomize_norm_stats
    torch.manual_seed(0)
    m = randomize_norm_stats(create_x3d(input_clip_length=16, input_crop_size=224, model_num_class=400), 0).eval()
    transmute_model(m, "mi355x")
    x = torch.zeros(batch, 3, 16, 224, 224, device="cuda", dtype=torch.bfloat16)
    return convert_to_deployable_form(m, x, dtype=torch.bfloat16, streams=streams)


class OldRoute:
    """Materialise the clips, pack them, fold: the pieces that existed before `VideoPredictor`."""

    def __init__(self, dep):
        self.packer = TR.DevicePacker(dep, spatial_idx=(0, 1, 2), src_layout="NTHWC", **KW)
        self.sampler = sampler()

    @torch.no_grad()
    def __call__(self, video, fps):
        table, _ = D.clip_frame_table(self.sampler, video.shape[0], fps, 16)
        n_clips, t = table.shape
        flat = table.reshape(-1).long().to(video.device)
        clips = video.index_select(0, flat).view(n_clips, t, *video.shape[1:])
        logits = self.packer(clips)
        ens = VideoEnsembler(1, logits.shape[1], "sum", video.device)
        ens.update(logits, torch.zeros(logits.shape[0], dtype=torch.int32, device=video.device))
        return ens.result()[0]


def window(fn, video, videos):
    for _ in range(2):
        fn(video, FPS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(videos):
        fn(video, FPS)
    torch.cuda.synchronize()
    return videos / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=300)     # ~1 s per timed window
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_video.py measures on the GPU; there is none here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    video = torch.randint(0, 256, (FRAMES, HS, WS, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    dep = deploy(30, a.streams)
    new, old = VideoPredictor(dep, sampler(), **KW), OldRoute(dep)
    s_new, s_old = new(video, FPS).clone(), old(video, FPS).clone()
    same = torch.equal(s_new, s_old)
    say("X3D-M bf16, one %d-frame %dx%d uint8 NTHWC video, 10 clips x 3 crops, deploy batch 30 (streams=%d); scores bit-equal: %s; "
        "rows folded: %d" % (FRAMES, HS, WS, a.streams, same, int(new.video_ensembler.counts.item())))
    rows = []
    for r in range(a.rounds):
        va, vb, va2 = window(new, video, a.videos), window(old, video, a.videos), window(new, video, a.videos)
        rows.append((va, vb, va2))
        say("round %d: VideoPredictor %8.2f videos/s | materialise + DevicePacker %8.2f | VideoPredictor again %8.2f" % (r, va, vb, va2))
    med_new = statistics.median([x for va, _, va2 in rows for x in (va, va2)])
    med_old = statistics.median([vb for _, vb, _ in rows])
    spread = max(abs(va - va2) / max(va, va2) for va, _, va2 in rows)
    say("median: VideoPredictor %.2f videos/s (%.1f views/s), old route %.2f videos/s; new / old = %.3f; A/A spread (max over "
        "rounds) %.1f %%" % (med_new, 30 * med_new, med_old, med_new / med_old, 100 * spread))
    say("not slower than the old route by more than the A/A spread: %s" % (med_new >= med_old * (1 - spread)))
    del new, old, dep
    torch.cuda.empty_cache()
    dep32 = deploy(32, a.streams)                      # the bench batch: 30 of 32 items, only the new route can run it
    new32 = VideoPredictor(dep32, sampler(), **KW)
    s32 = new32(video, FPS)
    say("deploy batch 32 (ragged: 30 of 32 items): rows folded %d, max |score - batch-30 score| %.3e"
        % (int(new32.video_ensembler.counts.item()), (s32 - s_new).abs().max().item()))
    v32 = [window(new32, video, a.videos) for _ in range(3)]
    say("deploy batch 32: VideoPredictor %s videos/s" % " ".join("%.2f" % v for v in v32))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
