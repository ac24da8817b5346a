"""Micro-benchmark of the packed YUV 4:2:2 source layouts of the ingest (src_layout "YUY2", "Y210": include/pv_mi355x.h,
"packed YUV 4:2:2") on the job of tools/bench_yuv4.py: the 30-item launch of a dataset evaluation -- 3 videos x 10 clips of 16
frames, short side to 256, centre crop 224, Div255 + Normalize, written as the planar bf16 clip a stem reads -- from 720p and
1080p sources, with the four-tap blend (pv_batch_views) and with the box filter (pv_area_views) (dev tool; needs the MI355X).

    python tools/bench_yuyv.py [--iters 20] [--rounds 3] [--sizes 720,1080] [--layouts YUY2,Y210] [--out FILE]

Every clip has 16 frames of its own (160 frames a video), so a launch reads far more than the last-level cache holds.  In this
process, on the same GPU, warmed up, timed with device events, `--rounds` interleaved rounds of:
  new      the launch on the packed frames, read where they lie
  (a)      the existing floor: the planar PV_SRC_YUV422 launch (I422 for YUY2, I216's arrangement for Y210, the same matrix)
           of the same frame size and sample width on the de-interleaved copy of the same frames
  (b)      the route a user has without the layouts: `yuyv_to_planar(video, layout).contiguous()` over the whole videos on the
           device, followed by launch (a) on the result
Before anything is timed, `new` is compared (torch.equal) with (a) -- the bit guarantee of the header, on benchmark-sized
frames.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pytorchvideo_amd import _lib as L
from pytorchvideo_amd import transforms as TR

MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
T, SHORT, SIZE = 16, 256, 224
VIDEOS, CLIPS = 3, 10
GEOMETRY = {720: (720, 1280), 1080: (1080, 1920), 2160: (2160, 3840)}
FLOOR = {"YUY2": "I422", "YVYU": "I422", "UYVY": "I422", "Y210": "I216", "Y212": "I216", "Y216": "I216"}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _launch(name, d):
    L.check(getattr(L.lib(), name)(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def run(size, layout, iters, rounds):
    dev = torch.device("cuda")
    hs, ws = GEOMETRY[size]
    floor = FLOOR[layout]
    wide = layout in TR._YUV_WIDE
    n_frames = CLIPS * T
    g = torch.Generator(device="cuda").manual_seed(5)
    lo, hi, dtype = (-32768, 32768, torch.int16) if wide else (0, 256, torch.uint8)
    videos = [torch.randint(lo, hi, (n_frames, hs, ws, 2), dtype=dtype, device="cuda", generator=g) for _ in range(VIDEOS)]
    copies = [TR.yuyv_to_planar(v, layout).contiguous() for v in videos]
    tables = [torch.arange(n_frames).view(CLIPS, T) for _ in range(VIDEOS)]           # every clip its own 16 frames
    n_items = VIDEOS * CLIPS
    scale, shift = TR._affine(MEAN, STD, True, 3, dev)
    matrix = TR._yuv_matrix_of(("bt709", False), layout).float().reshape(12).to(dev)   # ONE matrix: the copy holds the same codes
    lines = []
    for mode, entry in (("bilinear", "pv_batch_views"), ("area", "pv_area_views")):
        outs, descs, keep = [], [], []
        for vids, lay in ((videos, layout), (copies, floor)):
            batch = TR.build_video_batch(vids, tables, lay, SHORT, SIZE, (1,), [T], 3, dev, lambda t: t.to(dev))
            outer = L.AreaViewsDesc() if mode == "area" else L.BatchViewsDesc()
            d = outer.frames.batch if mode == "area" else outer
            if mode == "area":
                outer.filter = L.PV_FILTER_AREA
            TR._batch_launch_fields(d, batch, batch.tables[0], 0, n_items, 3, lay, matrix, (SIZE, SIZE))
            out = torch.empty((n_items, 3, T, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
            d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
            d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
            outs.append(out), descs.append(outer), keep.append(batch)

        def new():
            _launch(entry, descs[0])

        def floor_launch():
            _launch(entry, descs[1])

        def user_route():
            for c, v in zip(copies, videos):
                c.copy_(TR.yuyv_to_planar(v, layout).contiguous())   # the de-interleave pass, into the buffers (a) reads
            _launch(entry, descs[1])

        # the bit guarantee at this size: the new launch is the planar launch on the de-interleaved frames
        new(), floor_launch()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), "%s %s: the packed launch and the planar launch differ" % (layout, mode)
        user_route()
        torch.cuda.synchronize()
        tn, ta, tb = [], [], []
        for _ in range(rounds):
            tn.append(timed(new, iters))
            ta.append(timed(floor_launch, iters))
            tb.append(timed(user_route, max(1, iters // 4)))
        fmt = lambda v: " ".join("%8.4f" % x for x in v)
        spread = (max(ta) - min(ta)) / min(ta)
        spread_n = (max(tn) - min(tn)) / min(tn)
        lines.append("%dp %s %s, %d items x %d frames -> %d x %d planar bf16; ms per launch, %d interleaved rounds of %d launches" % (
            size, layout, mode, n_items, T, SIZE, SIZE, rounds, iters))
        lines.append("  new     %-14s  %s   min %.4f  (spread between rounds %.1f %%)" % (entry, fmt(tn), min(tn), 100 * spread_n))
        lines.append("  (a) %-4s launch, planar copy %s   min %.4f  (new / (a) %.3fx; spread of (a) between rounds %.1f %%)" % (
            floor, fmt(ta), min(ta), min(tn) / min(ta), 100 * spread))
        lines.append("  (b) yuyv_to_planar + (a)     %s   min %.4f  ((b) / new %.1fx)" % (fmt(tb), min(tb), min(tb) / min(tn)))
        print("\n".join(lines[-4:]), flush=True)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--layouts", default="YUY2,Y210")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuyv.py measures on the GPU; there is none here")
    table = []
    for s in args.sizes.split(","):
        for layout in args.layouts.split(","):
            table += run(int(s), layout, args.iters, args.rounds)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(table) + "\n")
