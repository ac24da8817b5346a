"""Micro-benchmark of the packed-pixel source layouts of the ingest (src_layout "BGR", "BGRA": include/pv_mi355x.h, "packed
pixels") on the job of tools/bench_area.py: the 30-item launch of a dataset evaluation -- 3 videos x 10 clips of 16 frames,
short side to 256, centre crop 224, Div255 + Normalize, written as the planar bf16 clip a stem reads -- from 720p and 1080p
sources, with the four-tap blend (pv_batch_views) and with the box filter (pv_area_views) (dev tool; needs the MI355X).

    python tools/bench_packed.py [--iters 20] [--rounds 3] [--sizes 720,1080]

Every clip has 16 frames of its own (160 frames a video), so a launch reads far more than the last-level cache holds.  The BGRA
surfaces are pitched (64 bytes of padding a row).  In this process, on the same GPU, warmed up, timed with device events,
`--rounds` interleaved rounds of:
  packed   the launch on the packed frames, read where they lie
  (a)      the PV_SRC_NTHWC launch of the dense R, G, B copy of the same frames: the kernel the packed one is compared with
  (b)      the route a user has without the layouts: the torch channel-select pass plus copy over the whole videos
           (`video[..., [2, 1, 0]].contiguous()`), followed by launch (a)
The outputs of `packed` and (a) are compared with torch.equal before anything is timed.
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
    pb = 3 if layout == "BGR" else 4
    pad = 0 if pb == 3 else 16                                   # pixels of row padding: a pitched 32-bit surface
    n_frames = CLIPS * T
    g = torch.Generator(device="cuda").manual_seed(5)
    surfaces = [torch.randint(0, 256, (n_frames, hs, ws + pad, pb), dtype=torch.uint8, device="cuda", generator=g) for _ in range(VIDEOS)]
    videos = [s[:, :, :ws] for s in surfaces]
    tables = [torch.arange(n_frames).view(CLIPS, T) for _ in range(VIDEOS)]           # every clip its own 16 frames
    n_items = VIDEOS * CLIPS
    scale, shift = TR._affine(MEAN, STD, True, 3, dev)
    select = list(TR._PACKED_RGB[layout])
    dense = [v[..., select].contiguous() for v in videos]
    lines = []
    for mode, entry in (("bilinear", "pv_batch_views"), ("area", "pv_area_views")):
        outs, descs, keep = [], [], []
        for vids, lay in ((videos, layout), (dense, "NTHWC")):
            batch = TR.build_video_batch(vids, tables, lay, SHORT, SIZE, (1,), [T], 3, dev, lambda t: t.to(dev))
            outer = L.AreaViewsDesc() if mode == "area" else L.BatchViewsDesc()
            d = outer.frames.batch if mode == "area" else outer
            if mode == "area":
                outer.filter = L.PV_FILTER_AREA
            TR._batch_launch_fields(d, batch, batch.tables[0], 0, n_items, 3, lay, None, (SIZE, SIZE))
            out = torch.empty((n_items, 3, T, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
            d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
            d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
            outs.append(out), descs.append(outer), keep.append(batch)

        def packed():
            _launch(entry, descs[0])

        def nthwc():
            _launch(entry, descs[1])

        def user_route():
            for k, v in enumerate(videos):
                dense[k].copy_(v[..., select])                   # the channel-select pass plus copy, into the buffer (a) reads
            _launch(entry, descs[1])

        packed(), nthwc(), user_route()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), "%s %s: the packed launch and the NTHWC launch differ" % (layout, mode)
        packed(), nthwc()
        torch.cuda.synchronize()
        tp, ta, tb = [], [], []
        for _ in range(rounds):
            tp.append(timed(packed, iters))
            ta.append(timed(nthwc, iters))
            tb.append(timed(user_route, max(1, iters // 4)))
        fmt = lambda v: " ".join("%8.4f" % x for x in v)
        spread = (max(ta) - min(ta)) / min(ta)
        lines.append("%dp %s %s, %d items x %d frames -> %d x %d planar bf16; ms per launch, %d interleaved rounds of %d launches" % (
            size, layout, mode, n_items, T, SIZE, SIZE, rounds, iters))
        lines.append("  packed  %-14s  %s   min %.4f" % (entry, fmt(tp), min(tp)))
        lines.append("  (a) NTHWC of the RGB copy %s   min %.4f  (packed / (a) %.3fx; spread of (a) between rounds %.1f %%)" % (
            fmt(ta), min(ta), min(tp) / min(ta), 100 * spread))
        lines.append("  (b) torch select + (a)    %s   min %.4f  ((b) / packed %.1fx)" % (fmt(tb), min(tb), min(tb) / min(tp)))
        print("\n".join(lines[-4:]), flush=True)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--layouts", default="BGR,BGRA")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_packed.py measures on the GPU; there is none here")
    for s in args.sizes.split(","):
        for layout in args.layouts.split(","):
            run(int(s), layout, args.iters, args.rounds)
            torch.cuda.empty_cache()
