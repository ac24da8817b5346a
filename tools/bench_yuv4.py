"""Micro-benchmark of the YUV 4:2:2 / 4:4:4 source layouts of the ingest (src_layout "I422", "NV16", "I210", "I444":
include/pv_mi355x.h, "YUV 4:2:2 and 4:4:4") on the job of tools/bench_packed.py: the 30-item launch of a dataset evaluation --
3 videos x 10 clips of 16 frames, short side to 256, centre crop 224, Div255 + Normalize, written as the planar bf16 clip a
stem reads -- from 720p and 1080p sources, with the four-tap blend (pv_batch_views) and with the box filter (pv_area_views)
(dev tool; needs the MI355X).

    python tools/bench_yuv4.py [--iters 20] [--rounds 3] [--sizes 720,1080] [--layouts I422,NV16,I210,I444]

Every clip has 16 frames of its own (160 frames a video), so a launch reads far more than the last-level cache holds.  In this
process, on the same GPU, warmed up, timed with device events, `--rounds` interleaved rounds of:
  new      the launch on the 4:2:2 / 4:4:4 frames, read where they lie
  (a)      the existing floor: the 4:2:0 launch of the same frame size, chroma arrangement and sample width (I420 for I422 and
           I444, NV12 for NV16, I010 for I210) on the decimated copy of the same frames
  (b)      the route a user has without the layouts: a torch pass that writes the 4:2:0 copy of the whole videos (luma copied,
           every other chroma row -- 4:4:4: and column -- kept), followed by launch (a)
Before anything is timed, `new` is compared (torch.equal) with the launch of its own layout on the frames whose chroma the
4:2:0 copy replicates -- the bit guarantee of the header, on benchmark-sized frames.
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
FLOOR = {"I422": "I420", "NV16": "NV12", "I210": "I010", "I444": "I420", "I410": "I010", "P210": "P010"}


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


def _rows(layout, h):
    return h * 2 if layout in TR.YUV422_LAYOUTS else h * 3 if layout in TR.YUV444_LAYOUTS else h * 3 // 2


def _planes(video, layout):
    """(Y, U, V) of contiguous frames as strided views: nothing is copied."""
    g = TR.yuv_geometry(video, layout)
    sb = video.element_size()
    csy, csx = g.get("csy", 1), g.get("csx", 1)

    def plane(rows, cols, pitch, step, start):
        return torch.as_strided(video, (g["N"], rows, cols), (g["frame_stride"] // sb, pitch // sb, step), video.storage_offset() + start // sb)

    hc, wc = g["Hs"] >> csy, g["Ws"] >> csx
    return (plane(g["Hs"], g["Ws"], g["y_pitch"], 1, 0), plane(hc, wc, g["c_pitch"], g["c_step"], g["u_offset"]),
            plane(hc, wc, g["c_pitch"], g["c_step"], g["v_offset"]), (csy, csx))


def decimate(dst420, floor, src, layout):
    """The torch pass of route (b): the 4:2:0 copy of 4:2:2 / 4:4:4 frames."""
    y, u, v, (csy, csx) = _planes(src, layout)
    y0, u0, v0, _ = _planes(dst420, floor)
    y0.copy_(y)
    u0.copy_(u[:, ::2 - csy, ::2 - csx])
    v0.copy_(v[:, ::2 - csy, ::2 - csx])


def replicate(dst, layout, src420, floor):
    """The frames of `layout` whose chroma the 4:2:0 frames replicate."""
    y, u, v, (csy, csx) = _planes(dst, layout)
    y0, u0, v0, _ = _planes(src420, floor)
    y.copy_(y0)
    for c, c0 in ((u, u0), (v, v0)):
        c.copy_(c0.repeat_interleave(2 - csy, 1).repeat_interleave(2 - csx, 2))


def run(size, layout, iters, rounds):
    dev = torch.device("cuda")
    hs, ws = GEOMETRY[size]
    floor = FLOOR[layout]
    wide = layout in TR._YUV_WIDE
    n_frames = CLIPS * T
    g = torch.Generator(device="cuda").manual_seed(5)

    def frames(lay):
        x = torch.randint(0, 1024 if wide else 256, (n_frames, _rows(lay, hs), ws), dtype=torch.int16 if wide else torch.uint8,
                          device="cuda", generator=g)
        return x

    videos = [frames(layout) for _ in range(VIDEOS)]
    copies = [torch.empty((n_frames, _rows(floor, hs), ws), dtype=videos[0].dtype, device="cuda") for _ in range(VIDEOS)]
    for c, v in zip(copies, videos):
        decimate(c, floor, v, layout)
    tables = [torch.arange(n_frames).view(CLIPS, T) for _ in range(VIDEOS)]           # every clip its own 16 frames
    n_items = VIDEOS * CLIPS
    scale, shift = TR._affine(MEAN, STD, True, 3, dev)
    lines = []
    for mode, entry in (("bilinear", "pv_batch_views"), ("area", "pv_area_views")):
        outs, descs, keep = [], [], []
        for vids, lay in ((videos, layout), (copies, floor)):
            batch = TR.build_video_batch(vids, tables, lay, SHORT, SIZE, (1,), [T], 3, dev, lambda t: t.to(dev))
            matrix = TR._yuv_matrix_of(("bt709", False), lay).float().reshape(12).to(dev)
            outer = L.AreaViewsDesc() if mode == "area" else L.BatchViewsDesc()
            d = outer.frames.batch if mode == "area" else outer
            if mode == "area":
                outer.filter = L.PV_FILTER_AREA
            TR._batch_launch_fields(d, batch, batch.tables[0], 0, n_items, 3, lay, matrix, (SIZE, SIZE))
            out = torch.empty((n_items, 3, T, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
            d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
            d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
            outs.append(out), descs.append(outer), keep.append((batch, matrix))

        def new():
            _launch(entry, descs[0])

        def floor_launch():
            _launch(entry, descs[1])

        def user_route():
            for c, v in zip(copies, videos):
                decimate(c, floor, v, layout)                    # the chroma decimation, into the buffers (a) reads
            _launch(entry, descs[1])

        # the bit guarantee at this size: the new launch on the replicated frames is the 4:2:0 launch
        saved = [v.clone() for v in videos[:1]]
        replicate(videos[0], layout, copies[0], floor)
        new(), floor_launch()
        torch.cuda.synchronize()
        per_video = CLIPS
        assert torch.equal(outs[0][:per_video], outs[1][:per_video]), "%s %s: the launch on replicated chroma and the 4:2:0 launch differ" % (layout, mode)
        videos[0].copy_(saved[0])
        del saved
        new(), floor_launch(), user_route()
        torch.cuda.synchronize()
        tn, ta, tb = [], [], []
        for _ in range(rounds):
            tn.append(timed(new, iters))
            ta.append(timed(floor_launch, iters))
            tb.append(timed(user_route, max(1, iters // 4)))
        fmt = lambda v: " ".join("%8.4f" % x for x in v)
        spread = (max(ta) - min(ta)) / min(ta)
        lines.append("%dp %s %s, %d items x %d frames -> %d x %d planar bf16; ms per launch, %d interleaved rounds of %d launches" % (
            size, layout, mode, n_items, T, SIZE, SIZE, rounds, iters))
        lines.append("  new     %-14s  %s   min %.4f" % (entry, fmt(tn), min(tn)))
        lines.append("  (a) %-4s launch, 4:2:0 copy %s   min %.4f  (new / (a) %.3fx; spread of (a) between rounds %.1f %%)" % (
            floor, fmt(ta), min(ta), min(tn) / min(ta), 100 * spread))
        lines.append("  (b) torch decimation + (a) %s   min %.4f  ((b) / new %.1fx)" % (fmt(tb), min(tb), min(tb) / min(tn)))
        print("\n".join(lines[-4:]), flush=True)
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="720,1080")
    ap.add_argument("--layouts", default="I422,NV16,I210,I444")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv4.py measures on the GPU; there is none here")
    for s in args.sizes.split(","):
        for layout in args.layouts.split(","):
            run(int(s), layout, args.iters, args.rounds)
            torch.cuda.empty_cache()
