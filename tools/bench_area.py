"""Micro-benchmark of pv_area_views (the box filter of interpolation="area" inside the ingest launch) on the job it was built
for: the 30-item launch of a dataset evaluation -- 3 videos x 10 clips of 16 frames, short side to 256, centre crop 224,
Div255 + Normalize, written as the planar bf16 clip a stem reads -- from 720p, 1080p and 2160p sources, as the decoder's
[N,H,W,3] uint8 and as NV12 (dev tool; needs the MI355X).

    python tools/bench_area.py [--iters 20] [--rounds 3] [--sizes 720,1080,2160]

Every clip has 16 frames of its own (160 frames a video: 1.3 GB of 720p RGB, 12 GB of 2160p), so a launch reads far more than
the 256 MB last-level cache holds and no round finds its source there.  In this process, on the same GPU, warmed up, timed with
device events (the method of tools/bench_regions.py), `--rounds` interleaved rounds of:
  area      the pv_area_views launch
  bilinear  the pv_batch_views launch of the same items (what the filter costs: it reads 4 taps where area reads the window)
  torch     the route a user has without it: per clip the frames gathered, an fp32 copy, F.interpolate(mode="area") of the
            whole frames, the crop, the affine map and the bf16 [3, T, 224, 224] layout; for NV12 the conversion of
            `transforms.yuv420_to_rgb` first, written with device ops as a user would.
Achieved bytes/s of the area launch: the source footprint of the windows read once (every source pixel under the crop's window,
3 or 1.5 bytes a pixel) plus the destination, over the time.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
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


def nv12_to_rgb(frames, m, hs, ws):
    """`transforms.yuv420_to_rgb` of tight NV12 frames [n, Hs*3/2, Ws] with device ops: fp32 [n, 3, Hs, Ws], clamped."""
    n = frames.shape[0]
    y = frames[:, :hs].float()
    uv = frames[:, hs:].reshape(n, hs // 2, ws // 2, 2).float()
    u, v = [uv[..., k].repeat_interleave(2, 1).repeat_interleave(2, 2) for k in (0, 1)]
    rgb = torch.stack([m[c, 0] * y + m[c, 1] * u + m[c, 2] * v + m[c, 3] for c in range(3)], 1)
    return rgb.clamp_(0.0, 255.0)


def footprint(hs, ws, hn, wn, y0, x0):
    """Source pixels under the SIZE x SIZE window at (y0, x0) of the scaled frame: the header's windows, first start to last end."""
    rows = ((y0 + SIZE) * hs + hn - 1) // hn - (y0 * hs) // hn
    cols = ((x0 + SIZE) * ws + wn - 1) // wn - (x0 * ws) // wn
    return rows * cols


def run(size, layout, iters, rounds, with_torch=True):
    dev = torch.device("cuda")
    hs, ws = GEOMETRY[size]
    yuv = layout == "NV12"
    n_frames = CLIPS * T
    g = torch.Generator(device="cuda").manual_seed(5)
    shape = (n_frames, hs * 3 // 2, ws) if yuv else (n_frames, hs, ws, 3)
    videos = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for _ in range(VIDEOS)]
    tables = [torch.arange(n_frames).view(CLIPS, T) for _ in range(VIDEOS)]           # every clip its own 16 frames
    n_items = VIDEOS * CLIPS
    matrix = TR.yuv_matrix("bt709", False)
    matrix_dev = matrix.float().reshape(12).to(dev) if yuv else None
    scale, shift = TR._affine(MEAN, STD, True, 3, dev)
    out_area = torch.empty((n_items, 3, T, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
    out_bil, out_torch = torch.empty_like(out_area), torch.empty_like(out_area)

    def destination(d, out):
        d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()

    batch = TR.build_video_batch(videos, tables, layout, SHORT, SIZE, (1,), [T], 3, dev, lambda t: t.to(dev))
    a = L.AreaViewsDesc()
    a.filter = L.PV_FILTER_AREA
    TR._batch_launch_fields(a.frames.batch, batch, batch.tables[0], 0, n_items, 3, layout, matrix_dev, (SIZE, SIZE))
    destination(a.frames.batch, out_area)
    b = L.BatchViewsDesc()
    TR._batch_launch_fields(b, batch, batch.tables[0], 0, n_items, 3, layout, matrix_dev, (SIZE, SIZE))
    destination(b, out_bil)
    m_dev = matrix.float().to(dev)
    sc, sh = scale.view(3, 1, 1, 1), shift.view(3, 1, 1, 1)
    hn, wn = TR.scaled_size(hs, ws, SHORT)
    y0, x0 = TR.crop_offsets(hn, wn, SIZE, 1)

    def area():
        _launch("pv_area_views", a)

    def bilinear():
        _launch("pv_batch_views", b)

    def torch_route():
        i = 0
        for video, table in zip(videos, tables):
            for k in range(CLIPS):
                idx = table[k].to(dev)
                if yuv:
                    x = nv12_to_rgb(video[idx], m_dev, hs, ws).permute(1, 0, 2, 3)      # [3, T, Hs, Ws] fp32: the RGB copy
                else:
                    x = video[idx].permute(3, 0, 1, 2).float()
                x = F.interpolate(x, size=(hn, wn), mode="area")[:, :, y0:y0 + SIZE, x0:x0 + SIZE]
                out_torch[i] = (x * sc + sh).to(torch.bfloat16)
                i += 1

    area(), bilinear(), torch_route()
    torch.cuda.synchronize()
    worst = (out_area.float() - out_torch.float()).abs().max().item()
    assert worst <= 2.0 ** -7 * out_torch.float().abs().max().item() + 2e-3, worst     # the same job: a bf16 rounding apart at most
    area(), bilinear()
    torch.cuda.synchronize()
    ta, tb, tt = [], [], []
    for _ in range(rounds):
        ta.append(timed(area, iters))
        tb.append(timed(bilinear, iters))
        tt.append(timed(torch_route, 1) if with_torch else float("nan"))
    px = 1.5 if yuv else 3.0
    src = n_items * T * footprint(hs, ws, hn, wn, y0, x0) * px
    dst = out_area.numel() * 2
    fmt = lambda v: " ".join("%8.4f" % x for x in v)
    print("%dp %s, %d items x %d frames -> %d x %d planar bf16; ms per launch, %d interleaved rounds of %d launches" % (
        size, layout, n_items, T, SIZE, SIZE, rounds, iters))
    print("  pv_area_views            %s   min %.4f  (source footprint %.1f MB, destination %.1f MB: %.2f TB/s at min)" % (
        fmt(ta), min(ta), src / 1e6, dst / 1e6, (src + dst) / (min(ta) * 1e-3) / 1e12))
    print("  bilinear pv_batch_views  %s   min %.4f  (area / bilinear %.2fx)" % (fmt(tb), min(tb), min(ta) / min(tb)))
    print("  torch route              %s   min %.4f  (torch / area %.1fx; outputs agree to %.2e)" % (
        fmt(tt), min(tt), min(tt) / min(ta), worst), flush=True)
    return not with_torch or min(ta) < min(tt)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="720,1080,2160")
    ap.add_argument("--skip-torch", action="store_true", help="time the two launches only (the torch route still runs once: the outputs are compared)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_area.py measures on the GPU; there is none here")
    results = [run(int(s), layout, args.iters, args.rounds, not args.skip_torch) for s in args.sizes.split(",") for layout in ("NTHWC", "NV12")]
    sys.exit(0 if all(results) else 1)
