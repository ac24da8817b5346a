"""Time the whole-video ingest on decoder-native frames against the RGB copy of the same frames.

    python tools/ingest_yuv_timing.py --out profiles/r9/ingest_yuv.md [--rgb-lib PATH]

The model-zoo test protocol on one 300-frame 720 x 1280 video: 10 clips x 3 crops, short side 256, crop 224, `--frames`
frames per clip, planar bf16 destination (what the stems read), all 30 items in ONE launch:

    nv12, i420   pv_yuv_views on the frames as a decoder hands them out (1.5 bytes per pixel)
    rgb          pv_video_views on the uint8 [N,H,W,3] copy of the same frames (3 bytes per pixel) -- from `--rgb-lib`, a
                 libpv_mi355x.so built from the commit to compare against, when given; else from this tree's library

Every step is a fresh child process under its own `timeout`; the first one that fails ends the run.  A step warms up, then
times `--reps` launches one by one with events on the stream and reports the median and the 10th / 90th percentile.  Bytes
are counted from the geometry: what the kernel stages (per view and frame: source rows x source columns of the crop
window x bytes per pixel) plus what it writes.  There is no fallback: without a GPU a step fails.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12        # measured-copy ceiling DESIGN.md uses, bytes / s
STEPS = ("nv12", "i420", "rgb")


def _span(n_in, n_out, off, n):
    """Source samples [first, last] that destination indices off .. off+n-1 touch (the pinned coordinate, in double)."""
    s = n_in / n_out
    first = int(max(0.0, s * (off + 0.5) - 0.5))
    last = min(int(max(0.0, s * (off + n - 0.5) - 0.5)) + 1, n_in - 1)
    return last - first + 1


def step(args):
    import torch
    from pytorchvideo_amd import _lib as L
    from pytorchvideo_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing can be timed here")
    dev = torch.device("cuda")
    n, hs, ws, t, clips, size, crop, views = args.video_frames, 720, 1280, args.frames, 10, 256, 224, (0, 1, 2)
    layout = {"nv12": "NV12", "i420": "I420", "rgb": "NV12"}[args.step]
    g = torch.Generator(device=dev).manual_seed(7)
    frames = torch.randint(0, 256, (n, hs * 3 // 2, ws), generator=g, dtype=torch.uint8, device=dev)
    starts = torch.linspace(0, n - 2 * t, clips).long()
    table = (starts[:, None] + 2 * torch.arange(t)[None, :]).to(torch.int32).to(dev)          # every other frame of a clip
    hn, wn = TR.scaled_size(hs, ws, size)
    scale, shift = TR._affine((0.45, 0.45, 0.45), (0.225, 0.225, 0.225), True, 3, dev)
    out = torch.empty((clips * len(views), 3, t, crop, crop), dtype=torch.bfloat16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if args.step == "rgb":
        m = TR.yuv_matrix("bt709", False).float().to(dev)
        rgb = torch.empty((n, hs, ws, 3), dtype=torch.uint8, device=dev)
        for i in range(0, n, 20):                                # the copy a user would have had to make
            f = frames[i:i + 20].float()
            c = f[:, hs:].reshape(-1, hs // 2, ws // 2, 2).repeat_interleave(2, 1).repeat_interleave(2, 2)
            yuv1 = torch.stack([f[:, :hs], c[..., 0], c[..., 1], torch.ones_like(f[:, :hs])], dim=-1)
            rgb[i:i + 20] = torch.clamp(yuv1 @ m.t(), 0, 255).round().to(torch.uint8)
        del frames
        lib = L.lib()
        which = "this tree"
        if args.rgb_lib:
            lib = C.CDLL(args.rgb_lib)
            lib.pv_video_views.restype, lib.pv_version.restype = C.c_int, C.c_int
            lib.pv_video_views.argtypes = [C.POINTER(L.VideoViewsDesc), C.c_void_p]
            which = "%s (ABI %d)" % (os.path.basename(os.path.dirname(args.rgb_lib)) or args.rgb_lib, lib.pv_version())
        d = L.VideoViewsDesc()
        d.src, d.t_index = rgb.data_ptr(), table.data_ptr()
        d.n_clips, d.C, d.T, d.N, d.t_stride, d.Hs, d.Ws = clips, 3, t, n, table.stride(0), hs, ws
        d.src_dtype, d.src_layout = L.PV_U8, L.SRC_NTHWC
        d.Hn, d.Wn, d.Ho, d.Wo, d.n_views = hn, wn, crop, crop, len(views)
        for i, v in enumerate(views):
            d.y_off[i], d.x_off[i] = TR.crop_offsets(hn, wn, crop, v)
        fn, bpp = lib.pv_video_views, 3.0
    else:
        geom = TR.yuv_geometry(frames, layout)
        m = TR.yuv_matrix("bt709", False).float().reshape(12).to(dev)
        d = TR._yuv_desc(frames, geom, table, m, size, crop, views)
        fn, bpp, which = L.lib().pv_yuv_views, 1.5, "this tree"
    d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16

    def launch():
        status = fn(C.byref(d), stream)
        if status != 0:
            raise SystemExit("%s: status %d" % (args.step, status))

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    times.sort()
    med, p10, p90 = times[len(times) // 2], times[len(times) // 10], times[len(times) * 9 // 10]
    staged = sum(_span(hs, hn, TR.crop_offsets(hn, wn, crop, v)[0], crop) * _span(ws, wn, TR.crop_offsets(hn, wn, crop, v)[1], crop)
                 for v in views) * bpp * clips * t
    written = out.numel() * 2
    res = dict(step=args.step, library=which, frames=n, clip_frames=t, items=clips * len(views), reps=args.reps,
               median_us=med * 1e6, p10_us=p10 * 1e6, p90_us=p90 * 1e6, staged_bytes=staged, written_bytes=written,
               gbps=(staged + written) / med / 1e9, share_of_copy_ceiling=(staged + written) / med / COPY_CEILING,
               checksum=float(out.float().sum().item()))
    print(json.dumps(res))
    with open(args.json, "w") as f:
        json.dump(res, f)


def report(results, path):
    rgb = next(r for r in results if r["step"] == "rgb")
    lines = ["# Ingest of decoder-native YUV 4:2:0 against the RGB copy", "",
             "One %d-frame 720 x 1280 video, 10 clips x 3 crops of %d frames, short side 256, crop 224, planar bf16 destination,"
             % (rgb["frames"], rgb["clip_frames"]),
             "all 30 items in one launch; %d timed launches per row after warm-up, events on the stream; MI355X." % rgb["reps"],
             "Bytes are counted from the geometry (staged source + written destination); the ceiling is the 6.29 TB/s measured copy.", "",
             "| source | entry | library | median us | p10 | p90 | staged MB | written MB | GB/s | of ceiling | vs rgb |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f | %.1f %% | %.2fx |" % (
            r["step"], "pv_video_views" if r["step"] == "rgb" else "pv_yuv_views", r["library"], r["median_us"], r["p10_us"],
            r["p90_us"], r["staged_bytes"] / 1e6, r["written_bytes"] / 1e6, r["gbps"], 100 * r["share_of_copy_ceiling"],
            rgb["median_us"] / r["median_us"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="time one source form in this process (what the driver starts)")
    ap.add_argument("--json", help="where a step writes its result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "ingest_yuv.md"))
    ap.add_argument("--rgb-lib", default=None, help="libpv_mi355x.so of the commit whose pv_video_views is the RGB row")
    ap.add_argument("--video-frames", type=int, default=300)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--step-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        return step(args)
    results = []
    tmp = os.path.splitext(os.path.abspath(args.out))[0]
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    for s in STEPS:                                              # one fresh process per step; stop at the first failure
        js = "%s_%s.json" % (tmp, s)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s, "--json", js,
               "--video-frames", str(args.video_frames), "--frames", str(args.frames), "--warmup", str(args.warmup),
               "--reps", str(args.reps)] + (["--rgb-lib", args.rgb_lib] if args.rgb_lib else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing more is started" % (s, rc))
        results.append(json.load(open(js)))
        os.remove(js)
    report(results, args.out)


if __name__ == "__main__":
    main()
