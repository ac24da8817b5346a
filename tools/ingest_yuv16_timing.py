"""Time the whole-video ingest on 10-bit decoder frames (P010 / yuv420p10le) read directly, against the route that existed
before `pv_yuv16_views`: narrow the video to uint8 NV12 in a torch pass, then `pv_yuv_views`.

    python tools/ingest_yuv16_timing.py --out profiles/r15/ingest_yuv16.md

The protocol of tools/ingest_yuv_timing.py (profiles/r9/ingest_yuv.md) on one 300-frame video, at 720 x 1280 and at
1080 x 1920: 10 clips x 3 crops, short side 256, crop 224, `--frames` frames per clip, planar bf16 destination, all 30 items
in ONE launch:

    nv12       pv_yuv_views on 8-bit NV12 frames (1.5 bytes per pixel): the launch the 16-bit one is compared to
    p010       pv_yuv16_views on P010 surfaces (3 bytes per pixel), bt709 limited composed for 10 bits MSB-aligned
    i010       pv_yuv16_views on yuv420p10le frames
    narrowed   the same P010 surfaces narrowed to uint8 NV12 by a torch pass over the WHOLE video (the high byte of every
               sample: one strided copy, timed with events and reported on its own), then pv_yuv_views on the copy

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
STEPS = ("nv12", "p010", "i010", "narrowed")
SIZES = {"720p": (720, 1280), "1080p": (1080, 1920)}


def _span(n_in, n_out, off, n):
    """Source samples [first, last] that destination indices off .. off+n-1 touch (the pinned coordinate, in double)."""
    s = n_in / n_out
    first = int(max(0.0, s * (off + 0.5) - 0.5))
    last = min(int(max(0.0, s * (off + n - 0.5) - 0.5)) + 1, n_in - 1)
    return last - first + 1


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    times.sort()
    return times[len(times) // 2], times[len(times) // 10], times[len(times) * 9 // 10]


def step(args):
    import torch
    from pytorchvideo_amd import _lib as L
    from pytorchvideo_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing can be timed here")
    dev = torch.device("cuda")
    hs, ws = SIZES[args.size]
    n, t, clips, size, crop, views = args.video_frames, args.frames, 10, 256, 224, (0, 1, 2)
    g = torch.Generator(device=dev).manual_seed(7)
    rows = hs * 3 // 2
    pass_times = None
    if args.step == "nv12":
        frames, layout = torch.randint(0, 256, (n, rows, ws), generator=g, dtype=torch.uint8, device=dev), "NV12"
    else:
        raw = torch.randint(0, 256, (n, rows, ws, 2), generator=g, dtype=torch.uint8, device=dev)     # little-endian samples
        if args.step == "i010":
            raw[..., 1] &= 0x03                                  # 10-bit codes in the low bits
            layout = "I010"
        else:
            raw[..., 0] &= 0xC0                                  # 10-bit codes in the high bits
            layout = "P010"
        frames = raw.view(torch.uint16).squeeze(-1)
        if args.step == "narrowed":
            narrow = torch.empty((n, rows, ws), dtype=torch.uint8, device=dev)
            pass_times = _timed(lambda: narrow.copy_(raw[..., 1]), 3, args.pass_reps)           # the whole video, as it must be
            frames, layout = narrow, "NV12"
    starts = torch.linspace(0, n - 2 * t, clips).long()
    table = (starts[:, None] + 2 * torch.arange(t)[None, :]).to(torch.int32).to(dev)          # every other frame of a clip
    hn, wn = TR.scaled_size(hs, ws, size)
    scale, shift = TR._affine((0.45, 0.45, 0.45), (0.225, 0.225, 0.225), True, 3, dev)
    out = torch.empty((clips * len(views), 3, t, crop, crop), dtype=torch.bfloat16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    geom = TR.yuv_geometry(frames, layout)
    m = TR._yuv_matrix_of(("bt709", False), layout).float().reshape(12).to(dev)
    d = TR._yuv_desc(frames, geom, table, m, size, crop, views)
    wide = layout in TR.YUV16_LAYOUTS
    fn, bpp = (L.lib().pv_yuv16_views, 3.0) if wide else (L.lib().pv_yuv_views, 1.5)
    d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16

    def launch():
        status = fn(C.byref(d), stream)
        if status != 0:
            raise SystemExit("%s: status %d" % (args.step, status))

    med, p10, p90 = _timed(launch, args.warmup, args.reps)
    staged = sum(_span(hs, hn, TR.crop_offsets(hn, wn, crop, v)[0], crop) * _span(ws, wn, TR.crop_offsets(hn, wn, crop, v)[1], crop)
                 for v in views) * bpp * clips * t
    written = out.numel() * 2
    res = dict(step=args.step, size=args.size, entry="pv_yuv16_views" if wide else "pv_yuv_views", frames=n, clip_frames=t,
               items=clips * len(views), reps=args.reps, median_us=med * 1e6, p10_us=p10 * 1e6, p90_us=p90 * 1e6,
               staged_bytes=staged, written_bytes=written, gbps=(staged + written) / med / 1e9,
               share_of_copy_ceiling=(staged + written) / med / COPY_CEILING, checksum=float(out.float().sum().item()))
    if pass_times is not None:
        res.update(pass_median_us=pass_times[0] * 1e6, pass_p10_us=pass_times[1] * 1e6, pass_p90_us=pass_times[2] * 1e6,
                   pass_bytes=3 * n * rows * ws)                 # 2 read + 1 written per sample
    print(json.dumps(res))
    with open(args.json, "w") as f:
        json.dump(res, f)


def report(results, path):
    r0 = results[0]
    lines = ["# Ingest of 10-bit YUV 4:2:0 read directly, against narrowing to NV12 first", "",
             "One %d-frame video per geometry, 10 clips x 3 crops of %d frames, short side 256, crop 224, planar bf16 destination,"
             % (r0["frames"], r0["clip_frames"]),
             "all 30 items in one launch; %d timed launches per row after warm-up, events on the stream; MI355X." % r0["reps"],
             "Bytes are counted from the geometry (staged source + written destination); the ceiling is the 6.29 TB/s measured copy.",
             "`narrowed` is the route for the same P010 surfaces without pv_yuv16_views: a torch pass over the whole video (the high",
             "byte of every sample), timed on its own, then pv_yuv_views on the copy; its total is pass + launch.", "",
             "| geometry | source | entry | launch median us | p10 | p90 | staged MB | written MB | GB/s | of ceiling | pass median us | total us | vs nv12 launch |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for size in SIZES:
        rows = [r for r in results if r["size"] == size]
        if not rows:
            continue
        nv12 = next(r for r in rows if r["step"] == "nv12")
        for r in rows:
            p = r.get("pass_median_us")
            lines.append("| %s | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.0f | %.1f %% | %s | %.1f | %.2fx |" % (
                size, r["step"], r["entry"], r["median_us"], r["p10_us"], r["p90_us"], r["staged_bytes"] / 1e6,
                r["written_bytes"] / 1e6, r["gbps"], 100 * r["share_of_copy_ceiling"], "%.1f" % p if p is not None else "-",
                r["median_us"] + (p or 0.0), r["median_us"] / nv12["median_us"]))
        p010 = next(r for r in rows if r["step"] == "p010")
        nar = next(r for r in rows if r["step"] == "narrowed")
        total = nar["median_us"] + nar["pass_median_us"]
        verdicts.append("%s: P010 read directly takes %.1f us; the narrowed route takes %.1f us (pass %.1f + launch %.1f): direct is %s."
                        % (size, p010["median_us"], total, nar["pass_median_us"], nar["median_us"],
                           "NOT slower" if p010["median_us"] <= total else "SLOWER -- the condition of this feature is not met"))
    lines += [""] + verdicts
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="time one source form in this process (what the driver starts)")
    ap.add_argument("--size", choices=tuple(SIZES), default="720p")
    ap.add_argument("--json", help="where a step writes its result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "ingest_yuv16.md"))
    ap.add_argument("--video-frames", type=int, default=300)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pass-reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.step:
        return step(args)
    results = []
    tmp = os.path.splitext(os.path.abspath(args.out))[0]
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    for size in SIZES:
        for s in STEPS:                                          # one fresh process per step; stop at the first failure
            js = "%s_%s_%s.json" % (tmp, size, s)
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s,
                   "--size", size, "--json", js, "--video-frames", str(args.video_frames), "--frames", str(args.frames),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--pass-reps", str(args.pass_reps)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit("step %s %s ended with status %d: nothing more is started" % (size, s, rc))
            results.append(json.load(open(js)))
            os.remove(js)
    report(results, args.out)


if __name__ == "__main__":
    main()
