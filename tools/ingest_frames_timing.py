"""Time the frame-list ingest against the one-allocation ingest on the same frames.

    python tools/ingest_frames_timing.py --out profiles/r14/ingest_frames.md

The model-zoo test protocol on one 300-frame 720 x 1280 NV12 video: 10 clips x 3 crops, short side 256, crop 224, `--frames`
frames per clip, planar bf16 destination (what the stems read), all 30 items in ONE launch:

    batch    pv_batch_views on the contiguous video (one record, a constant frame stride)
    frame    pv_frame_views on THE SAME memory expressed as a table of 300 frame addresses

so the two launches stage the same bytes from the same addresses and differ only in how a workgroup finds its frame.  The
steps run in the order batch, frame, batch, frame; the two `batch` rows are the A/A band a difference has to leave.

Every step is a fresh child process under its own `timeout`; the first one that fails ends the run.  A step warms up, then
times `--reps` launches one by one with events on the stream and reports the median and the 10th / 90th percentile, and
the sum of what it wrote (equal in all four rows).  There is no fallback: without a GPU a step fails.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("batch", "frame", "batch", "frame")


def step(args):
    import torch
    from pytorchvideo_amd import _lib as L
    from pytorchvideo_amd import transforms as TR
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing can be timed here")
    dev = torch.device("cuda")
    n, hs, ws, t, clips, size, crop, views = args.video_frames, 720, 1280, args.frames, 10, 256, 224, (0, 1, 2)
    g = torch.Generator(device=dev).manual_seed(7)
    frames = torch.randint(0, 256, (n, hs * 3 // 2, ws), generator=g, dtype=torch.uint8, device=dev)
    starts = torch.linspace(0, n - 2 * t, clips).long()
    table = (starts[:, None] + 2 * torch.arange(t)[None, :]).to(torch.int32)                  # every other frame of a clip
    matrix = TR.yuv_matrix("bt709", False).float().reshape(12).to(dev)
    scale, shift = TR._affine((0.45, 0.45, 0.45), (0.225, 0.225, 0.225), True, 3, dev)
    out = torch.empty((clips * len(views), 3, t, crop, crop), dtype=torch.bfloat16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    video = TR.FrameList(frames.unbind(0), "NV12") if args.step == "frame" else frames
    b = TR.build_video_batch([video], [table], "NV12", size, crop, views, [t], 3, dev, lambda x: x.to(dev))
    f = L.FrameViewsDesc()
    d = f.batch
    d.sources, d.sources_dev = C.addressof(b.sources), b.sources_dev.data_ptr()
    d.items, d.items_dev = C.addressof(b.items), b.items_dev.data_ptr()
    d.t_index, d.n_rows, d.t_stride = b.tables[0].data_ptr(), b.tables[0].shape[0], b.tables[0].stride(0)
    d.n_sources, d.n_items, d.C, d.T = 1, b.total, 3, t
    d.src_dtype, d.src_layout, d.c_step, d.yuv2rgb = L.PV_U8, L.SRC_YUV420, 2, matrix.data_ptr()
    d.Ho, d.Wo, d.n_views = crop, crop, len(views)
    d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
    if args.step == "frame":
        f.frame_ptrs, f.frame_ptrs_dev, f.n_frame_ptrs = b.frame_ptrs.data_ptr(), b.frame_ptrs_dev.data_ptr(), n
        assert b.frame_ptrs.tolist() == [frames.data_ptr() + i * frames.stride(0) for i in range(n)]
        fn, desc, entry = L.lib().pv_frame_views, f, "pv_frame_views"
    else:
        fn, desc, entry = L.lib().pv_batch_views, d, "pv_batch_views"

    def launch():
        status = fn(C.byref(desc), stream)
        if status != 0:
            raise SystemExit("%s: status %d" % (entry, status))

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        e.record()
        e.synchronize()
        times.append(a.elapsed_time(e) * 1e-3)
    times.sort()
    med, p10, p90 = times[len(times) // 2], times[len(times) // 10], times[len(times) * 9 // 10]
    res = dict(step=args.step, entry=entry, frames=n, clip_frames=t, items=b.total, reps=args.reps, median_us=med * 1e6,
               p10_us=p10 * 1e6, p90_us=p90 * 1e6, checksum=float(out.float().sum().item()))
    print(json.dumps(res))
    with open(args.json, "w") as fh:
        json.dump(res, fh)


def report(results, path):
    r0 = results[0]
    batch = [r["median_us"] for r in results if r["step"] == "batch"]
    frame = [r["median_us"] for r in results if r["step"] == "frame"]
    lo, hi = min(batch), max(batch)

    def where(m):
        return "inside" if lo <= m <= hi else "%.1f %% %s it" % (100 * (m - hi) / hi if m > hi else 100 * (lo - m) / lo,
                                                               "above" if m > hi else "below")

    lines = ["# Frame-list ingest against the one-allocation ingest, same frames, same addresses", "",
             "One %d-frame 720 x 1280 NV12 video, 10 clips x 3 crops of %d frames, short side 256, crop 224, planar bf16 destination,"
             % (r0["frames"], r0["clip_frames"]),
             "all %d items in one launch; %d timed launches per row after warm-up, events on the stream; MI355X; one fresh process"
             % (r0["items"], r0["reps"]),
             "per row, in this order.  `pv_frame_views` reads the contiguous video through a table of its frame addresses.", "",
             "| run | entry | median us | p10 | p90 | checksum |", "|---|---|---|---|---|---|"]
    for i, r in enumerate(results):
        lines.append("| %d | %s | %.1f | %.1f | %.1f | %.6g |" % (i, r["entry"], r["median_us"], r["p10_us"], r["p90_us"], r["checksum"]))
    lines += ["", "A/A band of `pv_batch_views` (its two medians): %.1f .. %.1f us.  `pv_frame_views` medians: %s."
              % (lo, hi, "; ".join("%.1f us, %s" % (m, where(m)) for m in frame)),
              "Checksums equal: %s." % (len({r["checksum"] for r in results}) == 1)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=("batch", "frame"), help="time one entry point in this process (what the driver starts)")
    ap.add_argument("--json", help="where a step writes its result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "ingest_frames.md"))
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
    for i, s in enumerate(STEPS):                                # one fresh process per step; stop at the first failure
        js = "%s_%d_%s.json" % (tmp, i, s)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s, "--json", js,
               "--video-frames", str(args.video_frames), "--frames", str(args.frames), "--warmup", str(args.warmup),
               "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing more is started" % (s, rc))
        results.append(json.load(open(js)))
        os.remove(js)
    report(results, args.out)


if __name__ == "__main__":
    main()
