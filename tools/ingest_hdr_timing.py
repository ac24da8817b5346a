"""Time the whole-video ingest on PQ / HLG P010 frames converted to SDR per tap (`pv_hdr_views`), against the route that
existed before it: a torch pass on the device that turns the WHOLE P010 video into SDR RGB, then the RGB ingest.

    python tools/ingest_hdr_timing.py --out profiles/r19/hdr_ingest_timing.md

(profiles/r19/hdr_ingest.md holds that table, with the accuracy figures behind it.)

The protocol of tools/ingest_yuv16_timing.py (profiles/r15/ingest_yuv16.md) on one 300-frame P010 video, at 720 x 1280 and at
1080 x 1920: 10 clips x 3 crops, short side 256, crop 224, `--frames` frames per clip, planar bf16 destination, all 30 items
in ONE launch:

    plain      pv_yuv16_views on the P010 surfaces, hdr=None: the launch the HDR ones are compared to
    pq         pv_hdr_views, PV_TRANSFER_PQ, the default tone table, the video as one upright record
    hlg        pv_hdr_views, PV_TRANSFER_HLG
    turned     pv_hdr_views, PQ, the record under orient = 1 (a quarter turn: the tile kernels); 720p only
    prepass    the route the parent commit offers for the same result: the whole video through the arithmetic of the header's
               "HDR sources" in torch on the device (fp32, frames in chunks of `--chunk`, the result rounded to a uint8
               [N,H,W,3] video -- the cheapest form for that route), timed with events and reported on its own, then
               pv_video_views on the copy

Every step is a fresh child process under its own `timeout`; the first one that fails ends the run.  A step warms up, then
times `--reps` launches one by one with events on the stream and reports the median and the 10th / 90th percentile.  The
condition is one of kind: the direct launch must not take longer than pass + launch.  The ratio to the plain P010 launch is
reported as it comes out.  There is no fallback: without a GPU a step fails.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("plain", "pq", "hlg", "turned", "prepass")
SIZES = {"720p": (720, 1280), "1080p": (1080, 1920)}


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


def sdr_pass(frames, hs, matrix, tone, out, chunk):
    """P010 frames [N, Hs*3/2, Ws] (uint16) -> `out` uint8 [N, Hs, Ws, 3]: the tap rule and the PQ map of the header in fp32
    torch operators, `chunk` frames at a time."""
    import torch
    from pytorchvideo_amd import transforms as TR
    m, t = matrix.reshape(3, 4), tone
    for i0 in range(0, frames.shape[0], chunk):
        f = frames[i0:i0 + chunk].view(torch.int16).to(torch.float32)
        f = torch.where(f < 0, f + 65536.0, f)                   # the codes, unsigned
        y = f[:, :hs]
        uv = f[:, hs:].reshape(f.shape[0], hs // 2, -1, 2).repeat_interleave(2, 1).repeat_interleave(2, 2)
        e = [torch.clamp(m[c, 0] * y + m[c, 1] * uv[..., 0] + m[c, 2] * uv[..., 1] + m[c, 3], 0.0, 255.0) / 255.0 for c in range(3)]
        lin = []
        for c in range(3):
            p = e[c] ** (1.0 / TR._PQ_M2)
            lin.append((torch.clamp(p - TR._PQ_C1, min=0.0) / (TR._PQ_C2 - TR._PQ_C3 * p)) ** (1.0 / TR._PQ_M1) * t[0])
        mx = torch.maximum(torch.maximum(lin[0], lin[1]), lin[2])
        safe = torch.where(mx > t[2], mx, torch.ones_like(mx))
        k = torch.where(mx > t[2], t[3] * (safe + t[4]) / ((safe + t[5]) * safe), torch.ones_like(mx))
        lin = [v * k for v in lin]
        for c in range(3):
            g = torch.clamp(t[6 + 3 * c] * lin[0] + t[7 + 3 * c] * lin[1] + t[8 + 3 * c] * lin[2], 0.0, 1.0)
            v = torch.where(g < TR._OETF_BETA, 4.5 * g, TR._OETF_ALPHA * g ** 0.45 - (TR._OETF_ALPHA - 1.0))
            out[i0:i0 + chunk, ..., c] = (255.0 * v + 0.5).to(torch.uint8)


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
    raw = torch.randint(0, 256, (n, rows, ws, 2), generator=g, dtype=torch.uint8, device=dev)         # little-endian samples
    raw[..., 0] &= 0xC0                                          # 10-bit codes in the high bits
    frames = raw.view(torch.uint16).squeeze(-1)
    starts = torch.linspace(0, n - 2 * t, clips).long()
    table_cpu = (starts[:, None] + 2 * torch.arange(t)[None, :]).to(torch.int32)                     # every other frame of a clip
    table = table_cpu.to(dev)
    scale, shift = TR._affine((0.45, 0.45, 0.45), (0.225, 0.225, 0.225), True, 3, dev)
    out = torch.empty((clips * len(views), 3, t, crop, crop), dtype=torch.bfloat16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m = TR._yuv_matrix_of(("bt2020", False), "P010").float().reshape(12).to(dev)
    transfer = "hlg" if args.step == "hlg" else "pq"
    tone = TR.tone_params(transfer).to(dev)
    pass_times, keep = None, []
    if args.step == "plain":
        d = TR._yuv_desc(frames, TR.yuv_geometry(frames, "P010"), table, m, size, crop, views)
        fn, entry, desc = L.lib().pv_yuv16_views, "pv_yuv16_views", d
    elif args.step == "prepass":
        video = torch.empty((n, hs, ws, 3), dtype=torch.uint8, device=dev)
        pass_times = _timed(lambda: sdr_pass(frames, hs, m, tone, video, args.chunk), 1, args.pass_reps)   # the whole video, as it must be
        d = TR._rgb_source(L.VideoViewsDesc(), video, "NTHWC", 3, hs, ws, TR._view_geometry(hs, ws, size, crop, views), crop)
        d.t_index, d.n_clips, d.T, d.N, d.t_stride = table.data_ptr(), clips, t, n, table.stride(0)
        fn, entry, desc = L.lib().pv_video_views, "pv_video_views", d
    else:
        batch = TR.build_video_batch([frames], [table_cpu], "P010", size, crop, views, [t], 3, dev, lambda x: x.to(dev),
                                     orientation=1 if args.step == "turned" else 0)
        keep.append(batch)
        h = L.HdrViewsDesc()
        d = h.frames.batch
        d.sources, d.sources_dev = C.addressof(batch.sources), batch.sources_dev.data_ptr()
        d.items, d.items_dev = C.addressof(batch.items), batch.items_dev.data_ptr()
        tab = batch.tables[0]
        d.t_index, d.n_rows, d.t_stride = tab.data_ptr(), tab.shape[0], tab.stride(0)
        d.n_sources, d.n_items, d.C, d.T = 1, batch.total, 3, t
        d.src_layout, d.src_dtype, d.c_step, d.yuv2rgb = L.SRC_YUV420, L.PV_U16, 2, m.data_ptr()
        d.Ho, d.Wo, d.n_views = crop, crop, len(views)
        h.tone, h.transfer = tone.data_ptr(), (L.TRANSFER_HLG if transfer == "hlg" else L.TRANSFER_PQ)
        fn, entry, desc = L.lib().pv_hdr_views, "pv_hdr_views", h
    d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
    d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16

    def launch():
        status = fn(C.byref(desc), stream)
        if status != 0:
            raise SystemExit("%s: status %d" % (args.step, status))

    med, p10, p90 = _timed(launch, args.warmup, args.reps)
    res = dict(step=args.step, size=args.size, entry=entry, frames=n, clip_frames=t, items=clips * len(views), reps=args.reps,
               median_us=med * 1e6, p10_us=p10 * 1e6, p90_us=p90 * 1e6, checksum=float(out.float().sum().item()))
    if pass_times is not None:
        res.update(pass_median_us=pass_times[0] * 1e6, pass_p10_us=pass_times[1] * 1e6, pass_p90_us=pass_times[2] * 1e6,
                   pass_reps=args.pass_reps)
    print(json.dumps(res))
    with open(args.json, "w") as f:
        json.dump(res, f)


def report(results, path):
    r0 = results[0]
    lines = ["# Ingest of PQ / HLG P010 video converted to SDR per tap, against a colour pass over the video first", "",
             "One %d-frame P010 video per geometry, 10 clips x 3 crops of %d frames, short side 256, crop 224, planar bf16 destination,"
             % (r0["frames"], r0["clip_frames"]),
             "all 30 items in one launch; %d timed launches per row after warm-up, events on the stream, a fresh process per row; MI355X."
             % r0["reps"],
             "`prepass` is the route for the same result without pv_hdr_views: the whole video through the same arithmetic in torch on",
             "the device (fp32, result rounded to a uint8 [N,H,W,3] video), timed on its own, then pv_video_views on the copy; its total",
             "is pass + launch.  `turned` is the PQ launch on the record under orient = 1 (the tile kernels).", "",
             "| geometry | row | entry | launch median us | p10 | p90 | pass median us | total us | vs plain P010 launch |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for size in SIZES:
        rows = [r for r in results if r["size"] == size]
        if not rows:
            continue
        plain = next(r for r in rows if r["step"] == "plain")
        for r in rows:
            p = r.get("pass_median_us")
            lines.append("| %s | %s | %s | %.1f | %.1f | %.1f | %s | %.1f | %.2fx |" % (
                size, r["step"], r["entry"], r["median_us"], r["p10_us"], r["p90_us"], "%.1f" % p if p is not None else "-",
                r["median_us"] + (p or 0.0), r["median_us"] / plain["median_us"]))
        pre = next(r for r in rows if r["step"] == "prepass")
        total = pre["median_us"] + pre["pass_median_us"]
        for name in ("pq", "hlg"):
            r = next(x for x in rows if x["step"] == name)
            verdicts.append("%s %s: converted per tap the launch takes %.1f us (+%.1f us on the plain P010 launch); the pass route takes "
                            "%.1f us (pass %.1f + launch %.1f): direct is %s."
                            % (size, name, r["median_us"], r["median_us"] - plain["median_us"], total, pre["pass_median_us"],
                               pre["median_us"], "NOT slower" if r["median_us"] <= total else "SLOWER -- the condition of this feature is not met"))
    lines += [""] + verdicts
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="time one row in this process (what the driver starts)")
    ap.add_argument("--size", choices=tuple(SIZES), default="720p")
    ap.add_argument("--json", help="where a step writes its result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "hdr_ingest_timing.md"))
    ap.add_argument("--video-frames", type=int, default=300)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.step:
        return step(args)
    results = []
    tmp = os.path.splitext(os.path.abspath(args.out))[0]
    os.makedirs(os.path.dirname(tmp), exist_ok=True)
    for size in SIZES:
        for s in STEPS:                                          # one fresh process per step; stop at the first failure
            if s == "turned" and size != "720p":
                continue
            js = "%s_%s_%s.json" % (tmp, size, s)
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s,
                   "--size", size, "--json", js, "--video-frames", str(args.video_frames), "--frames", str(args.frames),
                   "--warmup", str(args.warmup), "--reps", str(args.reps), "--pass-reps", str(args.pass_reps),
                   "--chunk", str(args.chunk)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                raise SystemExit("step %s %s ended with status %d: nothing more is started" % (size, s, rc))
            results.append(json.load(open(js)))
            os.remove(js)
    report(results, args.out)


if __name__ == "__main__":
    main()
