"""Time the item-sourced ingest on videos stored turned or mirrored (`pv_view_source.orient`), against the copy it replaces,
and show that upright launches cost what they cost before (dev tool; needs the MI355X).

    python tools/bench_orient.py --out profiles/r17/orient_ingest.md [--parent-lib /path/to/the/parent's/libpv_mi355x.so]

The case is the launch of DESIGN.md 4.9: one 300-frame video, 10 clips x 3 crops of 16 frames (every other frame of a clip),
short side 256, crop 224, planar bf16 destination, all 30 items in ONE `pv_batch_views` launch; at 720 x 1280 and at
1080 x 1920, NV12 and NTHWC.

    upright    the launch with every record's orient = 0.  With --parent-lib the same step also runs against the parent
               commit's library (PV_MI355X_LIB), parent and this commit alternating P T P T P in one session: the spread of the
               parent's own repeats is what a difference has to beat.
    turned c   in ONE process, for code c (1: a quarter turn, 4: mirrored):
                 A  the launch on the stored video with orient = c;
                 B  what a caller does without it: index_select of exactly the distinct frames the launch reads, rot90 / flip
                    (YUV: the Y and the interleaved UV plane each), one dense copy into a buffer kept from call to call, then
                    the upright launch on the copy -- timed as one region;
                 C  the upright launch alone on a copy made beforehand: the same geometry without the turn;
                 A' A again.  The outputs of A and C are compared bit for bit before anything is timed.

Every step is a fresh child process under its own `timeout`; the first one that fails ends the run.  A step warms up, then
times `--windows` windows of `--calls` back-to-back launches each between two events on the stream and reports the per-launch
median, minimum and maximum over the windows.  There is no fallback: without a GPU a step fails.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"720p": (720, 1280), "1080p": (1080, 1920)}
FORMS = ("NV12", "NTHWC")
CLIPS, SIZE, CROP, VIEWS = 10, 256, 224, (0, 1, 2)


def _windows(fn, warmup, windows, calls):
    """Per-call seconds: (median, min, max) over `windows` windows of `calls` calls between two events."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e-3 / calls)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


class Launch:
    """One pv_batch_views launch of all 30 items of one video (`orient` in its record) into a planar bf16 destination."""

    def __init__(self, video, form, table, t, orient):
        import torch
        from pytorchvideo_amd import _lib as L
        from pytorchvideo_amd import transforms as TR
        dev = video.device
        self.batch = TR.build_video_batch([video], [table.cpu()], form, SIZE, CROP, VIEWS, [t], 3, dev, lambda x: x.to(dev),
                                          orientation=orient)
        self.out = torch.empty((CLIPS * len(VIEWS), 3, t, CROP, CROP), dtype=torch.bfloat16, device=dev)
        self.affine = TR._affine((0.45, 0.45, 0.45), (0.225, 0.225, 0.225), True, 3, dev)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        b, d = self.batch, L.BatchViewsDesc()
        d.sources, d.sources_dev = C.addressof(b.sources), b.sources_dev.data_ptr()
        d.items, d.items_dev = C.addressof(b.items), b.items_dev.data_ptr()
        tab = b.tables[0]
        d.t_index, d.n_rows, d.t_stride = tab.data_ptr(), tab.shape[0], tab.stride(0)
        d.n_sources, d.n_items, d.C, d.T = 1, b.total, 3, t
        d.src_layout, d.src_dtype = TR._src_codes(form, torch.uint8)
        if form == "NV12":
            self.matrix = TR._yuv_matrix_of(("bt709", False), form).float().reshape(12).to(dev)
            d.c_step, d.yuv2rgb = 2, self.matrix.data_ptr()
        d.Ho, d.Wo, d.n_views = CROP, CROP, len(VIEWS)
        d.ch_scale, d.ch_shift = self.affine[0].data_ptr(), self.affine[1].data_ptr()
        d.dst, d.dst_layout, d.dst_dtype = self.out.data_ptr(), L.DST_NCTHW, L.PV_BF16
        self.d, self.fn = d, L.lib().pv_batch_views

    def __call__(self):
        status = self.fn(C.byref(self.d), self.stream)
        if status != 0:
            raise SystemExit("pv_batch_views: status %d" % status)


def _video(form, hs, ws, n, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    shape = (n, hs * 3 // 2, ws) if form == "NV12" else (n, hs, ws, 3)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8, device=dev)


def _turned_copy(video, form, hs, distinct, code, out=None):
    """index_select of the frames the launch reads, rot90 / flip, one dense copy -- into `out` when given, which spares the
    route an allocation and a new record: the cheapest route without `orient`."""
    import torch
    from pytorchvideo_amd import transforms as TR
    sel = video.index_select(0, distinct)
    if form != "NV12":
        turned = TR.oriented(sel, code, 1, 2)
        return turned.contiguous() if out is None else out.copy_(turned)
    n, ws = sel.shape[0], sel.shape[2]
    y = TR.oriented(sel[:, :hs], code, 1, 2)
    uv = TR.oriented(sel[:, hs:].view(n, hs // 2, ws // 2, 2), code, 1, 2)
    if out is None:
        out = torch.empty((n, y.shape[1] * 3 // 2, y.shape[2]), dtype=torch.uint8, device=video.device)
    out[:, :y.shape[1]].copy_(y)
    out[:, y.shape[1]:].view(n, uv.shape[1], uv.shape[2], 2).copy_(uv)
    return out


def step(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing can be timed here")
    dev = torch.device("cuda")
    hs, ws = SIZES[args.size]
    n, t = args.video_frames, args.frames
    video = _video(args.form, hs, ws, n, dev)
    starts = torch.linspace(0, n - 2 * t, CLIPS).long()
    table = (starts[:, None] + 2 * torch.arange(t)[None, :]).to(torch.int32)                   # every other frame of a clip
    timing = (args.warmup, args.windows, args.calls)
    res = dict(step=args.step, form=args.form, size=args.size, code=args.code, lib=os.environ.get("PV_MI355X_LIB") or "this commit",
               windows=args.windows, calls=args.calls)
    if args.step == "upright":
        launch = Launch(video, args.form, table, t, 0)
        res["upright_us"] = [x * 1e6 for x in _windows(launch, *timing)]
        res["checksum"] = float(launch.out.float().sum().item())
    else:
        distinct, inverse = torch.unique(table, return_inverse=True)
        distinct_dev, compact = distinct.to(dev), inverse.to(torch.int32)
        a = Launch(video, args.form, table, t, args.code)
        copy = _turned_copy(video, args.form, hs, distinct_dev, args.code)
        c = Launch(copy, args.form, compact, t, 0)
        a()
        c()
        torch.cuda.synchronize()
        same = torch.equal(a.out.view(torch.int16), c.out.view(torch.int16))
        if not same:
            raise SystemExit("code %d: the oriented launch and the launch on the pre-oriented copy differ" % args.code)

        def route_b():
            _turned_copy(video, args.form, hs, distinct_dev, args.code, copy)
            c()

        res["distinct_frames"] = int(distinct.numel())
        res["oriented_us"] = [x * 1e6 for x in _windows(a, *timing)]
        res["copy_then_upright_us"] = [x * 1e6 for x in _windows(route_b, args.warmup, args.windows, max(1, args.calls // 8))]
        res["upright_on_copy_us"] = [x * 1e6 for x in _windows(c, *timing)]
        res["oriented_again_us"] = [x * 1e6 for x in _windows(a, *timing)]
        res["bits_equal"] = same
        tile = a.batch.sources[0]
        res["stored"], res["displayed_scaled"] = [tile.Hs, tile.Ws], [tile.Hn, tile.Wn]
    print(json.dumps(res))
    with open(args.json, "w") as f:
        json.dump(res, f)


def _fmt(v):
    return "%.1f (%.1f .. %.1f)" % tuple(v)


def report(results, path, parent):
    lines = ["# Orientation in the item-sourced ingest: upright launches against the parent, turned launches against the copy", "",
             "One 300-frame video per case, 10 clips x 3 crops of 16 frames, short side 256, crop 224, planar bf16 destination, all 30",
             "items in one `pv_batch_views` launch; per-launch microseconds: median (minimum .. maximum) over %d windows of %d back-to-back"
             % (results[0]["windows"], results[0]["calls"]),
             "launches between two events, after warm-up; every step a fresh process; MI355X.", ""]
    ups = [r for r in results if r["step"] == "upright"]
    if ups:
        lines += ["## Upright launches (orient = 0 everywhere)", "", "| size | source | library | per launch us |", "|---|---|---|---|"]
        for r in ups:
            lines.append("| %s | %s | %s | %s |" % (r["size"], r["form"], "parent" if r["lib"] != "this commit" else "this commit", _fmt(r["upright_us"])))
        lines.append("")
        for size in SIZES:
            for form in FORMS:
                p = [r["upright_us"][0] for r in ups if (r["size"], r["form"]) == (size, form) and r["lib"] != "this commit"]
                t = [r["upright_us"][0] for r in ups if (r["size"], r["form"]) == (size, form) and r["lib"] == "this commit"]
                if p and t:
                    diff, spread = sum(t) / len(t) - sum(p) / len(p), max(p) - min(p)
                    lines.append("%s %s: parent medians %s us (spread %.2f), this commit %s us: the means differ by %+.2f us; this commit is %s."
                                 % (size, form, ", ".join("%.1f" % x for x in p), spread, ", ".join("%.1f" % x for x in t), diff,
                                    "not slower than the parent by more than the parent's own spread" if diff <= spread
                                    else "SLOWER than the parent by more than the parent's own spread"))
        if not parent:
            lines.append("No parent library was given: only this commit was timed.")
        lines.append("")
    turned = [r for r in results if r["step"] == "turned"]
    if turned:
        lines += ["## Turned launches against the copy they replace", "",
                  "A: orient = code on the stored video.  B: index_select of the distinct frames, rot90 / flip, dense copy, upright launch.",
                  "C: the upright launch alone on a copy made beforehand.  A and C write the same bits (checked in every step).", "",
                  "| size | source | code | distinct frames | A us | A again us | B us | C us | A / B | A / C |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in turned:
            a = min(r["oriented_us"][0], r["oriented_again_us"][0])
            worst = max(r["oriented_us"][0], r["oriented_again_us"][0])
            lines.append("| %s | %s | %d | %d | %s | %s | %s | %s | %.3f | %.2f |" % (
                r["size"], r["form"], r["code"], r["distinct_frames"], _fmt(r["oriented_us"]), _fmt(r["oriented_again_us"]),
                _fmt(r["copy_then_upright_us"]), _fmt(r["upright_on_copy_us"]), worst / r["copy_then_upright_us"][0],
                a / r["upright_on_copy_us"][0]))
        lines.append("")
        for r in turned:
            worst = max(r["oriented_us"][0], r["oriented_again_us"][0])
            lines.append("%s %s code %d: the oriented launch (%.1f us, the slower of A and A') is %s than the copy route (%.1f us)."
                         % (r["size"], r["form"], r["code"], worst,
                            "FASTER" if worst < r["copy_then_upright_us"][1] else "NOT faster", r["copy_then_upright_us"][0]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=("upright", "turned"), help="time one case in this process (what the driver starts)")
    ap.add_argument("--form", choices=FORMS, default="NV12")
    ap.add_argument("--size", choices=tuple(SIZES), default="720p")
    ap.add_argument("--code", type=int, default=0)
    ap.add_argument("--json", help="where a step writes its result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "orient_ingest.md"))
    ap.add_argument("--parent-lib", default=None, help="libpv_mi355x.so built from the parent commit")
    ap.add_argument("--codes", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--video-frames", type=int, default=300)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=120)
    args = ap.parse_args()
    if args.step:
        return step(args)
    results = []
    tmp = os.path.splitext(os.path.abspath(args.out))[0]
    os.makedirs(os.path.dirname(tmp), exist_ok=True)

    def run(step_name, form, size, code, lib):
        js = "%s_step.json" % tmp
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step_name,
               "--form", form, "--size", size, "--code", str(code), "--json", js, "--video-frames", str(args.video_frames),
               "--frames", str(args.frames), "--warmup", str(args.warmup), "--windows", str(args.windows), "--calls", str(args.calls)]
        env = dict(os.environ)
        env.pop("PV_MI355X_LIB", None)
        if lib:
            env["PV_MI355X_LIB"] = lib
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            raise SystemExit("step %s %s %s code %d ended with status %d: nothing more is started" % (step_name, form, size, code, rc))
        results.append(json.load(open(js)))
        os.remove(js)

    for size in SIZES:
        for form in FORMS:
            libs = [args.parent_lib, None, args.parent_lib, None, args.parent_lib] if args.parent_lib else [None, None]
            for lib in libs:                                     # parent and this commit alternate
                run("upright", form, size, 0, lib)
            for code in args.codes:
                run("turned", form, size, code, None)
    report(results, args.out, args.parent_lib)


if __name__ == "__main__":
    main()
