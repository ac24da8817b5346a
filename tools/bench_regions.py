"""Micro-benchmark of pv_region_views (a rectangle of the frame per destination frame, resized inside the ingest launch) on the
job it was built for: 30 actor tubes of about 200 x 400 pixels from three 720p videos -- two key frames a video, five people a
key frame, clips of 16 frames -- resized to 224 x 224, Div255 + Normalize, written as the planar bf16 clip a stem reads
(dev tool; needs the MI355X).

    python tools/bench_regions.py [--iters 50] [--rounds 5]

Against, in this process, on the same GPU, warmed up, timed with device events (the method of tools/bench_resample.py),
`--rounds` interleaved rounds:
  (a) the torch route it replaces: per tube the crop of the clip's frames, F.interpolate(bilinear) on an fp32 copy, the affine
      map and the bf16 [3, T, 224, 224] layout; for NV12 the conversion of `transforms.yuv420_to_rgb` first -- written with
      device ops here, once per clip, as a user would --, which is the RGB copy the ingest avoids;
  (b) a same-session pv_batch_views launch of 30 FULL-FRAME views of the same videos through the same frame table
      (short side 256, centre crop 224).  The region launch reads no more source than (b): its time should not be above (b)'s
      by more than the run-to-run spread of (b) seen in this session; the tool prints both and says which it is.
Source bytes are counted from the shapes: every pixel of every rectangle (region), every pixel of the crop's window (b).
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
HS, WS, N, T, SIZE = 720, 1280, 48, 16, 224
VIDEOS, KEYS, PEOPLE = 3, 2, 5


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def tubes(even):
    """Per video the frame table [KEYS * PEOPLE, T] and the rectangles [KEYS * PEOPLE, T, 4]: a person's box of about
    200 x 400, static over the clip (the torch route then needs one crop and one interpolate per tube, its best case)."""
    g = torch.Generator().manual_seed(21)
    tables, regions = [], []
    for _ in range(VIDEOS):
        rows, rects = [], []
        for k in range(KEYS):
            frames = k * 24 + torch.arange(T)
            for _ in range(PEOPLE):
                w, h = 200 + int(torch.randint(-30, 31, (1,), generator=g)), 400 + int(torch.randint(-60, 61, (1,), generator=g))
                x1, y1 = float(torch.rand(1, generator=g)) * (WS - w), float(torch.rand(1, generator=g)) * (HS - h)
                rows.append(frames)
                rects.append(TR.box_regions(torch.tensor([x1, y1, x1 + w, y1 + h]), HS, WS, even=even).expand(T, 4))
        tables.append(torch.stack(rows))
        regions.append(torch.stack(rects))
    return tables, regions


def _launch(name, d):
    L.check(getattr(L.lib(), name)(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def nv12_to_rgb(frames, m):
    """`transforms.yuv420_to_rgb` of tight NV12 frames [n, Hs*3/2, Ws] with device ops: fp32 [n, 3, Hs, Ws], clamped."""
    n = frames.shape[0]
    y = frames[:, :HS].float()
    uv = frames[:, HS:].reshape(n, HS // 2, WS // 2, 2).float()
    u, v = [uv[..., k].repeat_interleave(2, 1).repeat_interleave(2, 2) for k in (0, 1)]
    rgb = torch.stack([m[c, 0] * y + m[c, 1] * u + m[c, 2] * v + m[c, 3] for c in range(3)], 1)
    return rgb.clamp_(0.0, 255.0)


def run(layout, iters, rounds):
    dev = torch.device("cuda")
    yuv = layout == "NV12"
    g = torch.Generator(device="cuda").manual_seed(5)
    shape = (N, HS * 3 // 2, WS) if yuv else (N, HS, WS, 3)
    videos = [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for _ in range(VIDEOS)]
    tables, regions = tubes(yuv)
    n_items = VIDEOS * KEYS * PEOPLE
    matrix = TR.yuv_matrix("bt709", False)
    matrix_dev = matrix.float().reshape(12).to(dev) if yuv else None
    scale, shift = TR._affine(MEAN, STD, True, 3, dev)
    up = lambda t: t.to(dev)
    out_r = torch.empty((n_items, 3, T, SIZE, SIZE), dtype=torch.bfloat16, device=dev)
    out_b, out_a = torch.empty_like(out_r), torch.empty_like(out_r)

    def destination(d, out):
        d.dst, d.dst_layout, d.dst_dtype = out.data_ptr(), L.DST_NCTHW, L.PV_BF16
        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()

    rb = TR.build_video_batch(videos, tables, layout, None, (SIZE, SIZE), (1,), [T], 3, dev, up, regions=regions)
    r = L.RegionViewsDesc()
    TR._batch_launch_fields(r.frames.batch, rb, rb.tables[0], 0, n_items, 3, layout, matrix_dev, (SIZE, SIZE))
    r.regions, r.regions_dev = rb.regions[0].data_ptr(), rb.regions_dev[0].data_ptr()
    destination(r.frames.batch, out_r)
    fb = TR.build_video_batch(videos, tables, layout, 256, SIZE, (1,), [T], 3, dev, up)
    b = L.BatchViewsDesc()
    TR._batch_launch_fields(b, fb, fb.tables[0], 0, n_items, 3, layout, matrix_dev, (SIZE, SIZE))
    destination(b, out_b)
    m_dev = matrix.float().to(dev)
    sc, sh = scale.view(3, 1, 1, 1), shift.view(3, 1, 1, 1)

    def region():
        _launch("pv_region_views", r)

    def full_frames():
        _launch("pv_batch_views", b)

    def torch_route():
        i = 0
        for video, table, rects in zip(videos, tables, regions):
            for k in range(KEYS):
                idx = table[k * PEOPLE].to(dev)
                clip = nv12_to_rgb(video[idx], m_dev) if yuv else None          # [T, 3, Hs, Ws] fp32: the RGB copy
                for p in range(PEOPLE):
                    top, left, h, w = rects[k * PEOPLE + p, 0].tolist()
                    if yuv:
                        x = clip[:, :, top:top + h, left:left + w].permute(1, 0, 2, 3)
                    else:
                        x = video[idx, top:top + h, left:left + w].permute(3, 0, 1, 2).float()
                    x = F.interpolate(x, size=(SIZE, SIZE), mode="bilinear", align_corners=False)
                    out_a[i] = (x * sc + sh).to(torch.bfloat16)
                    i += 1

    region(), full_frames(), torch_route()
    torch.cuda.synchronize()
    worst = (out_r.float() - out_a.float()).abs().max().item()
    assert worst <= 2.0 ** -7 * out_a.float().abs().max().item() + 2e-3, worst       # the same job: a bf16 rounding apart at most
    for _ in range(2):
        region(), full_frames(), torch_route()
    torch.cuda.synchronize()
    tr, tb, ta = [], [], []
    for _ in range(rounds):
        tr.append(timed(region, iters))
        tb.append(timed(full_frames, iters))
        ta.append(timed(torch_route, max(2, iters // 10)))
    px = 1.5 if yuv else 3.0
    src_r = sum(int(rg[:, :, 2].mul(rg[:, :, 3]).sum()) for rg in regions) * px
    hn, wn = TR.scaled_size(HS, WS, 256)
    src_b = n_items * T * (SIZE * HS / hn) * (SIZE * WS / wn) * px
    dst = out_r.numel() * 2
    fmt = lambda v: " ".join("%7.4f" % x for x in v)
    print("%s, %d tubes x %d frames -> %d x %d planar bf16; ms per launch, %d interleaved rounds of %d launches" % (
        layout, n_items, T, SIZE, SIZE, rounds, iters))
    print("  pv_region_views          %s   min %.4f  (source %.1f MB, destination %.1f MB: %.2f TB/s at min)" % (
        fmt(tr), min(tr), src_r / 1e6, dst / 1e6, (src_r + dst) / (min(tr) * 1e-3) / 1e12))
    print("  (b) pv_batch_views       %s   min %.4f  (source %.1f MB window, 30 full-frame views)" % (fmt(tb), min(tb), src_b / 1e6))
    print("  (a) torch route          %s   min %.4f" % (fmt(ta), min(ta)))
    spread = max(tb) - min(tb)
    med = lambda v: sorted(v)[len(v) // 2]
    over = med(tr) - med(tb)
    print("  region vs (b): median %.4f vs %.4f ms (%+.4f); run-to-run spread of (b) %.4f ms -> %s" % (
        med(tr), med(tb), over, spread, "within the spread of (b) or faster" if over <= spread else "SLOWER than (b) by more than its spread"))
    print("  region vs (a): %.1fx faster (min over min); outputs agree to %.2e" % (min(ta) / min(tr), worst), flush=True)
    return over <= spread


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_regions.py measures on the GPU; there is none here")
    results = [run(layout, a.iters, a.rounds) for layout in ("NTHWC", "NV12")]
    sys.exit(0 if all(results) else 1)
