"""Micro-benchmark of pv_resample_crop (short-side scale + uniform crop fused into the ingest) against the way the same job
is done without it: F.interpolate on a device fp32 view of the clip, the crop slice, then the existing DevicePacker
(pv_ingest_ncdhw) -- both in this process, on the same GPU, warmed up, timed with device events, three interleaved pairs
per geometry (dev tool; needs the MI355X).

    python tools/bench_resample.py [--iters 20] [--no-model]

Byte model of the fused path (what the algorithm has to move): source bytes = the window of the selected source
frames that the crop touches (rows i0y(first) .. i1y(last), columns i0x(first) .. i1x(last), every channel), once per view;
destination bytes = what is written.  Bound = bytes / 6.29 TB/s (the measured float4 copy rate of the MI355X).
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

COPY_RATE = 6.29e12
MEAN, STD = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
# (label, Hs, Ws, short side, crop)
GEOMETRIES = [("256x340->224", 256, 340, 256, 224), ("360x640->256", 360, 640, 256, 256), ("720x1280->224", 720, 1280, 256, 224)]


def _span(n_in, n_out, off, n):
    """Source indices [first, last] that destination indices off .. off+n-1 read (the pinned formula, in fp32)."""
    s = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    r = torch.clamp(s * (torch.tensor([off, off + n - 1], dtype=torch.float32) + 0.5) - 0.5, min=0.0)
    i0 = r.to(torch.int64)
    return int(i0[0]), int(min(i0[1] + 1, n_in - 1))


def byte_model(b, c, frames, hs, ws, size, crop, views, dst_bytes_per_voxel):
    hn, wn = TR.scaled_size(hs, ws, size)
    src = 0
    for v in views:
        y, x = TR.crop_offsets(hn, wn, crop, v)
        y0, y1 = _span(hs, hn, y, crop)
        x0, x1 = _span(ws, wn, x, crop)
        src += b * c * frames * (y1 - y0 + 1) * (x1 - x0 + 1)           # uint8
    return src + b * len(views) * frames * crop * crop * dst_bytes_per_voxel


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_views(clip, size, crop, views):
    """The parent-commit way: an fp32 copy of every scaled frame, sliced per view -> [B*n_views, C, T, crop, crop] fp32."""
    b, c, t, hs, ws = clip.shape
    hn, wn = TR.scaled_size(hs, ws, size)
    scaled = F.interpolate(clip.float().view(b, c * t, hs, ws), size=(hn, wn), mode="bilinear", align_corners=False)
    scaled = scaled.view(b, c, t, hn, wn)
    crops = []
    for v in views:
        y, x = TR.crop_offsets(hn, wn, crop, v)
        crops.append(scaled[:, :, :, y:y + crop, x:x + crop])
    return torch.stack(crops, 1).reshape(b * len(views), c, t, crop, crop)


def _c4(n, t, crop):
    return torch.empty((n, t, crop, crop, 4), dtype=torch.bfloat16, device="cuda")


def _launch(name, d):
    L.check(getattr(L.lib(), name)(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)


def micro(iters):
    print("pv_resample_crop vs F.interpolate (fp32) + crop slice + pv_ingest_ncdhw; uint8 [B,3,T,Hs,Ws], B = 32; both write the "
          "4-channel bf16 first-layer layout [B*views,T,crop,crop,4] with frame selection, Div255 and Normalize; ms per call, "
          "three interleaved pairs")
    print("%-16s %-14s %5s | %27s | %27s | %8s %8s %8s" % ("geometry", "frames", "views", "fused ms (3 runs)", "torch ms (3 runs)",
                                                          "GB model", "TB/s", "of bound"))
    ok = True
    scale = (1.0 / (255.0 * torch.tensor(STD, dtype=torch.float64))).float().cuda()
    shift = (-torch.tensor(MEAN, dtype=torch.float64) / torch.tensor(STD, dtype=torch.float64)).float().cuda()
    for label, hs, ws, size, crop in GEOMETRIES:
        for frames_src, pathways in ((16, (16,)), (32, (8, 32))):
            for views in ((1,), (0, 1, 2)):
                b, n = 32, 32 * len(views)
                clip = torch.randint(0, 256, (b, 3, frames_src, hs, ws), dtype=torch.uint8, device="cuda")
                index = [None if t == frames_src else TR.temporal_indices(frames_src, t).to(torch.int32).cuda() for t in pathways]
                out_f = [_c4(n, t, crop) for t in pathways]
                out_t = [_c4(n, t, crop) for t in pathways]

                def fused():
                    for t, idx, dst in zip(pathways, index, out_f):
                        d = TR._resample_desc(clip, "NCTHW", size, crop, views)
                        if idx is not None:
                            d.T, d.t_index = t, idx.data_ptr()
                        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
                        d.dst, d.dst_layout, d.dst_dtype = dst.data_ptr(), L.DST_NDHWC, L.PV_BF16
                        d.c_p, d.ld, d.bs = 4, 4, t * crop * crop * 4
                        _launch("pv_resample_crop", d)

                def torch_way():
                    x = torch_views(clip, size, crop, views)         # fp32 [B*views, 3, T, crop, crop]
                    for t, idx, dst in zip(pathways, index, out_t):
                        d = L.LayoutDesc()
                        d.src, d.dst = x.data_ptr(), dst.data_ptr()
                        d.B, d.C, d.T, d.H, d.W, d.c_p, d.ld, d.bs = n, 3, t, crop, crop, 4, 4, t * crop * crop * 4
                        d.src_dtype, d.dst_dtype, d.src_T = L.PV_F32, L.PV_BF16, frames_src
                        if idx is not None:
                            d.t_index = idx.data_ptr()
                        d.ch_scale, d.ch_shift = scale.data_ptr(), shift.data_ptr()
                        _launch("pv_ingest_ncdhw", d)

                fused(), torch_way()
                for g_, w_ in zip(out_f, out_t):                     # same job: one bf16 rounding apart at most
                    assert (g_.float() - w_.float()).abs().max().item() <= 2.0 ** -7 * w_.float().abs().max().item() + 2e-3
                for _ in range(2):
                    fused(), torch_way()
                torch.cuda.synchronize()
                tf, tt = [], []
                for _ in range(3):
                    tf.append(timed(fused, iters))
                    tt.append(timed(torch_way, max(2, iters // 4)))
                nbytes = sum(byte_model(b, 3, t, hs, ws, size, crop, views, 4 * 2) for t in pathways)
                rate = nbytes / (min(tf) * 1e-3)
                print("%-16s %-14s %5d | %8.3f %8.3f %8.3f | %8.3f %8.3f %8.3f | %8.3f %8.2f %7.1f%%" % (
                    label, "%d -> %s" % (frames_src, "+".join(str(t) for t in pathways)), len(views), tf[0], tf[1], tf[2],
                    tt[0], tt[1], tt[2], nbytes / 1e9, rate / 1e12, 100.0 * rate / COPY_RATE), flush=True)
                ok = ok and all(f < t for f, t in zip(tf, tt))
                del clip, out_f, out_t
                torch.cuda.empty_cache()
    print("fused faster than the torch path in every pair of every geometry: %s" % ok)
    return ok


def model_rate(steps, warmup):
    """X3D-M (16 x 224 x 224, batch 32, bf16) clips/s through DevicePacker: resampling from 256x340 uint8 against
    pre-cropped 224x224 uint8 -- the end-to-end cost of the new step."""
    from pytorchvideo_amd.accelerator import convert_to_deployable_form, transmute_model
    from pytorchvideo_amd.models import create_x3d
    from pytorchvideo_amd.utils import randomize_norm_stats
    torch.manual_seed(0)
    m = randomize_norm_stats(create_x3d(input_clip_length=16, input_crop_size=224, model_num_class=400), 0).eval()
    transmute_model(m, "mi355x")
    b = 32
    dep = convert_to_deployable_form(m, torch.zeros(b, 3, 16, 224, 224, device="cuda", dtype=torch.bfloat16), dtype=torch.bfloat16)
    raw = torch.randint(0, 256, (b, 3, 16, 256, 340), dtype=torch.uint8, device="cuda")
    cropped = torch.randint(0, 256, (b, 3, 16, 224, 224), dtype=torch.uint8, device="cuda")
    with_rs = TR.DevicePacker(dep, MEAN, STD, div255=True, short_side=256, crop_size=224)
    without = TR.DevicePacker(dep, MEAN, STD, div255=True)
    for name, fn in (("resampled from 256x340 uint8", lambda: with_rs(raw)), ("pre-cropped 224x224 uint8", lambda: without(cropped)),
                     ("resampled from 256x340 uint8", lambda: with_rs(raw)), ("pre-cropped 224x224 uint8", lambda: without(cropped))):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, steps)
        print("X3D-M batch 32 through DevicePacker, %-30s %8.3f ms/step %9.1f clips/s" % (name + ":", ms, b / ms * 1e3), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resample.py measures on the GPU; there is none here")
    ok = micro(a.iters)
    if not a.no_model:
        model_rate(20, 5)
    sys.exit(0 if ok else 1)
