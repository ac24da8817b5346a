"""A/B of the grouped conv kernels (csrc/pv_gconv.hip, csrc/pv_gconv_wide.hip) against the block-diagonal dense route, one op
at a time.

    python tools/bench_gconv.py [--out FILE.md] [--iters 20] [--rounds 5] [--batch 16] [--min-gw 64]

Every shape is emitted twice through emit_conv into a one-op bf16 Session -- tuning "grouped_conv" on (compact weights,
gconv_plane_kernel / gconv_wide_kernel) and off (block-diagonal weights on the dense GEMM route) -- and the two plans are profiled
alternately in the same process (pv_plan_profile: HIP events around the op).  Times are the median over the rounds;
TFLOP/s and TB/s are on the GROUPED FLOP count and the algorithmic bytes (each input voxel, the compact filter and each
output voxel once) for both routes, so the columns compare like with like.  The outputs of the two routes are compared
on the same seeded input."""
import argparse
import statistics
import sys

import torch
import torch.nn as nn

from pytorchvideo_amd.accelerator.mi355x import emit, tuning
from pytorchvideo_amd.accelerator.mi355x.session import Session

#          C    gw  H=W  spatial stride
SHAPES = [(512, 16, 14, 1), (512, 16, 28, 2), (1024, 32, 7, 1), (1024, 32, 14, 2),
          (64, 16, 56, 1), (128, 16, 28, 1), (256, 16, 14, 1), (512, 16, 7, 1),
          # ResNeXt-101 32x8d res5 / 32x16d res4 (2048 channels, 64 per group), 32x16d res5 (4096, 128 per group)
          (2048, 64, 14, 1), (2048, 64, 14, 2), (2048, 64, 7, 1), (4096, 128, 14, 2), (4096, 128, 7, 1)]
KERNELS = [(3, 3, 3), (1, 3, 3)]


def one_op(conv, bn, shape, grouped, seed):
    tuning.OPTIONS["grouped_conv"] = grouped
    sess = Session(dtype=torch.bfloat16)
    x = sess.alloc_act(*shape)
    y = emit.emit_conv(sess, conv, x, norm=bn, act=emit.L.ACT_RELU, label="conv_b")
    sess.finalize()
    g = torch.Generator().manual_seed(seed)
    sess.view(x).copy_(torch.randn(sess.view(x).shape, generator=g).to(torch.bfloat16))
    return sess, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--min-gw", type=int, default=0, help="only the shapes with at least this many channels per group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gconv needs the GPU: no timing is taken without one")
    rows = ["| C | gw | kernel | in -> out | grouped kernel | grouped ms | dense ms | dense / grouped | grouped TFLOP/s | grouped TB/s | dense TFLOP/s | max rel diff |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for C, gw, hw, s in [sh for sh in SHAPES if sh[1] >= a.min_gw]:
        for k in KERNELS:
            torch.manual_seed(C + k[0])
            conv = nn.Conv3d(C, C, k, stride=(1, s, s), padding=tuple(v // 2 for v in k), groups=C // gw, bias=False)
            with torch.no_grad():
                conv.weight.mul_((gw * k[0] * 9) ** -0.5 / conv.weight.std())
            bn = nn.BatchNorm3d(C).eval()
            shape = (a.batch, a.frames, hw, hw, C)
            on, y_on = one_op(conv, bn, shape, True, 1)
            off, y_off = one_op(conv, bn, shape, False, 1)
            assert on.ops[0][2]["groups"] == C // gw and off.ops[0][2]["groups"] == 0
            for sess in (on, off):      # warm-up: code objects, clocks
                sess.profile(3)
            t_on, t_off = [], []
            for _ in range(a.rounds):
                t_on.append(on.profile(a.iters)[0][2])
                t_off.append(off.profile(a.iters)[0][2])
            on.launch()
            off.launch()
            torch.cuda.synchronize()
            got, ref = on.view(y_on).float(), off.view(y_off).float()
            assert ref.abs().max().item() > 1.0 and (got != 0).float().mean().item() > 0.25, "the op did not see the seeded input"
            diff = ((got - ref).abs().max() / ref.abs().max()).item()
            ms_on, ms_off = statistics.median(t_on), statistics.median(t_off)
            _, _, _, alg, flops = on.profile(1)[0]
            ho = on.ops[0][2]["Ho"]
            rows.append("| %d | %d | %dx%dx%d | %d -> %d | %s | %.4f | %.4f | %.2f | %.1f | %.2f | %.1f | %.1e |" % (
                C, gw, k[0], k[1], k[2], hw, ho, on.op_kernels[0], ms_on, ms_off, ms_off / ms_on, flops / ms_on * 1e-9,
                alg / ms_on * 1e-9, flops / ms_off * 1e-9, diff))
            print(rows[-1], flush=True)
            del on, off
            torch.cuda.empty_cache()
    text = ("Batch %d, T = %d, bf16, BatchNorm + ReLU epilogue; median of %d rounds x %d launches, the two plans alternating.\n\n"
            % (a.batch, a.frames, a.rounds, a.iters)) + "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
