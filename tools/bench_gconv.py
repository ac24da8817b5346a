"""A/B of the grouped conv kernels (csrc/pv_gconv.hip, csrc/pv_gconv_wide.hip) against the block-diagonal dense route, one op
at a time.

    python tools/bench_gconv.py [--out FILE.md] [--iters 20] [--rounds 5] [--batch 16] [--min-gw 64] [--dilated]

Every shape is emitted twice through emit_conv into a one-op bf16 Session -- tuning "grouped_conv" on (compact weights,
gconv_plane_kernel / gconv_wide_kernel) and off (block-diagonal weights on the dense GEMM route) -- and the two plans are profiled
alternately in the same process (pv_plan_profile: HIP events around the op).  Times are the median over the rounds;
TFLOP/s and TB/s are on the GROUPED FLOP count and the algorithmic bytes (each input voxel, the compact filter and each
output voxel once) for both routes, so the columns compare like with like.  The outputs of the two routes are compared
on the same seeded input.

--dilated: the res5 conv_b of a detection backbone instead -- kernel (1,3,3), stride 1, dilation (1,2,2), 16 x 16 planes -- with
tuning "grouped_conv_dilated" on (the polyphase form of the grouped kernels) and off (the dense route, which is what the
library ran before that form existed), and a third plan: the same shape UNDILATED on the grouped kernel, which shows what the
phase split costs."""
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
DILATED = [(1024, 32, 16, 1), (512, 16, 16, 1), (2048, 64, 16, 1), (4096, 128, 16, 1)]


def one_op(conv, bn, shape, grouped, seed, key="grouped_conv"):
    tuning.OPTIONS[key] = grouped
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
    ap.add_argument("--dilated", action="store_true", help="dilated (1,2,2) res5 shapes; A/B on tuning grouped_conv_dilated")
    a = ap.parse_args()
    dil, key = ((1, 2, 2), "grouped_conv_dilated") if a.dilated else ((1, 1, 1), "grouped_conv")
    if not torch.cuda.is_available():
        sys.exit("bench_gconv needs the GPU: no timing is taken without one")
    rows = ["| C | gw | kernel | in -> out | grouped kernel | grouped ms | dense ms | dense / grouped | grouped TFLOP/s | grouped TB/s | dense TFLOP/s | max rel diff |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    if a.dilated:
        rows = [rows[0] + " undilated grouped ms |", rows[1] + "---|"]
    for C, gw, hw, s in [sh for sh in (DILATED if a.dilated else SHAPES) if sh[1] >= a.min_gw]:
        for k in (KERNELS[1:] if a.dilated else KERNELS):
            torch.manual_seed(C + k[0])
            conv = nn.Conv3d(C, C, k, stride=(1, s, s), padding=tuple(v // 2 * e for v, e in zip(k, dil)), dilation=dil,
                             groups=C // gw, bias=False)
            with torch.no_grad():
                conv.weight.mul_((gw * k[0] * 9) ** -0.5 / conv.weight.std())
            bn = nn.BatchNorm3d(C).eval()
            shape = (a.batch, a.frames, hw, hw, C)
            on, y_on = one_op(conv, bn, shape, True, 1, key)
            off, y_off = one_op(conv, bn, shape, False, 1, key)
            tuning.OPTIONS[key] = True
            assert on.ops[0][2]["groups"] == C // gw and off.ops[0][2]["groups"] == 0
            und = None
            if a.dilated:   # same shape, same weights, dilation 1
                plain = nn.Conv3d(C, C, k, padding=tuple(v // 2 for v in k), groups=C // gw, bias=False)
                plain.weight = conv.weight
                und = one_op(plain, bn, shape, True, 1)[0]
                assert und.ops[0][2]["groups"] == C // gw
            for sess in (on, off) + ((und,) if und else ()):      # warm-up: code objects, clocks
                sess.profile(3)
            t_on, t_off, t_und = [], [], []
            for _ in range(a.rounds):
                t_on.append(on.profile(a.iters)[0][2])
                t_off.append(off.profile(a.iters)[0][2])
                if und:
                    t_und.append(und.profile(a.iters)[0][2])
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
                alg / ms_on * 1e-9, flops / ms_off * 1e-9, diff) + (" %.4f |" % statistics.median(t_und) if und else ""))
            print(rows[-1], flush=True)
            del on, off, und
            torch.cuda.empty_cache()
    text = ("Batch %d, T = %d, bf16, BatchNorm + ReLU epilogue; median of %d rounds x %d launches, the two plans alternating.\n\n"
            % (a.batch, a.frames, a.rounds, a.iters)) + "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
