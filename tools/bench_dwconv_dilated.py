"""Timing of the dilated depthwise / channel-wise grouped conv (csrc/pv_dwconv.hip: the polyphase form of dw3_plane_kernel for
depthwise bf16, dwconv_kernel<T, 0, 1, 1> for 2 / 4 / 8 channels per group), one op at a time.

    python tools/bench_dwconv_dilated.py [--out FILE.md] [--iters 20] [--rounds 7] [--batch 8] [--frames 8]

The shapes are the res5 conv_b of an ir-CSN-style detection backbone: 16 x 16 planes, C 1024 and 2048, kernel (3,3,3), stride 1,
dilation (1,2,2), "same" padding, BatchNorm + ReLU epilogue, bf16.  Every shape is emitted three times into a one-op Session:

  new        emit_conv with tuning "dwconv_dilated" on: a pv_dwconv3d with the dilation in its descriptor
  dense      what ran before that existed: the dense pv_conv3d with block-diagonal weights.  For gw 4 that is emit_conv with the
             key off; for gw 1 the emitter declined the conv, so the same block-diagonal dense conv is built here by hand
  undilated  the same filter at dilation 1 / padding 1 on the same kernel family: what the dilation costs

and the three plans are profiled alternately in one process (pv_plan_profile: HIP events around the op).  Times are the median
over the rounds with the min .. max spread; GB/s is on the algorithmic bytes (each input and output voxel once).  new and dense
are compared on the same seeded input."""
import argparse
import statistics
import sys

import torch
import torch.nn as nn

from pytorchvideo_amd.accelerator.mi355x import emit, tuning
from pytorchvideo_amd.accelerator.mi355x.session import Session

SHAPES = [(1024, 1), (2048, 1), (1024, 4), (2048, 4)]       # (C, channels per group)
K, DIL, HW = (3, 3, 3), (1, 2, 2), 16


def one_op(conv, bn, shape, key_on, seed=1):
    tuning.OPTIONS["dwconv_dilated"] = key_on
    try:
        sess = Session(dtype=torch.bfloat16)
        x = sess.alloc_act(*shape)
        y = emit.emit_conv(sess, conv, x, norm=bn, act=emit.L.ACT_RELU, label="conv_b")
        sess.finalize()
    finally:
        tuning.OPTIONS["dwconv_dilated"] = True
    g = torch.Generator().manual_seed(seed)
    sess.view(x).copy_(torch.randn(sess.view(x).shape, generator=g).to(torch.bfloat16))
    return sess, y


def block_diagonal(conv):
    """The dense nn.Conv3d that computes the grouped `conv` (zeros outside the groups' blocks)."""
    C, gw = conv.out_channels, conv.in_channels // conv.groups
    dense = nn.Conv3d(C, C, conv.kernel_size, conv.stride, conv.padding, conv.dilation, bias=False)
    with torch.no_grad():
        dense.weight.zero_()
        for g in range(conv.groups):
            dense.weight[g * gw:(g + 1) * gw, g * gw:(g + 1) * gw] = conv.weight[g * gw:(g + 1) * gw]
    return dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dwconv_dilated needs the GPU: no timing is taken without one")
    rows = ["| C | gw | new kernel | new ms (min .. max) | dense ms (min .. max) | dense / new | undilated kernel | undilated ms (min .. max) "
            "| new / undilated | new GB/s | max rel diff new vs dense |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for C, gw in SHAPES:
        torch.manual_seed(C + gw)
        conv = nn.Conv3d(C, C, K, padding=tuple(k // 2 * d for k, d in zip(K, DIL)), dilation=DIL, groups=C // gw, bias=False)
        with torch.no_grad():
            conv.weight.mul_((gw * 27) ** -0.5 / conv.weight.std())
        bn = nn.BatchNorm3d(C).eval()
        shape = (a.batch, a.frames, HW, HW, C)
        new, y_new = one_op(conv, bn, shape, True)
        dense, y_dense = one_op(conv, bn, shape, False) if gw > 1 else one_op(block_diagonal(conv), bn, shape, True)
        plain = nn.Conv3d(C, C, K, padding=1, groups=C // gw, bias=False)
        plain.weight = conv.weight
        und, _ = one_op(plain, bn, shape, True)
        assert new.ops[0][0] == und.ops[0][0] == emit.L.OP_DWCONV3D and new.ops[0][2]["dil_h"] == 2
        assert dense.ops[0][0] == emit.L.OP_CONV3D and dense.ops[0][2]["groups"] == 0
        plans = (new, dense, und)
        for sess in plans:      # warm-up: code objects, clocks
            sess.profile(3)
        times = [[], [], []]
        for _ in range(a.rounds):
            for t, sess in zip(times, plans):
                t.append(sess.profile(a.iters)[0][2])
        new.launch()
        dense.launch()
        torch.cuda.synchronize()
        got, ref = new.view(y_new).float(), dense.view(y_dense).float()
        assert ref.abs().max().item() > 1.0 and (got != 0).float().mean().item() > 0.25, "the op did not see the seeded input"
        diff = ((got - ref).abs().max() / ref.abs().max()).item()
        med = [statistics.median(t) for t in times]
        cell = ["%.4f (%.4f .. %.4f)" % (m, min(t), max(t)) for m, t in zip(med, times)]
        alg = new.profile(1)[0][3]
        rows.append("| %d | %d | %s | %s | %s | %.2f | %s | %s | %.2f | %.0f | %.1e |" % (
            C, gw, new.op_kernels[0], cell[0], cell[1], med[1] / med[0], und.op_kernels[0], cell[2], med[0] / med[2],
            alg / med[0] * 1e-6, diff))
        print(rows[-1], flush=True)
        del new, dense, und, plans
        torch.cuda.empty_cache()
    text = ("Batch %d, T = %d, %d x %d, kernel 3x3x3, dilation (1,2,2), bf16, BatchNorm + ReLU epilogue; median (min .. max) of %d "
            "rounds x %d launches, the three plans alternating.\n\n" % (a.batch, a.frames, HW, HW, a.rounds, a.iters)) + "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
