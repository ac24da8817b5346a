"""The non-local block in a launch plan (csrc/pv_nlattn.hip, emit.emit_nonlocal) against the torch module, one block at a time.

    python tools/bench_nonlocal.py [--out FILE.md] [--iters 20] [--rounds 5] [--batch 8]

Every shape is emitted through emit_nonlocal into a one-block bf16 Session.  The block is timed the same way on both routes:
HIP events around `iters` back-to-back forwards -- eager replays of the plan (launch gaps included) against the torch module
(what a model runs when the block is declined: bf16, same device, einsums that store the Nq x Nk matrix).  The attention op
alone comes from pv_plan_profile (events around the op).  The routes alternate in the same process; times are the median
over the rounds, the spread is (max - min) / median.  TFLOP/s of the attention op are on 4 B Nq Nk Ci FLOP.  The outputs
of the two routes are compared on the same seeded input."""
import argparse
import statistics
import sys

import torch

from pytorchvideo_amd import _lib as L
from pytorchvideo_amd.accelerator.mi355x import emit
from pytorchvideo_amd.accelerator.mi355x.session import Session
from pytorchvideo_amd.layers import create_nonlocal

#          dim_in  Ci   T  H=W  pool          (res3 and res4 of an 8-frame 224^2 clip)
SHAPES = [(512, 256, 8, 28, (1, 2, 2)), (1024, 512, 8, 14, (1, 2, 2))]


def timed_ms(forward, iters):
    """(ms per call, last result) of `iters` back-to-back calls between two events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        start.record()
        for _ in range(iters):
            y = forward()
        stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nonlocal needs the GPU: no timing is taken without one")
    rows = ["| Ci | Nq | Nk | mode | attention ms (spread) | attention TFLOP/s | block ms, plan (spread) | block ms, torch (spread) | torch / plan | max rel diff |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for dim_in, ci, T, hw, pool in SHAPES:
        for inst in ("softmax", "dot_product"):
            torch.manual_seed(ci)
            m = create_nonlocal(dim_in=dim_in, dim_inner=ci, pool_size=pool, instantiation=inst).eval()
            with torch.no_grad():
                m.norm.weight.uniform_(0.5, 1.5)
                m.norm.running_var.uniform_(0.5, 1.5)
            sess = Session(dtype=torch.bfloat16)
            x = sess.alloc_act(a.batch, T, hw, hw, dim_in)
            y = emit.emit_nonlocal(sess, m, x)
            sess.finalize()
            xin = sess.view(x)
            xin.copy_(torch.randn(xin.shape, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16))
            mt = m.to(device=sess.device, dtype=torch.bfloat16)
            att = [i for i, op in enumerate(sess.ops) if op[0] == L.OP_NONLOCAL][0]
            sess.profile(3)
            timed_ms(lambda: mt(xin), 3)
            timed_ms(sess.launch, 3)
            t_att, t_plan, t_torch = [], [], []
            for _ in range(a.rounds):
                t_att.append(sess.profile(a.iters)[att][2])
                t_plan.append(timed_ms(sess.launch, a.iters)[0])
                t_torch.append(timed_ms(lambda: mt(xin), a.iters)[0])
            ref = timed_ms(lambda: mt(xin), 1)[1].float()
            sess.launch()
            torch.cuda.synchronize()
            got = sess.view(y).float()
            diff = ((got - ref).abs().max() / ref.abs().max()).item()

            def med(t):
                return statistics.median(t), (max(t) - min(t)) / statistics.median(t)
            (ma, sa), (mp, sp), (mo, so) = med(t_att), med(t_plan), med(t_torch)
            nq, nk = T * hw * hw, T * (hw // 2) * (hw // 2)
            rows.append("| %d | %d | %d | %s | %.4f (%.0f %%) | %.1f | %.4f (%.0f %%) | %.4f (%.0f %%) | %.2f | %.1e |" % (
                ci, nq, nk, inst, ma, 100 * sa, sess.ops[att][5] / ma * 1e-9, mp, 100 * sp, mo, 100 * so, mo / mp, diff))
            print(rows[-1], flush=True)
            del sess
            torch.cuda.empty_cache()
    text = ("Batch %d, bf16; median of %d rounds x %d launches, plan and torch module alternating.\n\n"
            % (a.batch, a.rounds, a.iters)) + "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
