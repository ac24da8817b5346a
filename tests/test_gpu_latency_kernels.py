"""The two latency-bound launches of X3D's critical path, pv_segate.hip's se_gate_fast_kernel and pv_pool.hip's pool_reduce_kernel, at the
sizes where the way their bytes arrive changes: the SE gate stages fc2's [C][cr] matrix through LDS (flat 16-byte loads, a
dword head and tail where the matrix does not start or end on a 16-byte boundary, rows spread at pitch cr | 1) and runs 256,
512 or 1024 threads by instantiation; the pool issues a thread's taps in straight-line batches of 8 loads (whole batches, then
one with the taps past the window's end neutralised), with a constant step where the window is a run of whole input planes
and (dt, dh, dw) carries, out-of-window taps clamped and neutralised, otherwise.
References and bounds are tests/gpu_util.py's (float64; 1e-5 for the gate, TOL[dtype] for an average, bit-equality for a
maximum, zero padding channels, untouched canaries); the launch helpers are tests/test_gpu_misc_kernels.py's.
"""
import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
import test_gpu_misc_kernels as M

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------ pv_se_gate
@pytest.mark.parametrize("Cc,cr,nblk,extra_pad", [
    (432, 32, 2, 0),       # res5: 14 16-byte pieces of w2 per thread, two channels per thread
    (216, 16, 14, 0),      # res4
    (54, 8, 56, 0),        # res2: 108 pieces over 256 threads, the second half of the block stages nothing
    (54, 6, 5, 0),         # cr not a multiple of 4: a 16-byte piece straddles rows
    (448, 32, 3, 8),       # c_p = 456 above round_up(C, 8); the largest LDS image
    (24, 1, 1, 0),         # smallest case: pitch 1
    (27, 3, 2, 0),         # C * cr = 81: a one-float tail behind the last 16-byte piece
])
def test_se_gate_staged_w2(Cc, cr, nblk, extra_pad):
    i, p = U.make_se_gate(3, Cc, cr, nblk, extra_pad)
    got, routed = M._run("pv_se_gate", L.OP_SE_GATE, lambda t: M._se_desc(t, p), i)
    assert routed == "se_gate_fast_kernel", routed
    U.check_se_gate(got, i, p)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("Cc,cr", [(27, 3), (54, 6), (1, 2)])
def test_se_gate_w2_not_16_byte_aligned(Cc, cr, off):
    """w2 starting `off` floats behind a 16-byte boundary: 4 - off head floats by dword loads, then aligned pieces, then the
    tail ((1, 2): the head is the whole matrix).  The floats around the matrix are NaN: a read past either end shows."""
    i, p = U.make_se_gate(3, Cc, cr, 2)
    d = M._dev(i)
    n = Cc * cr
    buf = torch.full((n + 8,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n] = d["w2"].flatten()
    desc = M._se_desc(d, p)
    desc.w2 = buf.data_ptr() + 4 * off
    U.call("pv_se_gate", desc)
    U.check_se_gate(d["y0"], i, p)


# ------------------------------------------------------------------ pv_pool3d, taps >= 64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,H,W,Cc,k,s,pad,mode", [
    (16, 7, 7, 432, (16, 7, 7), (1, 1, 1), (0, 0, 0), L.POOL_AVG),   # the head's own window: 784 taps, 25 or 24 a thread
    (4, 6, 6, 20, (3, 5, 5), (1, 1, 1), (1, 1, 1), L.POOL_AVG),      # 75 taps: ragged last batch, out-of-window taps, 4 padding channels
    (4, 6, 6, 20, (3, 5, 5), (1, 1, 1), (1, 1, 1), L.POOL_MAX),
    (6, 6, 6, 40, (4, 4, 4), (2, 2, 2), (1, 1, 1), L.POOL_MAX),      # -FLT_MAX neutral element; 5 chunks: 256 / 5 not whole
    (5, 5, 5, 68, (4, 4, 4), (1, 1, 1), (0, 0, 0), L.POOL_AVG),      # exactly 64 taps; 9 chunks: the last slab holds one
    (16, 7, 7, 432, (16, 7, 7), (1, 1, 1), (0, 0, 0), L.POOL_MAX),   # whole planes, maximum
    (12, 7, 7, 64, (8, 7, 7), (4, 1, 1), (0, 0, 0), L.POOL_AVG),     # whole planes from frame 0 and 4: 392 taps, 12 or 13 a thread
    (6, 9, 9, 68, (5, 8, 8), (1, 1, 1), (1, 1, 1), L.POOL_AVG),      # 320 taps with carries and padding: a whole batch, then 2 taps
    (6, 9, 9, 68, (5, 8, 8), (1, 1, 1), (1, 1, 1), L.POOL_MAX),
])
def test_pool_reduce_batched_taps(T, H, W, Cc, k, s, pad, mode, dtype):
    i, p = U.make_pool(dtype, 2, T, H, W, Cc, k, s, pad, mode, gap=16)
    got, routed = M._run("pv_pool3d", L.OP_POOL3D, lambda t: M._pool_desc(t, p, dtype), i)
    assert routed == "pool_reduce_kernel", routed
    U.check_pool(got, i, p)
