"""Direct parity of the four dense GEMM kernels on the MI355X -- gemm_glds_kernel (pv_gemm.hip), gemm8_kernel (pv_gemm8.hip),
gemm_quad_kernel (pv_gemm9.hip), gemm_quad_half_kernel (pv_gemm9h.hip) -- on the LATER tiles of their persistent loops, through the
C ABI (pv_conv3d), with the routed symbol asserted for the large launch and for the first sub-launch of every case.

All four start min(total_tiles, R) workgroups and walk `for (it = blockIdx.x; it < total_tiles; it += gridDim.x)` over the
XCD-aware tile order.  What is delicate in them crosses from one tile to the next: the DMA stream issues the next work item's
first K tiles while this tile's stores are in flight (stores_behind / first_wait_stores, the partial vmcnt waits), gemm_glds's LDS
buffer parity gs runs on and cur = nxt hands the staging geometry over, the scale / shift tables are double-buffered on jt & 1,
the half_b offset barrier is restored at every tile end, the tap walk restarts with the rotation (pt - t) mod kt, and the tile
order has a remainder branch when total & 7 != 0.  None of that runs in a launch of one trip.  Every case here satisfies, asserted
on the CPU before anything is launched (gpu_util.gemm_trip_conditions):

  total_tiles > 2 R,  total_tiles % R != 0,  total_tiles % 8 != 0,  M % BM != 0,  S % BM != 0 (tiles straddle clips)

A ROTATION case cannot meet the last two: the launchers rotate only where a frame is a whole number of tiles, so S and M are
multiples of BM; those cases assert exactly that instead.  The launcher lines these rest on (tests/test_gemm_kernel_checks.py
pins them and checks the Python mirror of the tile order against the formula text):

  pv_gemm_tile.h  const long resident = 256;   dim3 grid((unsigned)(total < resident ? total : resident)), block(threads);
                  tile = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;  m0 = (tile / tiles_n) * BM;  n0 = (tile % tiles_n) * BN
                  pv_gemm_stream_geometry_ok: d.cin % 64 != 0 || K % k_mult != 0 || K < k_min
  pv_gemm.hip     BM = BN = 128, BMV = 64 * VT;  const long resident = 2 * 256;  vt = force_vt ? force_vt : (2 * t128 <= resident ? 1 : 2)
                  -> R 512; 64-row tiles are chosen only where the tiles fit one trip: a later trip of VT 1 needs gemm_vt = 1
  pv_gemm8.hip    BMV8 = 256, BN = 64 * CT;  K < 3 * 64 declined;  gemm8 = 2 | 4 is CT;  gemm8_bk 32 is the <2, 32, 4> ring
  pv_gemm9.hip    BT9 = 256;  pv_gemm_stream_geometry_ok(d, 128, 256, ...);  rows = pw && x_bs == S * ldx;  var = K >= 384 ? 2 : 0
  pv_gemm9h.hip   BMH = 128, BNH = 256, transposed 256 x 128;  pv_gemm_stream_geometry_ok(d, 192, 384, ...)

Checks, every case (gpu_util.GemmExpect; tests/test_gemm_kernel_checks.py proves on the CPU that they fail on the previous tile's
tables, its residual rows, a stale first K tile, the other LDS buffer, a reduction one tap off, two swapped tiles, an unwritten
last trip, one bf16 ulp, a non-zero padding channel, a touched canary):
  1. float64 reference of the same operation on the same bf16-rounded operands, tap by tap (gpu_util.ref_pointwise,
     ref_tap_conv, ref_act), on the host, or with torch on the device in float64 where the product is more than 8e9
     multiply-adds (the record says which); tolerance relative to the reference abs-max, gpu_util.TOL: fp32 out 1e-3, bf16 1e-2.
     A failure names voxel, clip, channel, tile, work item, workgroup and trip.
  2. Trip invariance, BIT FOR BIT: the same operands as sub-launches over whole clips (pointer offsets), each of at most R
     tiles, into a second allocation; torch.equal with the large launch.  Zero is derived, not measured: a voxel's reduction
     runs over the same K tiles in the same order in any tile and on any trip, and the rotation depends only on the frame index
     inside the clip.  Every launcher choice that depends on the tile count is forced to the same value in both launches:
     gemm_vt; gemm9 = 2 / gemm9h = 2 (no min_tiles, no gemm9-against-gemm9h heuristic); gemm9h_tr; gemm8 = CT.
  3. Padding channels [cout, round_up(cout, 8)) exact zeros, canaries around the output intact, a second launch gives the same bits.

Cases (pointwise clips are 1087 voxels = 15 mod 16; "affine" = scale and shift; symbol<template arguments> <- knobs):

  gemm_glds_kernel<PW, VT>           conv_route 2, gemm8 0, gemm9 0, gemm_vt VT                                        R 512
    glds_pw_vt2    <true, 2>   pw 136 -> 264 (K tail, ragged channel tile), B 41, affine, bf16 residual, ReLU        349 x 3 = 1047
    glds_pw_vt1    <true, 1>   pw 192 -> 136, B 31, fp32 out + fp32 residual, affine                                 527 x 2 = 1054
    glds_rot       <false, 2>  (3,1,1) 64 -> 136, frames 16 x 8, T 5, B 103: rotation + temporal fast path; affine, ReLU;
                               once more with gemm_tap_rot 0                                                         515 x 2 = 1030
    glds_chunk     <false, 2>  (1,3,3) s(1,2,2) 72 -> 200 on 17 x 13, T 7, B 149: per-chunk tap decode; scale only, ReLU   514 x 2 = 1028
    glds_umode_vt1 <false, 1>  (3,3,3) 64 -> 136 on 9 x 11, T 5, B 67: uniform-tap staging; shift only                   519 x 2 = 1038
  gemm_quad_kernel<PW, YF32, VAR>    gemm9 2                                                                           R 256
    quad_pw_k256   <true, false, 0>   pw 256 -> 520, B 41, affine, bf16 residual, ReLU                               175 x 3 = 525
    quad_pw_k384   <true, false, 2>   pw 384 -> 520, B 41, affine, ReLU (the form SlowFast and MViT launch most)     525
    quad_pw_f32    <true, true, 2>    pw 384 -> 520, B 41, fp32 out + fp32 residual, shift only                      525
    quad_pw_gap    <false, false, 0>  pw 256 -> 520 with a gap between clips (x_bs > S * ldx, NaN in the gap), B 41, affine  525
    quad_rot       <false, false, 2>  (3,1,1) 128 -> 264, frames 16 x 16, T 5, B 53, affine, ReLU; once more unrotated   265 x 2 = 530
    quad_rot5      <false, false, 2>  (5,1,1) 128 -> 264, frames 16 x 16, T 7, B 37, scale only, ReLU; once more unrotated (with T = kt = 5
                                      the rotated walk visits the frames 0..4 in the unrotated order: the two runs came out
                                      bit-equal, so the clip has two frames more)                                    259 x 2 = 518
    quad_straddle  <false, false, 2>  (1,3,3) s(1,2,2) 128 -> 264 on 17 x 13, T 5, B 209, affine, bf16 residual, ReLU    258 x 2 = 516
    quad_strided   <false, false, 0>  (1,1,1) s(1,2,2) 256 -> 520 on 17 x 13, T 5, B 142 (63 outputs per frame), shift only  175 x 3 = 525
  gemm_quad_half_kernel<PW, YF32, TR>   gemm9h 2, gemm9h_tr TR                                                        R 256
    half_pw        <true, true, false>   pw 384 -> 520, B 21, fp32 out + fp32 residual, affine                       179 x 3 = 537
    half_rot       <false, false, false> (3,1,1) 128 -> 264, frames 16 x 8, T 5, B 53, affine, ReLU; once more unrotated   265 x 2 = 530
    half_27        <false, false, false> (3,3,3) 64 -> 264 on 9 x 11, T 5, B 68, shift only                           263 x 2 = 526
    halftr_pw      <true, true, true>    pw 384 -> 264, B 41, fp32 out, affine                                       175 x 3 = 525
    halftr_rot     <false, false, true>  (3,1,1) 128 -> 136, frames 16 x 16, T 5, B 53, affine, ReLU; once more unrotated  265 x 2 = 530
    halftr_straddle <false, false, true> (1,3,3) s(1,2,2) 64 -> 136 on 17 x 13, T 5, B 209, affine, bf16 residual, ReLU    258 x 2 = 516
  gemm8_kernel<PW, CT, BK, NS>       gemm8 CT, gemm9 0 (, gemm8_bk 32)                                                 R 256
    ring_pw_k192   <true, 2, 64, 3>   pw 192 -> 264 (exactly three stages), B 41, affine, bf16 residual, ReLU        175 x 3 = 525
    ring_pw_bk32   <true, 2, 32, 4>   pw 256 -> 264, B 41, scale only, ReLU                                          525
    ring_pw_ct4    <true, 4, 32, 4>   pw 256 -> 520, B 41, fp32 out + fp32 residual, affine                          525
    ring_t311      <false, 2, 64, 3>  (3,1,1) 64 -> 264 on 17 x 13, T 5, B 41, affine, ReLU (exactly three stages; the ring kernel
                                      does not rotate, so its frames are no whole tiles: the tiles straddle frames and clips;
                                      264 channels are THREE 128-channel tiles)                                      177 x 3 = 531
    ring_ct4_s2    <false, 4, 32, 4>  (1,3,3) s(1,2,2) 64 -> 520 on 17 x 13, T 5, B 142, affine, bf16 residual, ReLU     175 x 3 = 525

The rotated and the unrotated run of a rotation case each pass checks 1 to 3 and agree to one bf16 rounding of the output (8e-3,
the bound of test_temporal_conv_tap_rotation_* in tests/test_gpu_kernels.py).  gemm8_kernel has no rotation.

Which forms the models launch: the kernel traces of the four bench plans (profiles/r6/*_kernel_stats.csv) name
  slowfast_r50   gemm_glds_kernel<true, 2>, <false, 2>, <false, 1>; gemm8_kernel<true, 2, 64, 3>, <false, 2, 64, 3>;
                 gemm_quad_kernel<true, false, 0>, <true, false, 2>, <false, false, 2>; gemm_quad_half_kernel<false, false, false>,
                 <false, false, true>
  mvit_b_32x3    gemm_glds_kernel<true, 2>; gemm_quad_kernel<true, false, 2>, <true, true, 2>; gemm_quad_half_kernel<true, true, false>,
                 <true, true, true>
  x3d_m, x3d_l   gemm_glds_kernel<true, 2>, <false, 2>, <true, 1>
Every one of them is a row above.  Instantiated forms that no case reaches on a later trip, and why:
  - gemm_quad_kernel<true, true, 0>, <false, true, 0>, <false, true, 2> and gemm_quad_half_kernel<true, false, *>, <false, true, *>:
    YF32 selects the store count of the epilogue (and with it the counted waits of the next tile's first K tiles), PW the staging
    rows, VAR where a phase issues its DMAs; each value of each argument is a row above, on the same loop, and no trace shows
    these combinations (an fp32 output belongs to MViT's pointwise layers with K >= 384).
  - gemm8_kernel<false, 2, 32, 4>: the BK 32 ring of ring_pw_bk32 / ring_ct4_s2 with the tap staging of ring_t311; gemm8_bk = 32 is
    an experiment no plan sets.
  - gemm_glds_kernel<*, 2, 1 | 2 | 3>: ablation builds (PV_DEV_ABLATION), not in the library.

What covered a later trip before this module, all in tests/test_gpu_kernels.py (they stay: other shapes, torch's fp32 conv as
reference): the 70000-row and 40000-row pointwise cases of test_large_tile_gemm_kernel, test_quad_phase_gemm_kernel and its
half-height and transposed forms, and the one conv with taps, (16, 8, 32, 32, 128, 128, (1,3,3)) on the transposed half tile --
512 tiles, two whole trips, no ragged last trip, no temporal taps.
"""
import os
import time

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel, cdiv

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
G = U.STREAM_GUARD
DEV = "cuda"                     # where the operands live
HOST_MACS = 8e9                  # a float64 product larger than this is evaluated with torch on the device
ROT_AGREE = 8e-3                 # rotated against unrotated: one bf16 rounding of the output (tests/test_gpu_kernels.py)
DEFAULTS = dict(conv_route=0, gemm8=1, gemm9=1, gemm9h=1, gemm9h_tr=-1, gemm_vt=0, gemm8_bk=64, gemm_tap_rot=1, gemm9_tap_rot=1)
_REC, _CASE_T0 = [], [0.0]

PW1, S_PW = (1, 1, 1), (1, 1, 1087)
S2 = (1, 2, 2)
RELU, NONE = L.ACT_RELU, L.ACT_NONE
# case: (form, form argument, cin, cout, B, input grid (T, H, W), kernel, stride, epilogue, template arguments, tiles_m, tiles_n)
# epilogue: scale, shift, residual ("bf16" | "f32" | None), fp32 output, activation; "gap": the clips of x are not adjacent
CASES = {
    "glds_pw_vt2": ("glds", 2, 136, 264, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, res="bf16", act=RELU), "true, 2", 349, 3),
    "glds_pw_vt1": ("glds", 1, 192, 136, 31, S_PW, PW1, PW1, dict(scale=1, shift=1, res="f32", yf32=1), "true, 1", 527, 2),
    "glds_rot": ("glds", 2, 64, 136, 103, (5, 16, 8), (3, 1, 1), PW1, dict(scale=1, shift=1, act=RELU), "false, 2", 515, 2),
    "glds_chunk": ("glds", 2, 72, 200, 149, (7, 17, 13), (1, 3, 3), S2, dict(scale=1, act=RELU), "false, 2", 514, 2),
    "glds_umode_vt1": ("glds", 1, 64, 136, 67, (5, 9, 11), (3, 3, 3), PW1, dict(shift=1), "false, 1", 519, 2),
    "quad_pw_k256": ("quad", 0, 256, 520, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, res="bf16", act=RELU), "true, false, 0", 175, 3),
    "quad_pw_k384": ("quad", 0, 384, 520, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, act=RELU), "true, false, 2", 175, 3),
    "quad_pw_f32": ("quad", 0, 384, 520, 41, S_PW, PW1, PW1, dict(shift=1, res="f32", yf32=1), "true, true, 2", 175, 3),
    "quad_pw_gap": ("quad", 0, 256, 520, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, gap=264), "false, false, 0", 175, 3),
    "quad_rot": ("quad", 0, 128, 264, 53, (5, 16, 16), (3, 1, 1), PW1, dict(scale=1, shift=1, act=RELU), "false, false, 2", 265, 2),
    "quad_rot5": ("quad", 0, 128, 264, 37, (7, 16, 16), (5, 1, 1), PW1, dict(scale=1, act=RELU), "false, false, 2", 259, 2),
    "quad_straddle": ("quad", 0, 128, 264, 209, (5, 17, 13), (1, 3, 3), S2, dict(scale=1, shift=1, res="bf16", act=RELU), "false, false, 2", 258, 2),
    "quad_strided": ("quad", 0, 256, 520, 142, (5, 17, 13), PW1, S2, dict(shift=1), "false, false, 0", 175, 3),
    "half_pw": ("half", 0, 384, 520, 21, S_PW, PW1, PW1, dict(scale=1, shift=1, res="f32", yf32=1), "true, true, false", 179, 3),
    "half_rot": ("half", 0, 128, 264, 53, (5, 16, 8), (3, 1, 1), PW1, dict(scale=1, shift=1, act=RELU), "false, false, false", 265, 2),
    "half_27": ("half", 0, 64, 264, 68, (5, 9, 11), (3, 3, 3), PW1, dict(shift=1), "false, false, false", 263, 2),
    "halftr_pw": ("half", 1, 384, 264, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, yf32=1), "true, true, true", 175, 3),
    "halftr_rot": ("half", 1, 128, 136, 53, (5, 16, 16), (3, 1, 1), PW1, dict(scale=1, shift=1, act=RELU), "false, false, true", 265, 2),
    "halftr_straddle": ("half", 1, 64, 136, 209, (5, 17, 13), (1, 3, 3), S2, dict(scale=1, shift=1, res="bf16", act=RELU), "false, false, true", 258, 2),
    "ring_pw_k192": ("ring", (2, 64), 192, 264, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, res="bf16", act=RELU), "true, 2, 64, 3", 175, 3),
    "ring_pw_bk32": ("ring", (2, 32), 256, 264, 41, S_PW, PW1, PW1, dict(scale=1, act=RELU), "true, 2, 32, 4", 175, 3),
    "ring_pw_ct4": ("ring", (4, 64), 256, 520, 41, S_PW, PW1, PW1, dict(scale=1, shift=1, res="f32", yf32=1), "true, 4, 32, 4", 175, 3),
    "ring_t311": ("ring", (2, 64), 64, 264, 41, (5, 17, 13), (3, 1, 1), PW1, dict(scale=1, shift=1, act=RELU), "false, 2, 64, 3", 177, 3),
    "ring_ct4_s2": ("ring", (4, 64), 64, 520, 142, (5, 17, 13), (1, 3, 3), S2, dict(scale=1, shift=1, res="bf16", act=RELU), "false, 4, 32, 4", 175, 3),
}
ROTATION = ("glds_rot", "quad_rot", "quad_rot5", "half_rot", "halftr_rot")
SYMBOL = dict(glds="gemm_glds_kernel", quad="gemm_quad_kernel", half="gemm_quad_half_kernel", ring="gemm8_kernel")


@pytest.fixture(scope="module", autouse=True)
def _record():
    """PV_PARITY_RECORD=path: leave the table of the run there (profiles/r32/gemm_kernel_parity.md)."""
    t0 = time.perf_counter()
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if not path:
        return
    worst = {}
    for r in _REC:
        key = (r["kernel"], r["dtype"])
        w = worst.setdefault(key, dict(err=0.0, tiles=set(), subs=set(), bits=set(), seconds=0.0))
        w["err"] = max(w["err"], r["err"])
        w["tiles"].add(r["total"]), w["subs"].add(r["subs"]), w["bits"].add(r["bits"])
        w["seconds"] += r["seconds"]
    with open(path, "w") as f:
        f.write("| kernel form | dtype | worst error | bound asserted | tiles | sub-launches | bit check | seconds |\n|---|---|---|---|---|---|---|---|\n")
        for (k, dt), w in sorted(worst.items()):
            f.write("| `%s` | %s | %.2e | %.0e | %s | %s | %s | %.2f |\n" % (
                k, dt, w["err"], U.TOL[F32 if dt == "float32" else BF16], ", ".join(map(str, sorted(w["tiles"]))),
                ", ".join(map(str, sorted(w["subs"]))), ", ".join(sorted(w["bits"])), w["seconds"]))
        f.write("\n| case | kernel form | tiles | R | trips | sub-launches | error | bound | bit check | reference | seconds |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in _REC:
            f.write("| %s | `%s` | %d x %d = %d | %d | %d + %d tiles | %d | %.2e | %.0e | %s | float64 on the %s | %.2f |\n" % (
                r["case"], r["kernel"], r["tiles_m"], r["tiles_n"], r["total"], r["R"], r["total"] // r["R"], r["total"] % r["R"],
                r["subs"], r["err"], r["tol"], r["bits"], r["ref"], r["seconds"]))
        f.write("\nwhole module: %.1f s\n" % (time.perf_counter() - t0))


@pytest.fixture(autouse=True)
def _case_clock():
    _CASE_T0[0] = time.perf_counter()       # a case's seconds include its operands and its reference
    yield


def _randn(shape, seed, scale=1.0, shift=0.0, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale + shift).to(dtype)


def _ptr(t, elems=0):
    return t.data_ptr() + elems * t.element_size()


def _out_dims(dims, k, s, pad):
    return tuple((n + 2 * p - kk) // ss + 1 for n, kk, ss, p in zip(dims, k, s, pad))


def _form(case):
    """-> (BM, BN, R, knobs, template arguments the launcher's rules give) of a case; the K rules of its unit asserted."""
    form, arg, cin, cout, B, dims, k, stride, ep, targs, _, _ = CASES[case]
    taps = k[0] * k[1] * k[2]
    K = taps * cin
    pw = taps == 1 and stride == (1, 1, 1)
    yf = "true" if ep.get("yf32") else "false"
    rows = "true" if pw and not ep.get("gap") else "false"
    if form == "glds":
        return 64 * arg, 128, 512, dict(conv_route=2, gemm8=0, gemm9=0, gemm_vt=arg), "%s, %d" % (str(pw).lower(), arg)
    if form == "quad":
        assert cin % 64 == 0 and K % 128 == 0 and K >= 256
        return 256, 256, 256, dict(gemm9=2), "%s, %s, %d" % (rows, yf, 2 if K >= 384 else 0)
    if form == "half":
        assert cin % 64 == 0 and K % 192 == 0 and K >= 384
        bm, bn = (256, 128) if arg else (128, 256)
        return bm, bn, 256, dict(gemm9h=2, gemm9h_tr=arg), "%s, %s, %s" % (rows, yf, "true" if arg else "false")
    ct, bk = arg
    assert K >= 3 * 64
    ring = "4, 32, 4" if ct == 4 else "2, 32, 4" if bk == 32 else "2, 64, 3"
    return 256, 64 * ct, 256, dict(gemm8=ct, gemm9=0, gemm8_bk=bk), "%s, %s" % (str(pw).lower(), ring)


def _rotates(form, arg, k, stride, pad, To, HoWo, BM):
    """The launchers' tap_rot rules."""
    if form == "glds":
        return k == (3, 1, 1) and stride[0] == 1 and pad[0] == 1 and To >= 3 and HoWo % BM == 0
    if form in ("quad", "half"):
        return k[0] > 1 and stride[0] == 1 and HoWo % BM == 0
    return False


def _glds_staging(cin, k, stride, pad):
    taps = k[0] * k[1] * k[2]
    if k[1] == k[2] == 1 and stride[1:] == (1, 1) and pad[1:] == (0, 0) and cin % 64 == 0 and k[0] > 1:
        return "temporal fast path"
    return "uniform tap" if taps > 1 and cin % 64 == 0 else "per chunk"


class _Case:
    """Operands on the device, the descriptor of clips [lo, hi), and the float64 reference (computed once)."""

    def __init__(self, case):
        form, arg, cin, cout, B, dims, k, stride, ep, targs, tiles_m, tiles_n = CASES[case]
        self.case, self.form, self.arg, self.ep, self.targs, self.B, self.cin, self.cout = case, form, arg, ep, targs, B, cin, cout
        self.dims, self.k, self.stride = dims, k, stride
        self.pad = pad = tuple(kk // 2 for kk in k)
        self.odims = _out_dims(dims, k, stride, pad)
        self.Si, self.S = dims[0] * dims[1] * dims[2], self.odims[0] * self.odims[1] * self.odims[2]
        self.M, self.cp = B * self.S, U.round_up8(cout)
        self.BM, self.BN, self.R, self.knobs, derived = _form(case)
        assert derived == targs, "%s: the launcher's rules give <%s>, the table says <%s>" % (case, derived, targs)
        self.rotation = case in ROTATION
        assert self.rotation == _rotates(form, arg, k, stride, pad, self.odims[0], self.odims[1] * self.odims[2], self.BM), case
        # the conditions on the inputs, before anything is launched
        tm, tn, self.total = U.gemm_trip_conditions(self.M, self.S, cout, self.BM, self.BN, self.R, self.rotation)
        assert (tm, tn) == (tiles_m, tiles_n), "%s: %d x %d tiles, the table says %d x %d" % (case, tm, tn, tiles_m, tiles_n)
        self.step = U.gemm_sub_clips(self.S, tn, self.BM, self.R)
        self.tiles_m, self.tiles_n = tm, tn
        self.dtype = F32 if ep.get("yf32") else BF16
        taps = k[0] * k[1] * k[2]
        self.gap = ep.get("gap", 0)
        self.x_bs = self.Si * cin + self.gap
        seed = sum(map(ord, case))
        x = torch.full((B, self.x_bs), float("nan"), dtype=BF16, device=DEV)
        x[:, :self.Si * cin] = _randn((B, self.Si * cin), seed)
        self.x = x
        self.w5 = _randn((cout, cin) + tuple(k), seed + 1, (cin * taps) ** -0.5)
        self.w = self.w5.permute(0, 2, 3, 4, 1).reshape(cout, taps * cin).contiguous()
        self.scale = _randn((cout,), seed + 2, 0.2, 1.0, F32) if ep.get("scale") else None
        self.shift = _randn((cout,), seed + 3, 0.5, dtype=F32) if ep.get("shift") else None
        self.res = _randn((self.M, self.cp), seed + 4, dtype=F32 if ep.get("res") == "f32" else BF16) if ep.get("res") else None
        assert (ep.get("res") == "f32") <= bool(ep.get("yf32"))            # the descriptor's r_f32 goes with y_f32
        self.act = ep.get("act", NONE)
        self._want = None
        self.ref = None

    def desc(self, lo, hi, y):
        d = L.Conv3dDesc()
        d.x, d.w, d.y = _ptr(self.x, lo * self.x_bs), _ptr(self.w), _ptr(y, G + lo * self.S * self.cp)
        d.scale = _ptr(self.scale) if self.scale is not None else None
        d.shift = _ptr(self.shift) if self.shift is not None else None
        if self.res is not None:
            d.residual, d.r_bs, d.ldr = _ptr(self.res, lo * self.S * self.cp), self.S * self.cp, self.cp
        d.x_bs, d.y_bs, d.ldx, d.ldy = self.x_bs, self.S * self.cp, self.cin, self.cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = hi - lo, *self.dims, self.cin, *self.odims, self.cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*self.k, *self.stride, *self.pad)
        d.act, d.a_act, d.dtype = self.act, NONE, L.PV_BF16
        d.y_f32, d.r_f32 = int(self.dtype == F32), int(self.ep.get("res") == "f32")
        return d

    def want(self):
        """(M, cout) float64 on the host; evaluated there, or on the device where the product is large"""
        if self._want is not None:
            return self._want
        macs = self.M * self.cout * self.cin * self.k[0] * self.k[1] * self.k[2]
        self.ref = "device" if macs > HOST_MACS else "host"
        dev = DEV if self.ref == "device" else "cpu"
        to = lambda t: None if t is None else t.to(dev)
        x = self.x[:, :self.Si * self.cin].contiguous().to(dev)
        res = None if self.res is None else to(self.res)[:, :self.cout]
        if self.k == (1, 1, 1) and self.stride == (1, 1, 1):
            one, zero = torch.ones(self.cout, device=dev), torch.zeros(self.cout, device=dev)
            out = U.ref_pointwise(x.reshape(self.M, self.cin), to(self.w), one if self.scale is None else to(self.scale),
                                  zero if self.shift is None else to(self.shift), self.act, res=res)
        else:
            out = U.ref_tap_conv(x.view(self.B, *self.dims, self.cin), to(self.w5), self.stride, self.pad, to(self.scale),
                                 to(self.shift), NONE).reshape(self.M, self.cout)
            out = U.ref_act(out if res is None else out + res.double(), self.act)
        self._want = out.cpu()
        return self._want


def _run(c, label, extra_knobs=None):
    """One multi-trip launch of case c against its reference, its one-trip sub-launches and itself -> the output (host)."""
    before = U.stream_buf(c.M, c.cp, c.dtype)
    big, pieces = before.to(DEV), before.to(DEV)
    subs = 0
    try:
        L.tune(**c.knobs)
        L.tune(**(extra_knobs or {}))
        d = c.desc(0, c.B, big)
        routed = _routed_kernel(L.OP_CONV3D, d)
        assert routed == SYMBOL[c.form], routed
        call("pv_conv3d", d)
        first = big.clone()
        call("pv_conv3d", d)
        again = torch.equal(first, big)
        for lo in range(0, c.B, c.step):
            ds = c.desc(lo, min(lo + c.step, c.B), pieces)
            if lo == 0:
                sub_routed = _routed_kernel(L.OP_CONV3D, ds)
                assert sub_routed == SYMBOL[c.form], sub_routed
            call("pv_conv3d", ds)
            subs += 1
    finally:
        L.tune(**DEFAULTS)
    same = torch.equal(first, pieces)
    e = U.GemmExpect(c.want(), before, c.cp, c.S, c.BM, c.BN, c.R, U.TOL[c.dtype])
    assert e.total == c.total and cdiv(c.B, c.step) == subs
    rec = dict(case=label, kernel="%s<%s>" % (SYMBOL[c.form], c.targs), dtype=str(c.dtype).replace("torch.", ""), tiles_m=c.tiles_m,
               tiles_n=c.tiles_n, total=c.total, R=c.R, subs=subs, err=float("nan"), tol=U.TOL[c.dtype],
               bits="equal" if same else "DIFFER", ref=c.ref, seconds=0.0)
    _REC.append(rec)
    got = first.cpu()
    try:
        rec["err"] = e.check(got, label)
        print("%s: error %.3e (bound %.0e), bit check %s, %d tiles, %d sub-launches" % (label, rec["err"], rec["tol"], rec["bits"], c.total, subs))
        if not same:
            e.check_trips(got, pieces.cpu(), label)
        assert again, "%s: a second launch gave other bits" % label
    finally:
        rec["seconds"] = time.perf_counter() - _CASE_T0[0]
        _CASE_T0[0] = time.perf_counter()
    return got


@pytest.mark.parametrize("case", [c for c in CASES if c not in ROTATION])
def test_dense_gemm_later_tiles(case):
    """More than two trips of the persistent loop, a ragged last one, a remainder branch in the tile order, an M tail and tiles
    that straddle clips: float64 reference, bit equality with one-trip sub-launches, padding, canaries, a second launch."""
    c = _Case(case)
    if c.form == "glds":
        staging = {"glds_chunk": "per chunk", "glds_umode_vt1": "uniform tap"}.get(case)
        assert staging is None or staging == _glds_staging(c.cin, c.k, c.stride, c.pad)
    _run(c, case)


@pytest.mark.parametrize("case", ROTATION)
def test_dense_gemm_tap_rotation_on_later_tiles(case):
    """Frames that are whole tiles: the tap walk of a later tile restarts at (pt - t) mod kt.  The rotated and the unrotated run
    each pass every check; they sum the same products in another order and agree to one bf16 rounding of the output."""
    c = _Case(case)
    if c.form == "glds":
        assert _glds_staging(c.cin, c.k, c.stride, c.pad) == "temporal fast path"
    knob = "gemm_tap_rot" if c.form == "glds" else "gemm9_tap_rot"
    rotated = _run(c, case)
    plain = _run(c, case + " unrotated", {knob: 0})
    rows = lambda t: t[G:G + c.M * c.cp].view(c.M, c.cp)[:, :c.cout]
    err = U.rel_err(rows(plain), rows(rotated))
    print("%s: unrotated against rotated %.3e (bound %.0e)" % (case, err, ROT_AGREE))
    assert err <= ROT_AGREE, "%s: the unrotated run is %.3e of the abs-max off the rotated one > %.0e" % (case, err, ROT_AGREE)
