"""Direct parity of the three streaming conv kernels on the MI355X -- pw_stream_kernel (pv_pwconv.hip), tap_stream_kernel
(pv_lateral.hip), stem_c4_kernel (pv_stem.hip) -- on the LATER trips of their grid-stride loops, through the C ABI (pv_conv3d,
pv_lateral_fuse), with the routed symbol asserted in every case.

The kernels stage a filter slab once per workgroup, launch about one resident generation of workgroups and walk the voxel
groups in a loop; the first two hand state from one trip to the next (row geometry, the next group's first operand, the
residual request, the wave's gate cache, PW2's residual one pass ahead).  Every case here runs more than two whole trips and a
ragged last one under every grid the launcher can choose (the stem: more than one; no state crosses its trips).  That is a
condition on the inputs, asserted on the CPU before anything is launched (gpu_util.assert_trips), from the launchers' own lines
(tests/test_stream_kernel_checks.py pins them):

  pv_pwconv.hip   ngroups = pv_ceil_div(M, 4 * TM * 16)        nsplit = pv_ceil_div(pv_round_up(d.cout, 8), NT * 16)
                  resident = 256 * per_cu, per_cu = occ > 4 ? 4 : occ       nchunks = pv_ceil_div(resident, nsplit)
                  -> candidates ceil(256 p / nsplit), p = 1..4; a group is 128 voxels at TM 2 (NT 2, 4), 64 at TM 1 (NT 8)
  pv_lateral.hip  ngroups = pv_ceil_div(M, (kLatThreads / 64) * TM * 16), kLatThreads = 512
                  per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu)       nchunks = pv_ceil_div(256 * per_cu, nsplit)
                  -> candidates ceil(256 p / nsplit), p = 1, 2; a group is 256 voxels at TM 2, 128 at TM 1
  pv_stem.hip     ngroups = pv_ceil_div(M, 4 * TM * 16), gx = ngroups < 4096 ? ngroups : 4096; TM = 4: 256 MFMA columns

Checks, every case (gpu_util.StreamExpect; tests/test_stream_kernel_checks.py proves on the CPU that they fail on a stale
operand, a stale or neighbouring gate row, the previous group's residual, an unwritten last trip, one bf16 ulp, a non-zero
padding channel, a touched canary):
  1. float64 CPU reference of the same operation on the same bf16-rounded operands, rounding where the kernel rounds (the gated
     operand, PW2's inner tensor); tolerance relative to the reference abs-max, gpu_util.TOL: fp32 out 1e-3, bf16 1e-2.  A
     failure names the worst voxel, its clip, its group g and g // nchunks for every candidate grid.
  2. Trip invariance, BIT FOR BIT: the same operands as a series of sub-launches over whole clips (pointer offsets), each of at
     most min(candidates) groups -- one trip under every residency -- into a second allocation; torch.equal with the large
     launch.  Zero is derived, not measured: a voxel's value comes from the same instruction sequence in the same order on any
     trip and in any MFMA column.
  3. Padding channels [cout, round_up(cout, 8)) exact zeros; canaries around the output and every element of a wider row
     outside the written slice as they went in; a second launch gives the same bits.

Case -> symbol -> template arguments <- dispatch condition

pw_stream_kernel<NT, TM, XFORM, KS, F32, X2V> (bf16 operands; NT 2 | 4 | 8 <- round_up(cout, 8) <= 32 | <= 64 | else, TM 2 | 2 | 1;
KS = ceil(cin_p / 32) where launch_pw_x names it, else 0; clips of 8123 voxels = 11 mod 16 unless stated)
  ks1     32 -> 24,  B 37, plain | residual       <2, 2, false, 1, false, false>
  ks1_nt4 24 -> 54,  B 37, plain | residual       <4, 2, false, 1, false, false>    X3D res2 conv_a (its own launch bound)
  ks1_nt8 24 -> 108, B 19, plain | residual       <8, 1, false, 1, false, false>    X3D res3 conv_a of the first block
  ks2     54 -> 54,  B 37, plain | residual       <4, 2, false, 2, false, false>
  ks2_nt2 54 -> 24,  B 37, plain | residual       <2, 2, false, 2, false, false>
  ks3     96 -> 24,  B 37, plain | residual       <2, 2, false, 3, false, false>
  ks3_nt4 80 -> 64,  B 37, plain | residual       <4, 2, false, 3, false, false>    SlowFast's fused slow + lateral width
  ks4_nt8 128 -> 512, B 31, S 1087, plain | residual  <8, 1, false, 4, false, false>  SlowFast fast res5; nsplit 4
  ks4     108 -> 48, B 37, plain | residual       <4, 2, false, 4, false, false>
  ks2_nt8 48 -> 108, B 19, plain | residual       <8, 1, false, 2, false, false>    X3D res3 conv_a
  ks3_nt8 96 -> 216, B 9,  plain | residual       <8, 1, false, 3, false, false>    X3D res4 conv_a; nsplit 2
  ks7     216 -> 96, B 19, plain | residual       <8, 1, false, 7, false, false>    conv_route = 1 (cin > 128)
  ks0_6   192 -> 48, B 37, plain | residual       <4, 2, false, 0, false, false>    6 K steps: no whole-K form; conv_route = 1
  ks0_5   160 -> 72, B 19, plain | residual       <8, 1, false, 0, false, false>    5 K steps at TM 1; conv_route = 1
  split2  216 -> 192, B 9, plain | residual       <8, 1, false, 7, false, false>    nsplit 2; conv_route = 1
  gate_long_ks7   216 -> 96, B 37, S 8123         <8, 1, true, 7, false, false>     a_gate + Swish, residual, ReLU
  gate_long_ks4   108 -> 48, B 37, S 8123         <4, 2, true, 4, false, false>
  gate_long_ks2   54 -> 24,  B 37, S 8123         <2, 2, true, 2, false, false>
  gate_tiny_ks7   216 -> 96, B 4486, S 67         <8, 1, true, 7, false, false>     most tiles span two clips
  gate_tiny_ks2   54 -> 24,  B 4486, S 67         <2, 2, true, 2, false, false>
  swish_ks2       54 -> 24,  B 37, S 8123         <2, 2, true, 2, false, false>     a_act Swish without a gate, residual
  f32     96 -> 288, B 41, S 1087, plain | fp32 residual   <8, 1, false, 3, true, false>   y_f32 (+ r_f32); nsplit 3
  x2_ks3  54 (+ 24 strided) -> 24, gate, 37 x 4 x 45 x 45  <2, 2, true, 3, false, true>    x2, 2 + 1 K steps
  x2_ks0  108 (+ 24 strided) -> 48, gate, 37 x 4 x 45 x 45 <4, 2, true, 0, false, true>    x2, 4 + 1 K steps
  x2_plain 32 (+ 24 strided) -> 32, 37 x 4 x 45 x 45       <2, 2, false, 0, false, true>   x2 without gate; 1 + 1 K steps
  x2_plain_nt4     16 (+ 32 strided) -> 64,  37 x 4 x 45 x 45   <4, 2, false, 0, false, true>   SlowFast fast res3 conv_c
  x2_plain_nt8_ks3 32 (+ 64 strided) -> 128, 17 x 4 x 45 x 45   <8, 1, false, 3, false, true>   fast res4; 1 + 2 K steps
  x2_plain_nt8_ks0 64 (+ 80 strided) -> 256, 17 x 2 x 45 x 45   <8, 1, false, 0, false, true>   slow res2; 2 + 3 K steps, nsplit 2
tap_stream_kernel<NT, TM, PW2> (bf16; each pv_conv3d case with tap_xcont 1 and 0; output grids of 125 x 125 per frame)
  (1,3,3) 8 -> 8              <2, 2, false>      cout_p8 <= 32
  (3,1,1) 32 -> 8             <2, 2, false>
  (1,3,3) s(1,2,2) 16 -> 16 on 249 x 249          <2, 2, false>      odd input grid
  (3,3,3) s(2,1,1) 16 -> 40   <4, 2, false>      cout_p8 <= 64; every tap direction, temporal stride
  (3,1,1) 32 -> 96            <8, 1, false>      cout in (64, 128]
  (1,3,3) 56 -> 72            <4, 2, false>      lds_of(8) = 134656 > 120 KB: NT halved, nsplit 2
  (1,3,3) 8 -> 8 -> 32 + residual                 <2, 2, true>       pw2_w; ldy 40: channels [32, 40) untouched
  (1,3,3) 16 -> 24 -> 72                          <2, 2, true>       24 inner channels are NT 2 as well
  (1,3,3) 16 -> 40 -> 72                          <4, 2, true>       inner channels in (32, 64]
  pv_lateral_fuse 8 -> 16, kt 7, st 4, Ti 30      <2, 2, false>      into channels [16, 32) of 40-wide rows
  pv_lateral_fuse 24 -> 40, kt 5, st 2, Ti 15     <4, 2, false>      into channels [16, 56) of 64-wide rows
stem_c4_kernel<NT, TM, JP>
  (1,3,3) s(1,2,2) 3 -> 24, 2 x 9 x 501 x 501     <2, 4>             cout_p8 <= 32: 4430 groups against 4096 workgroups
  (1,3,3) 3 -> 8, c4_wpair 2, 2 x 5 x 501 x 501   <1, 4, 2>          4913 groups of 256 two-output columns

Which forms the models launch: the kernel traces of the four bench plans (profiles/r3 and profiles/r6, *_kernel_stats.csv) name
  mvit_b_32x3    pw_stream_kernel<8, 1, false, 3, true, false>
  slowfast_r50   pw_stream_kernel<2, 2, false, 1>, <4, 2, false, 1>, <8, 1, false, 1>, <8, 1, false, 2>, <4, 2, false, 3>, <8, 1, false, 4>
                 and, with X2V, <2, 2, false, 0>, <4, 2, false, 0>, <8, 1, false, 3>, <8, 1, false, 0>; tap_stream_kernel<2, 2>, <4, 2>, both
                 with and without PW2
  x3d_m, x3d_l   pw_stream_kernel<2, 2, false, 2>, <4, 2, false, 4>, <8, 1, false, 3>, <2, 2, true, 2>, <4, 2, true, 4>, <8, 1, true, 7>
                 and, with X2V, <2, 2, true, 3>, <4, 2, true, 0>; tap_stream_kernel<8, 1, false>
Every one of them is a row of the table above.  Not reached on a later trip, and why:
  - pw_stream_kernel<8, 1, *, 14, *, *> cannot be launched at all: launch_pw_x names KS 14 at TM 1 only, TM 1 is NT 8, and the slab
    of NT 8 at 14 K steps is 128 * (14 * 32 + 8) * 2 = 116736 B, over the 96 KB pv_pwconv_stream_try admits.  432 input channels
    go to another kernel whatever the knob; test_whole_k_form_of_14_steps_is_out_of_the_launchers_reach asserts that, so that a
    change of the limit brings the form into this file.
  - Forms no trace shows: XFORM at KS 1 and at KS 0 without a second operand, XFORM at NT other than the rows above (a gate or an
    activation on load belongs to X3D's conv_c at 54, 108, 216 input channels); plain (NT, KS) pairs without a row; F32 at KS other than 3 (the fp32-out form serves MViT's 96-channel
    linears); X2V at the (NT, KS, XFORM) triples without a row.  They share the loop of the rows above and differ in unroll counts.
  - The m32 == false path needs 2^31 voxels; inputs near the 2 GiB buffer-offset limit are out of scope.
"""
import ctypes as C
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
PW_PER_CU, TAP_PER_CU = (1, 2, 3, 4), (1, 2)
_REC, _T0, _CASE_T0 = [], time.perf_counter(), [0.0]


@pytest.fixture(scope="module", autouse=True)
def _record():
    """PV_PARITY_RECORD=path: leave the table of the run there (profiles/r31/stream_kernel_parity.md)."""
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if not path:
        return
    worst = {}
    for r in _REC:
        key = (r["kernel"], r["dtype"])
        worst[key] = max(worst.get(key, 0.0), r["err"])
    with open(path, "w") as f:
        f.write("| kernel | dtype | worst error | bound asserted |\n|---|---|---|---|\n")
        for (k, dt), v in sorted(worst.items()):
            f.write("| `%s` | %s | %.2e | %.0e |\n" % (k, dt, v, U.TOL[F32 if dt == "float32" else BF16]))
        f.write("\n| case | kernel | ngroups | candidate nchunks | sub-launches | error | bit check | seconds |\n|---|---|---|---|---|---|---|---|\n")
        for r in _REC:
            f.write("| %s | `%s` | %d | %s | %d | %.2e | %s | %.2f |\n" % (
                r["case"], r["kernel"], r["ngroups"], ", ".join(map(str, r["nchunks"])), r["subs"], r["err"], r["bits"], r["seconds"]))
        f.write("\nwhole module: %.1f s\n" % (time.perf_counter() - _T0))


@pytest.fixture(autouse=True)
def _case_clock():
    _CASE_T0[0] = time.perf_counter()       # a case's seconds include its operands and its reference
    yield


def _randn(shape, seed, scale=1.0, shift=0.0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale + shift).to(dtype)


def _zeros(shape):
    return torch.zeros(shape, dtype=BF16, device="cuda")


def _padded(shape, c, seed, scale=1.0, dtype=BF16):
    """Random values in channels [0, c) of the last dimension, zeros up to its multiple of 8."""
    t = _randn(shape, seed, scale, dtype=dtype)
    t[..., c:] = 0
    return t


def _ptr(t, elems=0):
    return t.data_ptr() + elems * t.element_size()


def _run(case, kernel, targs, fn, op, desc, nclips, per_clip, want, ld, gvox, cands, dtype, c_off=0, units_per_clip=None,
         unit=None, knobs=None, restore=None, full=2, fill=False):
    """One multi-trip case.  desc(lo, hi, y) -> the descriptor of clips [lo, hi) writing at their place in allocation y;
    want() -> (M, cout) float64.  units_per_clip: MFMA columns per clip where a column is not a voxel."""
    upc = units_per_clip or per_clip
    M, ngroups = nclips * per_clip, cdiv(nclips * upc, gvox)
    U.assert_trips(ngroups, cands, full)                              # on the CPU, before anything is launched
    step = min(cands) * gvox // upc
    assert step >= 1 and cdiv(step * upc, gvox) <= min(cands)         # a sub-launch is one trip under every candidate
    assert (nclips * upc) % 16 != 0                                   # the last 16-column tile is ragged as well
    filler = U.randn((M, ld), 5) if fill else None
    before = U.stream_buf(M, ld, dtype, fill=filler)
    big, pieces = before.cuda(), before.cuda()
    subs = 0
    try:
        L.tune(**(knobs or {}))
        d = desc(0, nclips, big)
        routed = _routed_kernel(op, d)
        assert routed == kernel, routed
        call(fn, d)
        first = big.clone()
        call(fn, d)
        again = torch.equal(first, big)
        for lo in range(0, nclips, step):
            ds = desc(lo, min(lo + step, nclips), pieces)
            if lo == 0:
                assert _routed_kernel(op, ds) == kernel
            call(fn, ds)
            subs += 1
    finally:
        L.tune(**(restore or {}))
    same = torch.equal(first, pieces)
    e = U.StreamExpect(want(), before, ld, per_clip, gvox, cands, U.TOL[dtype], c_off=c_off, unit=unit)
    rec = dict(case=case, kernel="%s<%s>" % (kernel, targs), dtype=str(dtype).replace("torch.", ""), ngroups=ngroups,
               nchunks=list(cands), subs=subs, err=float("nan"), bits="equal" if same else "DIFFER")
    _REC.append(rec)
    try:
        rec["err"] = e.check(first.cpu(), case)
        print("%s: error %.3e, bit check %s" % (case, rec["err"], rec["bits"]))
        if not same:
            e.check_trips(first.cpu(), pieces.cpu(), case)
        assert again, "%s: a second launch gave other bits" % case
    finally:
        rec["seconds"] = time.perf_counter() - _CASE_T0[0]


# ------------------------------------------------------------------ pw_stream_kernel
ROUTE1 = dict(knobs=dict(conv_route=1), restore=dict(conv_route=0))
PW = {      # case: (cin, cout, B, (T, H, W), NT, KS, conv_route = 1, {"gate", "swish", "x2", "f32"})
    "ks1": (32, 24, 37, (1, 1, 8123), 2, 1, False, ()),
    "ks1_nt4": (24, 54, 37, (1, 1, 8123), 4, 1, False, ()),
    "ks1_nt8": (24, 108, 19, (1, 1, 8123), 8, 1, False, ()),
    "ks2": (54, 54, 37, (1, 1, 8123), 4, 2, False, ()),
    "ks2_nt2": (54, 24, 37, (1, 1, 8123), 2, 2, False, ()),
    "ks3_nt4": (80, 64, 37, (1, 1, 8123), 4, 3, False, ()),
    "ks4_nt8": (128, 512, 31, (1, 1, 1087), 8, 4, False, ()),
    "ks3": (96, 24, 37, (1, 1, 8123), 2, 3, False, ()),
    "ks4": (108, 48, 37, (1, 1, 8123), 4, 4, False, ()),
    "ks2_nt8": (48, 108, 19, (1, 1, 8123), 8, 2, False, ()),
    "ks3_nt8": (96, 216, 9, (1, 1, 8123), 8, 3, False, ()),
    "ks7": (216, 96, 19, (1, 1, 8123), 8, 7, True, ()),
    "ks0_6": (192, 48, 37, (1, 1, 8123), 4, 0, True, ()),
    "ks0_5": (160, 72, 19, (1, 1, 8123), 8, 0, True, ()),
    "split2": (216, 192, 9, (1, 1, 8123), 8, 7, True, ()),
    "gate_long_ks7": (216, 96, 37, (1, 1, 8123), 8, 7, True, ("gate", "swish")),
    "gate_long_ks4": (108, 48, 37, (1, 1, 8123), 4, 4, False, ("gate", "swish")),
    "gate_long_ks2": (54, 24, 37, (1, 1, 8123), 2, 2, False, ("gate", "swish")),
    "gate_tiny_ks7": (216, 96, 4486, (1, 1, 67), 8, 7, True, ("gate", "swish")),
    "gate_tiny_ks2": (54, 24, 4486, (1, 1, 67), 2, 2, False, ("gate", "swish")),
    "swish_ks2": (54, 24, 37, (1, 1, 8123), 2, 2, False, ("swish",)),
    "f32": (96, 288, 41, (1, 1, 1087), 8, 3, False, ("f32",)),
    "x2_ks3": (54, 24, 37, (4, 45, 45), 2, 3, False, ("gate", "swish", "x2")),
    "x2_ks0": (108, 48, 37, (4, 45, 45), 4, 0, False, ("gate", "swish", "x2")),
    "x2_plain": (32, 32, 37, (4, 45, 45), 2, 0, False, ("x2",)),
    "x2_plain_nt4": (16, 64, 37, (4, 45, 45), 4, 0, False, ("x2",)),
    "x2_plain_nt8_ks3": (32, 128, 17, (4, 45, 45), 8, 3, False, ("x2",)),
    "x2_plain_nt8_ks0": (64, 256, 17, (2, 45, 45), 8, 0, False, ("x2",)),
}
X2_CIN = {"x2_plain_nt4": 32, "x2_plain_nt8_ks3": 64, "x2_plain_nt8_ks0": 80}      # channels of the second operand (default 24)
_PW_OPERANDS = {}       # one slot: the plain and the residual form of a case share operands and the reference's product


def _pw_operands(case):
    if case in _PW_OPERANDS:
        return _PW_OPERANDS[case]
    _PW_OPERANDS.clear()
    cin, cout, B, (T, H, W), NT, KS, _, flags = PW[case]
    S, cin_p, cp = T * H * W, U.round_up8(cin), U.round_up8(cout)
    gated, swish, f32, x2 = ("gate" in flags), ("swish" in flags), ("f32" in flags), ("x2" in flags)
    t = dict(x=_padded((B * S, cin_p), cin, 31), scale=_randn((cout,), 33, 0.2, 1.0, F32), shift=_randn((cout,), 34, dtype=F32))
    t["res"] = _padded((B * S, cp), cout, 36, dtype=F32 if f32 else BF16)
    if gated:                                                         # a row per clip, drawn per clip
        t["gate"] = torch.sigmoid(_randn((B, cin_p), 35, 2.0, dtype=F32))
    k1 = cin_p
    if x2:
        cin2, k1 = X2_CIN.get(case, 24), U.round_up32(cin_p)
        H2, W2 = (H - 1) * 2 + 2, (W - 1) * 2 + 1                     # a last input row that no output samples
        t["x2"] = _randn((B, T, H2, W2, cin2), 37)
        t["x2_scale"] = _randn((cout,), 38, 0.2, 0.7, F32)
        w = _zeros((cout, k1 + U.round_up32(cin2)))
        w[:, :cin] = _randn((cout, cin), 32, cin ** -0.5)
        w[:, k1:k1 + cin2] = _randn((cout, cin2), 39, cin2 ** -0.5)
        t["w"] = w
    else:
        t["w"] = _padded((cout, cin_p), cin, 32, cin ** -0.5)
    c = {k: v.cpu() for k, v in t.items()}
    clip = torch.arange(B * S) // S
    kw = dict(gate=c["gate"], clip=clip) if gated else {}
    kw["a_act"] = L.ACT_SWISH if swish else L.ACT_NONE
    if x2:
        kw.update(x2=c["x2"][:, :, ::2, ::2].reshape(B * S, -1), w2=c["w"][:, k1:k1 + cin2], scale2=c["x2_scale"])
    pre = U.ref_pointwise(c["x"], c["w"][:, :cin_p], c["scale"], c["shift"], L.ACT_NONE, **kw)
    _PW_OPERANDS[case] = (t, c, pre)
    return _PW_OPERANDS[case]


def _pw_case(case, res):
    cin, cout, B, (T, H, W), NT, KS, route, flags = PW[case]
    S, cin_p, cp = T * H * W, U.round_up8(cin), U.round_up8(cout)
    gated, swish, f32, x2 = ("gate" in flags), ("swish" in flags), ("f32" in flags), ("x2" in flags)
    TM = 1 if NT == 8 else 2
    nsplit = cdiv(cp, 16 * NT)
    assert NT == (2 if cp <= 32 else 4 if cp <= 64 else 8)
    cin2 = X2_CIN.get(case, 24)
    ksteps = cdiv(cin_p, 32) + (cdiv(cin2, 32) if x2 else 0)
    whole_k = (3,) if x2 else (1, 2, 3, 4, 7, 14) if TM == 1 else (1, 2, 3, 4)                   # launch_pw_x
    assert KS == (ksteps if ksteps in whole_k else 0)
    if gated:
        assert S >= 64 and S % 16 != 0
    t, c, pre = _pw_operands(case)
    act = L.ACT_NONE if f32 else L.ACT_RELU

    def desc(lo, hi, y):
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = _ptr(t["x"], lo * S * cin_p), _ptr(t["w"]), _ptr(y, G + lo * S * cp), _ptr(t["scale"]), _ptr(t["shift"])
        if res:
            d.residual = _ptr(t["res"], lo * S * cp)
        if gated:
            d.a_gate = _ptr(t["gate"], lo * cin_p)
        d.a_act = L.ACT_SWISH if swish else L.ACT_NONE
        d.x_bs, d.y_bs, d.r_bs, d.ldx, d.ldy, d.ldr = S * cin_p, S * cp, S * cp, cin_p, cp, cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = hi - lo, T, H, W, cin_p, T, H, W, cout
        d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
        d.act, d.dtype, d.y_f32, d.r_f32 = act, L.PV_BF16, int(f32), int(f32 and res)
        if x2:
            v = t["x2"]
            d.x2, d.x2_scale, d.x2_bs, d.x2_ld, d.x2_cin = _ptr(v, lo * v.stride(0)), _ptr(t["x2_scale"]), v.stride(0), cin2, cin2
            d.x2_Hi, d.x2_Wi, d.x2_st, d.x2_sh, d.x2_sw = v.shape[2], v.shape[3], 1, 2, 2
            assert L.lib().pv_conv3d_x2_supported(C.byref(d)) == 1 and (H * W) % 16 != 0
        return d

    def want():
        return U.ref_act(pre + c["res"][:, :cout].double() if res else pre, act)

    targs = "%d, %d, %s, %d, %s, %s" % (NT, TM, str(gated or swish).lower(), KS, str(f32).lower(), str(x2).lower())
    _run("%s %s" % (case, "residual" if res else "plain"), "pw_stream_kernel", targs, "pv_conv3d", L.OP_CONV3D, desc, B, S, want, cp,
         64 * TM, U.stream_chunks(256, PW_PER_CU, nsplit), F32 if f32 else BF16, **(ROUTE1 if route else {}))


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", ["ks1", "ks1_nt4", "ks1_nt8", "ks2", "ks2_nt2", "ks3", "ks3_nt4", "ks4", "ks4_nt8", "ks2_nt8", "ks3_nt8", "ks7", "ks0_6", "ks0_5", "split2", "f32"])
def test_pointwise_conv_later_trips(case, res):
    """cur = nxt, the operand prefetched for the next group ahead of this group's epilogue, the residual requested at the loop
    top: M = 11 mod 16 voxels over clips of 8123 (f32: 1087), so tiles straddle clips and the last trip is ragged twice over."""
    _pw_case(case, res)


def test_whole_k_form_of_14_steps_is_out_of_the_launchers_reach():
    """432 input channels, the only width launch_pw_x sends to KS 14, need an NT 8 slab of 116736 B: pv_pwconv_stream_try's 96 KB
    limit declines it before launch_pw is asked, with and without the knob that prefers the streaming kernel."""
    cin, cout, S = 432, 72, 256
    assert cdiv(cin, 32) == 14 and 8 * 16 * (14 * 32 + 8) * 2 + 2 * 8 * 16 * 4 > 96 * 1024
    x, w, y = _randn((S, cin), 81), _randn((cout, cin), 82, cin ** -0.5), _zeros((S, cout))
    d = L.Conv3dDesc()
    d.x, d.w, d.y = _ptr(x), _ptr(w), _ptr(y)
    d.x_bs, d.y_bs, d.ldx, d.ldy = S * cin, S * cout, cin, cout
    d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = 1, 1, 1, S, cin, 1, 1, S, cout
    d.kt = d.kh = d.kw = d.st = d.sh = d.sw = 1
    d.act, d.dtype = L.ACT_RELU, L.PV_BF16
    for route in (1, 0):
        try:
            L.tune(conv_route=route)
            routed = _routed_kernel(L.OP_CONV3D, d)
        finally:
            L.tune(conv_route=0)
        assert routed and routed != "pw_stream_kernel", routed


@pytest.mark.parametrize("case", ["gate_long_ks7", "gate_long_ks4", "gate_long_ks2", "gate_tiny_ks7", "gate_tiny_ks2", "swish_ks2"])
def test_gated_pointwise_conv_refreshes_its_gate_cache_between_trips(case):
    """Long clips: a wave's later trips land many clips further on and the last clip has no next one.  Tiny clips (S = 67, just
    above the launcher's 64): almost every trip begins in a clip other than the cached one and most tiles span two clips.  The
    gate rows are drawn per clip: another clip's row moves the result by tens of per cent.  swish_ks2: the activation on load
    without a gate (a block without squeeze-excitation), XFORM with nothing to cache."""
    _pw_case(case, True)


@pytest.mark.parametrize("case", ["x2_ks3", "x2_ks0", "x2_plain", "x2_plain_nt4", "x2_plain_nt8_ks3", "x2_plain_nt8_ks0"])
def test_two_operand_pointwise_conv_later_trips(case):
    """The projection shortcut as second K operand, sampled with stride (1, 2, 2) from a grid with one more row than the outputs
    reach, its own scale, and the gate on the first operand only (x2_plain*: no gate, no activation on load, SlowFast's first
    block of a stage, at every NT, at KS 3 and with nsplit 2); Ho Wo = 2025 is no multiple of 16."""
    _pw_case(case, False)


# ------------------------------------------------------------------ tap_stream_kernel
def _tap_operands(B, Ti, Hi, Wi, cin, cout, k, seed=41):
    taps = k[0] * k[1] * k[2]
    x = _randn((B, Ti, Hi, Wi, cin), seed)
    w = _randn((cout, cin) + tuple(k), seed + 1, (cin * taps) ** -0.5)
    t = dict(x=x, w=w.permute(0, 2, 3, 4, 1).reshape(cout, taps * cin).contiguous(), scale=_randn((cout,), seed + 2, 0.2, 1.0, F32),
             shift=_randn((cout,), seed + 3, 0.5, dtype=F32))
    return t, dict(x=x.cpu(), w=w.cpu(), scale=t["scale"].cpu(), shift=t["shift"].cpu())


def _out_dims(dims, k, s, pad):
    return tuple((n + 2 * p - kk) // ss + 1 for n, kk, ss, p in zip(dims, k, s, pad))


TAP = {     # case: (B, (Ti, Hi, Wi), cin, cout, k, stride, NT)
    "1x3x3_8_8": (5, (4, 125, 125), 8, 8, (1, 3, 3), (1, 1, 1), 2),
    "3x1x1_32_8": (5, (4, 125, 125), 32, 8, (3, 1, 1), (1, 1, 1), 2),
    "1x3x3_s2_16_16": (5, (4, 249, 249), 16, 16, (1, 3, 3), (1, 2, 2), 2),
    "3x3x3_st2_16_40": (5, (8, 125, 125), 16, 40, (3, 3, 3), (2, 1, 1), 4),
    "3x1x1_32_96": (5, (2, 125, 125), 32, 96, (3, 1, 1), (1, 1, 1), 8),
    "1x3x3_56_72": (5, (2, 125, 125), 56, 72, (1, 3, 3), (1, 1, 1), 4),
}
_TAP_OPERANDS = {}


@pytest.mark.parametrize("xcont", [1, 0])
@pytest.mark.parametrize("case", list(TAP))
def test_narrow_dense_conv_later_trips(case, xcont):
    """tile_of(g + nchunks), the next tile's first operand requested behind the last K step, cur = nxt -- under both chunk -> XCD
    mappings.  15625 voxels per frame: M is no multiple of 16 and the tiles straddle rows, frames and clips."""
    B, dims, cin, cout, k, s, NT = TAP[case]
    pad = tuple(kk // 2 for kk in k)
    To, Ho, Wo = _out_dims(dims, k, s, pad)
    Si, So, cp = dims[0] * dims[1] * dims[2], To * Ho * Wo, U.round_up8(cout)
    TM, K = (1 if NT == 8 else 2), k[0] * k[1] * k[2] * cin
    ksteps = cdiv(K, 32)
    lds_of = lambda nt: nt * 16 * (ksteps * 32 + 8) * 2 + 2 * nt * 16 * 4 + ksteps * 4 * 8      # tapstream_launch
    nt = 2 if cp <= 32 else 4 if cp <= 64 else 8
    while nt > 2 and lds_of(nt) > 120 * 1024:
        nt >>= 1
    assert nt == NT and K <= 640
    nsplit = cdiv(cp, 16 * NT)
    if case == "1x3x3_56_72":
        assert lds_of(8) == 134656 > 120 * 1024 and nsplit == 2
    if case not in _TAP_OPERANDS:
        _TAP_OPERANDS.clear()
        t, c = _tap_operands(B, *dims, cin, cout, k)
        _TAP_OPERANDS[case] = (t, c, U.ref_tap_conv(c["x"], c["w"], s, pad, c["scale"], c["shift"], L.ACT_RELU).reshape(-1, cout))
    t, c, ref = _TAP_OPERANDS[case]

    def desc(lo, hi, y):
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = _ptr(t["x"], lo * Si * cin), _ptr(t["w"]), _ptr(y, G + lo * So * cp), _ptr(t["scale"]), _ptr(t["shift"])
        d.x_bs, d.y_bs, d.ldx, d.ldy = Si * cin, So * cp, cin, cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = hi - lo, *dims, cin, To, Ho, Wo, cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *pad)
        d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
        return d

    _run("%s xcont %d" % (case, xcont), "tap_stream_kernel", "%d, %d, false" % (NT, TM), "pv_conv3d", L.OP_CONV3D, desc, B, So,
         lambda: ref, cp, 128 * TM, U.stream_chunks(256, TAP_PER_CU, nsplit), BF16, knobs=dict(tap_xcont=xcont),
         restore=dict(tap_xcont=1))


@pytest.mark.parametrize("cin,cmid,cout2,res,NT", [(8, 8, 32, True, 2), (16, 24, 72, False, 2), (16, 40, 72, False, 4)])
def test_conv_b_and_pointwise_conv_c_in_one_launch_later_trips(cin, cmid, cout2, res, NT):
    """PW2: the residual of the second product (rq / rn, one pass ahead at NT 4) on later trips.  The output rows are 8 channels
    wider than round_up(cout2, 8): that slice, in y and in the residual's buffer of the same strides, is not touched."""
    B, dims, k, s, pad = 5, (4, 125, 125), (1, 3, 3), (1, 1, 1), (0, 1, 1)
    So, cmp8, c2p = dims[0] * dims[1] * dims[2], U.round_up8(cmid), U.round_up8(cout2)
    ld = c2p + 8
    assert NT == (2 if cmp8 <= 32 else 4)
    t, c = _tap_operands(B, *dims, cin, cmid, k, seed=51)
    w2 = _padded((cout2, cmp8), cmid, 55, cmid ** -0.5)
    s2, h2 = _randn((cout2,), 56, 0.2, 1.0, F32), _randn((cout2,), 57, 0.5, dtype=F32)
    r = _randn((B * So, ld), 58)

    def desc(lo, hi, y):
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.scale, d.shift = _ptr(t["x"], lo * So * cin), _ptr(t["w"]), _ptr(y, G + lo * So * ld), _ptr(t["scale"]), _ptr(t["shift"])
        d.x_bs, d.y_bs, d.ldx, d.ldy = So * cin, So * ld, cin, ld
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = hi - lo, *dims, cin, *dims, cmid
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *pad)
        d.act, d.a_act, d.dtype = L.ACT_RELU, L.ACT_NONE, L.PV_BF16
        d.pw2_w, d.pw2_scale, d.pw2_shift, d.pw2_cout, d.pw2_act = _ptr(w2), _ptr(s2), _ptr(h2), cout2, L.ACT_RELU
        if res:
            d.residual, d.r_bs, d.ldr = _ptr(r, lo * So * ld), So * ld, ld
        assert L.lib().pv_conv3d_pw2_supported(C.byref(d)) == 1
        return d

    def want():
        return U.ref_tap_pw2(c["x"], c["w"], s, pad, c["scale"], c["shift"], L.ACT_RELU, w2.cpu()[:, :cmid], s2.cpu(), h2.cpu(),
                             L.ACT_RELU, res=r.cpu()[:, :cout2] if res else None)

    r0 = r.clone()
    _run("pw2 %d-%d-%d" % (cin, cmid, cout2), "tap_stream_kernel", "%d, 2, true" % NT, "pv_conv3d", L.OP_CONV3D, desc, B, So, want, ld,
         256, U.stream_chunks(256, TAP_PER_CU, 1), BF16, fill=True)
    assert torch.equal(r, r0)


@pytest.mark.parametrize("cin,cout,kt,st,Ti,NT", [(8, 16, 7, 4, 30, 2), (24, 40, 5, 2, 15, 4)])
def test_lateral_fusion_later_trips(cin, cout, kt, st, Ti, NT):
    """A time-strided gather written into the channel slice [16, 16 + round_up(cout, 8)) of the slow pathway's rows; Ti is no
    multiple of the stride, so the last slow frame's window ends in the zero padding.  The slow slice must come back bit-equal."""
    B, H, W, c_slow = 7, 75, 77, 16
    pt = kt // 2
    To = (Ti + 2 * pt - kt) // st + 1
    assert Ti % st != 0 and To == 8
    So, cp = To * H * W, U.round_up8(cout)
    ld = c_slow + cp + 8
    t, c = _tap_operands(B, Ti, H, W, cin, cout, (kt, 1, 1), seed=61)

    def desc(lo, hi, y):
        d = L.LateralDesc()
        d.x, d.w, d.y, d.scale, d.shift = _ptr(t["x"], lo * Ti * H * W * cin), _ptr(t["w"]), _ptr(y, G + lo * So * ld + c_slow), _ptr(t["scale"]), _ptr(t["shift"])
        d.x_bs, d.y_bs, d.ldx, d.ldy = Ti * H * W * cin, So * ld, cin, ld
        d.B, d.Ti, d.H, d.W, d.cin, d.To, d.cout = hi - lo, Ti, H, W, cin, To, cout
        d.kt, d.st, d.pt, d.act, d.dtype = kt, st, pt, L.ACT_RELU, L.PV_BF16
        return d

    def want():
        return U.ref_tap_conv(c["x"], c["w"], (st, 1, 1), (pt, 0, 0), c["scale"], c["shift"], L.ACT_RELU).reshape(-1, cout)

    _run("lateral %d-%d kt %d st %d" % (cin, cout, kt, st), "tap_stream_kernel", "%d, 2, false" % NT, "pv_lateral_fuse", L.OP_LATERAL, desc,
         B, So, want, ld, 256, U.stream_chunks(256, TAP_PER_CU, 1), BF16, c_off=c_slow, fill=True)


# ------------------------------------------------------------------ stem_c4_kernel
@pytest.mark.parametrize("cout,T,s,wpair", [(24, 9, (1, 2, 2), 0), (8, 5, (1, 1, 1), 2)], ids=["x3d_stem_24", "wpair_8"])
def test_first_layer_conv_second_grid_trip(cout, T, s, wpair):
    """gridDim.x = min(ngroups, 4096): one whole trip and a ragged second (no state crosses the trips of this kernel).  The X3D
    stem conv on 2 x 9 x 501 x 501 is 4430 groups; with two outputs per MFMA column, 2 x 5 x 501 x 501 at stride 1 is 4913."""
    B, H, W, k, pad = 2, 501, 501, (1, 3, 3), (0, 1, 1)
    To, Ho, Wo = _out_dims((T, H, W), k, s, pad)
    Si, So, cp = T * H * W, To * Ho * Wo, U.round_up8(cout)
    jp = 2 if wpair else 1
    Wo2 = cdiv(Wo, jp)
    x4 = _randn((B, T, H, W, 4), 71)
    x4[..., 3] = 0
    w = _randn((cout, 3) + k, 72, 27 ** -0.5)
    bias = _randn((cout,), 73, dtype=F32)
    if wpair:
        kwp = (k[2] + s[2] + 1) // 2 * 2
        wp = _zeros((2, 8, k[0], k[1], kwp, 4))
        for j in range(2):
            wp[j, :cout, :, :, j * s[2]: j * s[2] + k[2], :3] = w.permute(0, 2, 3, 4, 1)
    else:
        kwp = (k[2] + 1) // 2 * 2
        wp = _zeros((cout, k[0], k[1], kwp, 4))
        wp[:, :, :, :k[2], :3] = w.permute(0, 2, 3, 4, 1)

    def desc(lo, hi, y):
        d = L.Conv3dDesc()
        d.x, d.w, d.y, d.shift = _ptr(x4, lo * Si * 4), _ptr(wp), _ptr(y, G + lo * So * cp), _ptr(bias)
        d.x_bs, d.y_bs, d.ldx, d.ldy = Si * 4, So * cp, 4, cp
        d.B, d.Ti, d.Hi, d.Wi, d.cin, d.To, d.Ho, d.Wo, d.cout = hi - lo, T, H, W, 4, To, Ho, Wo, cout
        d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*k, *s, *pad)
        d.act, d.a_act, d.dtype, d.c4_wpair = L.ACT_RELU, L.ACT_NONE, L.PV_BF16, wpair
        return d

    def want():
        return U.ref_tap_conv(x4.cpu()[..., :3], w.cpu(), s, pad, None, bias.cpu(), L.ACT_RELU).reshape(-1, cout)

    unit = None
    if wpair:                                                         # voxel -> its two-output MFMA column
        m = torch.arange(B * So)
        unit = (m // Wo) * Wo2 + (m % Wo) // 2
    _run("stem %d%s" % (cout, " wpair" if wpair else ""), "stem_c4_kernel", "1, 4, 2" if wpair else "2, 4", "pv_conv3d", L.OP_CONV3D,
         desc, B, So, want, cp, 256, [4096], BF16, units_per_clip=To * Ho * Wo2, unit=unit, full=1)
