"""Direct parity of the channel-wise stencil kernels on the MI355X -- pv_dwconv.hip, pv_pwdw.hip, pv_tokpool.hip -- through
the C ABI (pv_dwconv3d, pv_dwconv3d_psum_blocks, pv_dwconv3d_pw_supported, pv_token_pool) against a float64 CPU reference of
the same operation on the same (bf16-rounded) inputs, at the smallest shapes that reach each branch of the dispatchers, with
the routed symbol asserted in every case.

Every case also asserts that the padding channels [C, round_up(C, 8)) of written rows are zero, that a canary (7.0) survives
beyond the padding up to the row stride and in the gap behind every batch item, that cls (prefix) rows of pv_dwconv3d are
bit-equal to the input, and -- with psum -- that every entry [b][blk < psum_blocks][c < round_up(C, 8)] of a NaN-filled
buffer became finite, its padding channels exactly 0 (both kernels multiply them by sc = sh = 0), the one block allocated
behind the last still NaN.  The references and checks live in gpu_util.py (tests/test_stencil_kernel_checks.py proves on the CPU
that they fail on a dropped tap, a wrong head's filter, a halo of act(pw_shift), a missing psum tile, a shifted prefix row,
LayerNorm statistics over 16-lane width, a non-zero padding channel and a touched canary).

Tolerances, relative to the reference abs-max: y fp32 1e-3, bf16 1e-2 (gpu_util.TOL); the mean over T,H,W taken from psum
1e-3, from the fused producer's 2e-3; fused against the unfused pv_conv3d -> pv_dwconv3d pair 2e-3; the same inputs on
4-wide and 2-wide lanes 4e-3.  The fused producer's reference rounds where the kernel does: conv_a + affine + activation in
float64, rounded to bf16, zero outside the image, then the depthwise conv in float64.

The symbol carries no template arguments; they follow from the dispatch condition quoted, and for NW from the block count:
pv_dwconv3d_psum_blocks == ceil(Ho / 4) * ceil(Wo / (4 NW)) for the plane kernels, ceil(To Ho ceil(Wo / nw) / gpb) with
gpb = 256 / (round_up(C, 8) / 8) for the generic kernel (nw = 4 outputs per thread for kw = 3, sw <= 2 and for kw = 1,
sw = 1; else 1).  Both are asserted.

Case -> symbol -> template arguments <- dispatch condition

pv_dwconv3d, generic (T = float | bf16_t unless stated; B = 2 with a batch gap)
  1   (1,3,3) s1, 3x5x6, C 20, psum        dwconv_kernel<T, 3, 1, 4>   kw = 3, sw = 1; bf16 stays here: kt != 3
  2   (3,3,3) s2 p1, 4x7x9, C 53, psum     dwconv_kernel<T, 3, 2, 4>   kw = 3, sw = 2; bf16 stays here: st = 2
  3   (3,1,1) s(2,1,1), 5x4x5, C 24        dwconv_kernel<T, 1, 1, 4>   kw = 1, sw = 1, gw = 0
  4a  (1,5,5) s1, 2x5x6, C 54, psum        dwconv_kernel<T, 0, 1, 1>   kw = 5; CG = 7, gpb = 36: threads 252..255 idle
  4b  (3,3,3) s(1,3,3), 4x8x11, C 54, psum dwconv_kernel<T, 0, 1, 1>   sw = 3; the same idle threads
  5   (3,3,3), 2x3x5, C 640, psum, fp32    dwconv_kernel<float, 3, 1, 4>   LDS 69120 + 7680 B in (64 KB, 96 KB]: hipFuncSetAttribute
  6   (3,3,3), 2x3x5, C 896, psum, fp32    dwconv_kernel<float, 3, 1, 4>   96768 B of taps fit, + 7168 B do not: w_global, s_red at 0
  7   gw 8 (3,3,3), B 1, 2x3x3, C 128, psum  dwconv_kernel<T, 0, 1, 1>  gw > 1; 110592 B of taps: w_global, grouped
  8   (3,3,3) p1, 4x5x6, heads 2, w_mod 96,
      n_prefix 1, x = k of q|k|v, ldy 200  dwconv_kernel<T, 3, 2, 4> + dw_prefix_kernel<T>   fp32 s(1,2,2); bf16 s(2,2,2): st = 2
pv_dwconv3d, bf16 3x3x3 st 1 pad 1 (B = 3: ntiles * B not a multiple of 8; C 53, ldx = ldy = 64, batch gap)
  S 1, 5x9 (NW 2) | 5x17 (NW 4), T 1..4,
  every ACT, psum on | off             dw3_plane_kernel<1, NW, ACT>    sw = 1; NW 4 <- dw_wide_min_wo = 1, NW 2 <- above Wo
  S 2, 10x18 | 9x33, T 1 | 3,
  every ACT, psum on | off             dw3_plane_kernel<2, NW, ACT>    sw = 2; same knob
  C 8 (S 1, NW 2), C 40 (S 2, NW 4)    dw3_plane_kernel<S, NW, SWISH>  12 of 16 channel pairs idle; second slab of one chunk
  n_prefix 1, w_mod 96, C 192          dw3_plane_kernel<1, 2, NONE> + dw_prefix_kernel<bf16_t>   n_prefix > 0, no psum
  1x2x4x64 | 1x2x4x63, C 8, no knob    dw3_plane_kernel<1, 4 | 2, RELU>  Wo >= 64 (the default dw_wide_min_wo)
  All twelve <S, NW, ACT> are reached.
pv_dwconv3d with pw_w (bf16; B = 2, H = 5; KS = ceil(pw_cin / 32) for pw_cin 24, 40, 96, 128, 192)
  every KS x S x NW x ACT              pwdw_plane_kernel<S, NW, KS, ACT>   NW 4 <- Wo = 13 >= 12, NW 2 <- Wo = 9
  All sixty <S, NW, KS, ACT> are reached; T 1 | 3, pw_act NONE | RELU, C 24 | 53 and ldx = round_up(pw_cin, 8) (+ 16) alternate.
  pw_cin 136 | 200, w_mod, n_prefix, pw_act SWISH, narrow ldx: refused before anything is launched.
pv_token_pool (T = float | bf16_t; every ld wider than heads * head_dim, batch gap)
  (1,3,3) (3,1,1) (2,2,2); (1,3,3)
  without gamma / beta                 token_pool_kernel<T, false>     kernel != 3x3x3
  head_dim 8 | 104 | 128, n 1..3,
  no gamma / beta, second grid trip    token_pool_kernel<T, true>      3x3x3
  All four <T, K333> are reached.
  No descriptor reaches a dwconv_kernel<T, KW, SW, NW> other than <3,1,4>, <3,2,4>, <1,1,4>, <0,1,1>: launch_dw names no other.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
PV = {torch.float32: L.PV_F32, torch.bfloat16: L.PV_BF16}
ACT_NAME = {L.ACT_NONE: "NONE", L.ACT_RELU: "RELU", L.ACT_SWISH: "SWISH"}
ACTS = [L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH]
K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)
WIDE_DEFAULT = 64               # dw_wide_min_wo as the library ships it
_WORST, _NOTES, _T0 = {}, {}, time.perf_counter()


def _note(symbol, dtype, err):
    key = (symbol, str(dtype).replace("torch.", ""))
    _WORST[key] = max(_WORST.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """PV_PARITY_RECORD=path: leave the worst measured error per (symbol, dtype) there (profiles/r18/stencil_kernel_parity.md)."""
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({"seconds": round(time.perf_counter() - _T0, 2), "notes": _NOTES,
                       "worst": [[k[0], k[1], v] for k, v in sorted(_WORST.items())]}, f, indent=1)


def _dev(inputs):
    return {k: [None if t is None else t.cuda() for t in v] if isinstance(v, list) else (None if v is None else v.cuda())
            for k, v in inputs.items()}


def _status(fn, desc):
    rc = getattr(L.lib(), fn)(C.byref(desc), U.stream())
    torch.cuda.synchronize()
    return rc


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ pv_dwconv3d
def _dw_desc(t, p, dtype, psum=None):
    d = U.fill_dw_geometry(L.DwConv3dDesc(), p, dtype)
    d.x = t["x"].data_ptr() + p["x_off"] * t["x"].element_size()
    d.w, d.y, d.scale, d.shift = (t[k].data_ptr() for k in ("w", "y0", "scale", "shift"))
    if p.get("pw_cin", 0):
        d.pw_w, d.pw_scale, d.pw_shift = (t[k].data_ptr() for k in ("pw_w", "pw_scale", "pw_shift"))
    if psum is not None:
        d.psum = psum.data_ptr()
    return d


def _generic_blocks(p, nw):
    To, Ho, Wo = U.conv_out_dims(p)
    return _cdiv(To * Ho * _cdiv(Wo, nw), 256 // (U.round_up8(p["C"]) // 8))


def _plane_blocks(p, NW):
    To, Ho, Wo = U.conv_out_dims(p)
    return _cdiv(Ho, 4) * _cdiv(Wo, 4 * NW)


def _run_dw(i, p, dtype, want_psum, blocks):
    """Route on one set of buffers, launch once on a fresh set -> (y, psum | None, routed symbol).  `blocks` is the block
    count the dispatch condition predicts; pv_dwconv3d_psum_blocks must report it with and without the psum pointer."""
    lib = L.lib()
    t1 = _dev(i)
    nblk = lib.pv_dwconv3d_psum_blocks(C.byref(_dw_desc(t1, p, dtype)))
    assert nblk == blocks, (nblk, blocks)

    def psum_buf():
        return torch.full((p["B"] * nblk + 1, U.round_up8(p["C"])), float("nan"), device="cuda") if want_psum else None
    psum1 = psum_buf()
    d1 = _dw_desc(t1, p, dtype, psum1)
    assert lib.pv_dwconv3d_psum_blocks(C.byref(d1)) == blocks
    routed = _routed_kernel(L.OP_DWCONV3D, d1)
    t2, psum = _dev(i), psum_buf()
    call("pv_dwconv3d", _dw_desc(t2, p, dtype, psum))
    return t2["y0"], psum, routed


def _check_dw(i, p, dtype, want_psum, blocks, symbol, label):
    got, psum, routed = _run_dw(i, p, dtype, want_psum, blocks)
    assert routed == symbol, routed
    err, perr = U.check_dwconv(got, i, p, psum, blocks)
    _note(label, dtype, err)
    if perr is not None:
        _note(label + " psum mean", dtype, perr)
    return got


GENERIC = {     # case: (dtypes, B, T, H, W, C, k, s, pad, act, psum, nw, <KW, SW, NW>, extras)
    "1": (DTYPES, 2, 3, 5, 6, 20, (1, 3, 3), S1, (0, 1, 1), L.ACT_SWISH, True, 4, "3, 1, 4", {}),
    "2": (DTYPES, 2, 4, 7, 9, 53, K3, (2, 2, 2), P1, L.ACT_RELU, True, 4, "3, 2, 4", {}),
    "3": (DTYPES, 2, 5, 4, 5, 24, (3, 1, 1), (2, 1, 1), (1, 0, 0), L.ACT_NONE, False, 4, "1, 1, 4", {}),
    "4a": (DTYPES, 2, 2, 5, 6, 54, (1, 5, 5), S1, (0, 2, 2), L.ACT_RELU, True, 1, "0, 1, 1", {}),
    "4b": (DTYPES, 2, 4, 8, 11, 54, K3, (1, 3, 3), P1, L.ACT_SWISH, True, 1, "0, 1, 1", {}),
    "5": (DTYPES[:1], 2, 2, 3, 5, 640, K3, S1, P1, L.ACT_RELU, True, 4, "3, 1, 4", {}),
    "6": (DTYPES[:1], 2, 2, 3, 5, 896, K3, S1, P1, L.ACT_SWISH, True, 4, "3, 1, 4", {}),
    "7": (DTYPES, 1, 2, 3, 3, 128, K3, S1, P1, L.ACT_RELU, True, 1, "0, 1, 1", dict(gw=8)),
}


@pytest.mark.parametrize("case,dtype", [(c, dt) for c, v in GENERIC.items() for dt in v[0]])
def test_generic_depthwise_kernel(case, dtype):
    _, B, T, H, W, Cc, k, s, pad, act, psum, nw, targs, extras = GENERIC[case]
    i, p = U.make_dwconv(dtype, B, T, H, W, Cc, k, s, pad, act, ldx=U.round_up8(Cc) + 8, ldy=U.round_up8(Cc) + 16, **extras)
    # the branch the case is here for, from the dispatcher's own arithmetic (pv_dwconv.hip geom / launch_variant)
    cp, gw = U.round_up8(Cc), max(p["gw"], 1)
    gpb = 256 // (cp // 8)
    w_bytes, red_bytes = 4 * k[0] * k[1] * k[2] * gw * cp, 4 * gpb * cp * int(psum)
    if case in ("4a", "4b"):
        assert gpb * (cp // 8) == 252                        # threads 252..255 own no unit and must stay out of s_red
    if case == "5":
        assert (w_bytes, red_bytes) == (69120, 7680) and 64 * 1024 < w_bytes + red_bytes <= 96 * 1024
    if case == "6":
        assert w_bytes <= 96 * 1024 < w_bytes + red_bytes and red_bytes == 7168
    if case == "7":
        assert w_bytes == 110592 > 96 * 1024
    _check_dw(i, p, dtype, psum, _generic_blocks(p, nw), "dwconv_kernel",
              "dwconv_kernel<%s, %s>%s" % ("float" if dtype == torch.float32 else "bf16_t", targs,
                                           " w_global" if w_bytes + red_bytes > 96 * 1024 else ""))


@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_depthwise_on_a_fused_qkv_slice_with_shared_filter_and_cls_row(dtype):
    """Case 8: x is the k third of a (q | k | v) token buffer (ldx = 3 * 192), one 96-channel filter shared by two heads, the
    cls row copied by dw_prefix_kernel, ldy = 200."""
    stride = (1, 2, 2) if dtype == torch.float32 else (2, 2, 2)
    i, p = U.make_dwconv(dtype, 2, 4, 5, 6, 192, K3, stride, P1, L.ACT_NONE, w_mod=96, n_prefix=1, ldy=200, qkv=True)
    assert p["ldx"] == 3 * 192 and p["x_off"] == 192
    _check_dw(i, p, dtype, False, _generic_blocks(p, 4), "dwconv_kernel",
              "dwconv_kernel<%s, 3, 2, 4> w_mod + dw_prefix_kernel" % ("float" if dtype == torch.float32 else "bf16_t"))


# ------------------------------------------------------------------ dw3_plane_kernel
def _plane_case(S, NW, act, T, H, W, Cc=53, psum=True, B=3, knob=True, **kw):
    ld = dict(ldx=64, ldy=64) if Cc <= 56 else {}
    i, p = U.make_dwconv(torch.bfloat16, B, T, H, W, Cc, K3, (1, S, S), P1, act, **ld, **kw)
    try:
        if knob:
            L.tune(dw_wide_min_wo=1 if NW == 4 else 1 << 30)
        got = _check_dw(i, p, torch.bfloat16, psum, _plane_blocks(p, NW), "dw3_plane_kernel",
                        "dw3_plane_kernel<%d, %d, %s>" % (S, NW, ACT_NAME[act]))
    finally:
        L.tune(dw_wide_min_wo=WIDE_DEFAULT)
    assert _plane_blocks(p, 2) != _plane_blocks(p, 4)        # the block count tells the two widths apart
    return got


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("NW,H,W", [(2, 5, 9), (4, 5, 17)])
def test_plane_kernel_stride_1_both_exits_of_the_two_plane_walk(NW, H, W, T, act):
    """T = 1: the plane without a temporal neighbour; odd and even T leave the double-buffered loop by its two exits.  C = 53
    splits the last channel pair between a real and a padding channel; B = 3 leaves the padded grid's last tiles empty."""
    _plane_case(1, NW, act, T, H, W, psum=(T + act) % 2 == 0)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H,W", [(10, 18), (9, 33)])
@pytest.mark.parametrize("NW", [2, 4])
def test_plane_kernel_stride_2_even_and_odd_grids(NW, H, W, T, act):
    """Even grid: the last halo row and column lie outside the image; odd grid: inside it."""
    _plane_case(2, NW, act, T, H, W, psum=(T // 2 + act) % 2 == 0)


@pytest.mark.parametrize("S,NW,H,W,Cc", [(1, 2, 5, 9, 8), (2, 4, 9, 33, 40)])
def test_plane_kernel_idle_channel_pairs_and_a_one_chunk_second_slab(S, NW, H, W, Cc):
    i_ld = dict(ldx=U.round_up8(Cc) + 8, ldy=U.round_up8(Cc) + 16)
    i, p = U.make_dwconv(torch.bfloat16, 3, 3, H, W, Cc, K3, (1, S, S), P1, L.ACT_SWISH, **i_ld)
    try:
        L.tune(dw_wide_min_wo=1 if NW == 4 else 1 << 30)
        _check_dw(i, p, torch.bfloat16, True, _plane_blocks(p, NW), "dw3_plane_kernel", "dw3_plane_kernel<%d, %d, SWISH>" % (S, NW))
    finally:
        L.tune(dw_wide_min_wo=WIDE_DEFAULT)


def test_plane_kernel_with_cls_row_and_shared_filter():
    """n_prefix = 1, no psum: dw_prefix_kernel<bf16_t> copies the cls row, the plane kernel skips it; w_mod = 96 over two heads."""
    _plane_case(1, 2, L.ACT_NONE, 3, 5, 9, Cc=192, psum=False, n_prefix=1, w_mod=96, ldx=200, ldy=208)


@pytest.mark.parametrize("W,NW", [(64, 4), (63, 2)])
def test_plane_kernel_default_width_threshold(W, NW):
    """No knob: Wo >= 64 takes 4 outputs per lane (X3D-L's res2), Wo = 63 takes 2."""
    _plane_case(1, NW, L.ACT_RELU, 2, 4, W, Cc=8, B=1, knob=False)


@pytest.mark.parametrize("S,H,W", [(1, 5, 17), (2, 9, 33)])
def test_plane_kernel_lane_widths_agree(S, H, W):
    """The same inputs at NW = 2 and NW = 4 sum the same products: within 4e-3 of the abs-max (bit-equal is recorded)."""
    outs = [_plane_case(S, NW, L.ACT_SWISH, 3, H, W).cpu() for NW in (2, 4)]
    err = U.rel_err(outs[0], outs[1])
    _NOTES["dw3_plane_kernel<%d> NW 2 vs NW 4" % S] = "bit-equal" if torch.equal(outs[0], outs[1]) else "differ by %.3e" % err
    assert err <= 4e-3, err


# ------------------------------------------------------------------ pwdw_plane_kernel
def _unfused_pair(i, p):
    """pv_conv3d (conv_a) into a dense buffer, then pv_dwconv3d on it: the same bf16 rounding point as the fused launch."""
    B, T, H, W, Cc, cin = p["B"], p["T"], p["H"], p["W"], p["C"], p["pw_cin"]
    cp, cinp = U.round_up8(Cc), U.round_up8(cin)
    t = _dev(i)
    hbuf = torch.zeros(B, T * H * W * cp, dtype=torch.bfloat16, device="cuda")
    wa8 = torch.zeros(Cc, cinp, dtype=torch.bfloat16, device="cuda")
    wa8[:, :cin] = t["wa"]
    c = L.Conv3dDesc()
    c.x, c.w, c.y, c.scale, c.shift = t["x"].data_ptr(), wa8.data_ptr(), hbuf.data_ptr(), t["pw_scale"].data_ptr(), t["pw_shift"].data_ptr()
    c.x_bs, c.y_bs, c.ldx, c.ldy = p["x_bs"], T * H * W * cp, p["ldx"], cp
    c.B, c.Ti, c.Hi, c.Wi, c.cin, c.To, c.Ho, c.Wo, c.cout = B, T, H, W, cinp, T, H, W, Cc
    c.kt = c.kh = c.kw = c.st = c.sh = c.sw = 1
    c.act, c.a_act, c.dtype = p["pw_act"], L.ACT_NONE, L.PV_BF16
    call("pv_conv3d", c)
    q = dict(p, pw_cin=0, pw_act=0, ldx=cp, x_bs=T * H * W * cp)
    t["x"] = hbuf
    call("pv_dwconv3d", _dw_desc(t, q, torch.bfloat16))
    return t["y0"]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("nw_i", [0, 1])
@pytest.mark.parametrize("s_i", [0, 1])
@pytest.mark.parametrize("ks_i,cin", enumerate([24, 40, 96, 128, 192]))
def test_fused_pointwise_producer(ks_i, cin, s_i, nw_i, act):
    """conv_a + affine + act_a computed per halo tile in front of the depthwise 3x3x3: every <S, NW, KS, ACT>.  pw_cin = 40 leaves
    a ragged K tail; T, pw_act, C and a wider ldx alternate over the cases so that each meets every KS, S and NW."""
    KS, S, NW, a = _cdiv(cin, 32), 1 + s_i, (2, 4)[nw_i], ACTS.index(act)
    assert KS == (1, 2, 3, 4, 6)[ks_i]
    Wo = (9, 13)[nw_i]
    W = Wo if S == 1 else 2 * Wo - 1
    T = 1 if (ks_i + s_i + a) % 2 == 0 else 3
    pw_act = L.ACT_RELU if (ks_i + nw_i + a) % 2 else L.ACT_NONE
    Cc = 53 if (ks_i + s_i + nw_i + a) % 2 else 24
    i, p = U.make_pwdw(2, T, 5, W, cin, Cc, S, act, pw_act, wide_ldx=(s_i + nw_i + a) % 2 == 1)
    assert U.conv_out_dims(p)[2] == Wo and _plane_blocks(p, 2) != _plane_blocks(p, 4)
    assert L.lib().pv_dwconv3d_pw_supported(C.byref(_dw_desc(_dev(i), p, torch.bfloat16))) == 1
    got = _check_dw(i, p, torch.bfloat16, True, _plane_blocks(p, NW), "pwdw_plane_kernel", "pwdw_plane_kernel<%d, %d, %d>" % (S, NW, KS))
    if (s_i, nw_i, a) == (ks_i % 2, (ks_i // 2) % 2, ks_i % 3):        # one case per KS: the unfused pair gives the same bits
        err = U.rel_err(got, _unfused_pair(i, p))
        _note("pwdw_plane_kernel<%d, %d, %d> vs unfused pair" % (S, NW, KS), torch.bfloat16, err)
        assert err <= 2e-3, err


@pytest.mark.parametrize("change", [dict(pw_cin=136), dict(pw_cin=200), dict(w_mod=8), dict(n_prefix=1), dict(pw_act=L.ACT_SWISH),
                                    dict(ldx=16)], ids=lambda c: "%s=%s" % next(iter(c.items())))
def test_fused_pointwise_producer_refusals_launch_nothing(change):
    """ceil(pw_cin / 32) of 5 or 7, a shared filter, a cls row, a SWISH producer, rows narrower than pw_cin: not supported, and
    pv_dwconv3d says so without touching y."""
    cin = change.get("pw_cin", 24)
    i, p = U.make_pwdw(2, 1, 5, 9, cin, 24, 1, L.ACT_RELU, L.ACT_RELU)
    ok = _dw_desc(_dev(i), p, torch.bfloat16)
    if "pw_cin" not in change:
        assert L.lib().pv_dwconv3d_pw_supported(C.byref(ok)) == 1
    t = _dev(i)
    d = _dw_desc(t, dict(p, **change), torch.bfloat16)
    assert L.lib().pv_dwconv3d_pw_supported(C.byref(d)) == 0
    assert _status("pv_dwconv3d", d) == L.PV_ERR_UNSUPPORTED
    assert torch.equal(t["y0"].cpu(), i["y0"])


# ------------------------------------------------------------------ token_pool_kernel
def _tp_desc(t, p, dtype):
    d = L.TokenPoolDesc()
    for z in range(p["n"]):
        d.x[z], d.y[z], d.w[z] = t["x"][z].data_ptr(), t["y0"][z].data_ptr(), t["w"][z].data_ptr()
        d.gamma[z] = None if t["gamma"][z] is None else t["gamma"][z].data_ptr()
        d.beta[z] = None if t["beta"][z] is None else t["beta"][z].data_ptr()
        d.x_bs[z], d.y_bs[z], d.ldx[z], d.ldy[z] = p["x_bs"][z], p["y_bs"][z], p["ldx"][z], p["ldy"][z]
        d.st[z], d.sh[z], d.sw[z] = p["strides"][z]
        d.To[z], d.Ho[z], d.Wo[z] = U.token_pool_out_dims(p, z)
    d.n, d.B, d.Ti, d.Hi, d.Wi, d.heads, d.head_dim = p["n"], p["B"], p["T"], p["H"], p["W"], p["heads"], p["hd"]
    d.kt, d.kh, d.kw = p["k"]
    d.n_prefix, d.eps, d.dtype = p["n_prefix"], p["eps"], PV[dtype]
    return d


def _check_tp(i, p, dtype, k333):
    assert (p["k"] == K3) == k333
    routed = _routed_kernel(L.OP_TOKEN_POOL, _tp_desc(_dev(i), p, dtype))
    assert routed == "token_pool_kernel", routed
    t = _dev(i)
    call("pv_token_pool", _tp_desc(t, p, dtype))
    _note("token_pool_kernel<%s, %s>" % ("float" if dtype == torch.float32 else "bf16_t", "true" if k333 else "false"), dtype,
          U.check_token_pool(t["y0"], i, p))


STRIDES = [(1, 1, 1), (1, 2, 2), (2, 2, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [(1, 3, 3), (3, 1, 1), (2, 2, 2)])
def test_token_pool_kernels_other_than_3x3x3(k, dtype):
    """K333 = false: the runtime tap loops; the even kernel's output size follows padding = k / 2."""
    i, p = U.make_token_pool(dtype, 2, 2, 16, (3, 5, 6), k, STRIDES[:2], 1, wide=True, gap=16)
    if k == (2, 2, 2):
        assert U.token_pool_out_dims(p, 0) == (4, 6, 7)
    _check_tp(i, p, dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("hd", [8, 104, 128])
def test_token_pool_head_dim_mask_and_tensors_of_unequal_length(hd, n, dtype):
    """heads = 3; head_dim 8 leaves 15 of 16 lanes idle, 104 three, 128 none.  Every tensor has its own stride: the shorter
    ones idle through part of the grid sized for the longest."""
    i, p = U.make_token_pool(dtype, 2, 3, hd, (2, 4, 5), K3, STRIDES[:n], 1, wide=True, gap=16)
    _check_tp(i, p, dtype, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_pool_second_grid_trip(dtype):
    """804 (token, head) units against 43 resident workgroups of 16: the grid-stride loop runs a second, ragged trip."""
    i, p = U.make_token_pool(dtype, 16, 4, 8, (2, 10, 10), K3, STRIDES, 1, wide=True, gap=16)
    units, resident = (1 + 200) * 4, _cdiv(256 * 8, 16 * 3)
    assert (units, resident) == (804, 43) and resident * 16 < units < 2 * resident * 16
    _check_tp(i, p, dtype, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [K3, (1, 3, 3)])
@pytest.mark.parametrize("gamma,beta", [(False, False), (True, False)])
def test_token_pool_without_normalisation_and_with_gamma_alone(gamma, beta, k, dtype):
    """gamma = beta = NULL: the output is the pooled value (the cls row bit-equal); gamma alone: normalised, no bias."""
    i, p = U.make_token_pool(dtype, 2, 2, 24, (2, 4, 5), k, STRIDES[1:], 1, gamma=gamma, beta=beta, wide=True, gap=16)
    _check_tp(i, p, dtype, k == K3)


@pytest.mark.parametrize("change,status", [
    (dict(k=(5, 5, 3)), L.PV_ERR_UNSUPPORTED),       # 75 taps
    (dict(hd=136), L.PV_ERR_UNSUPPORTED),
    (dict(hd=12), L.PV_ERR_UNSUPPORTED),
    (dict(Wo=1), L.PV_ERR_INVALID),                  # not nn.Conv3d's output size
], ids=["taps", "head_dim_136", "head_dim_12", "output_size"])
def test_token_pool_refusals_launch_nothing(change, status):
    i, p = U.make_token_pool(torch.float32, 2, 2, 16, (2, 4, 5), K3, STRIDES[:2], 1, wide=True, gap=16)
    t = _dev(i)
    d = _tp_desc(t, dict(p, **{k: v for k, v in change.items() if k != "Wo"}), torch.float32)
    if "Wo" in change:
        d.Wo[1] += change["Wo"]
    assert _status("pv_token_pool", d) == status
    assert all(torch.equal(a.cpu(), b) for a, b in zip(t["y0"], i["y0"]))
