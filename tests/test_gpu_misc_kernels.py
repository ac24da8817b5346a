"""Direct parity of the pv_rows.hip, pv_pool.hip, pv_layout.hip and pv_segate.hip families on the MI355X: every C-ABI entry of
the row, pooling, layout, SE-gate and head kernels against a float64 CPU reference of the same operation on the same
(bf16-rounded) inputs, at the smallest shapes that reach each branch of the dispatchers, with the routed symbol asserted.

Every case also asserts that the padding channels [C, round_up(C, 8)) of written rows are zero where the kernel's contract
says so, and that a canary (7.0) survives beyond the padding up to the row stride, in rows the launch does not own and in
the gaps behind batch items.  The references and checks live in gpu_util.py (tests/test_misc_kernel_checks.py proves on the
CPU that they fail on a dropped tap, a gamma row of the wrong period and a non-zero padding channel).

Tolerances, relative to the reference abs-max: fp32 1e-3, bf16 1e-2, the SE gate 1e-5; bit equality where nothing is
computed or the arithmetic is exact (max pooling, prefix rows, layout changes that do not narrow, untouched rows, fp32
pv_add_posenc in the kernel's own order); one bf16 rounding (2**-8 per element) where a layout change narrows.

Case -> symbol -> template arguments (the symbol is asserted; the arguments follow from the dispatch condition quoted):

pv_se_gate [pv_segate.hip] (C <= 448 && cr <= 32 && c_p <= 512: fast kernel, cj = ceil(C / 64))
  (64, 8)                          se_gate_fast_kernel<1, 8>     cj <= 1 && cr <= 8
  (65, 8) (128, 8)                 se_gate_fast_kernel<2, 8>     cj <= 2 && cr <= 8
  (129, 8) (48, 16) (256, 16)      se_gate_fast_kernel<4, 16>    cj <= 4 && cr <= 16
  (54, 6) (24, 1)                  se_gate_fast_kernel<1, 8>     cr not a multiple of 4
  (257, 16) (448, 32)              se_gate_fast_kernel<7, 32>    else
  (448, 32) with c_p = 456         se_gate_fast_kernel<7, 32>    c_p above round_up(C, 8)
  (449, 32) (448, 33)              se_gate_kernel                C > 448 | cr > 32
pv_pool3d [pv_pool.hip] (T = float | bf16_t for every kernel)
  (16,7,7) / 432, (8,7,7) / 2048,
  (4,4,4) s2 p1 / 40, (4,4,4) / 4  pool_reduce_kernel<T>         taps >= 64
  (7,3,3), 63 taps                 pool_direct_kernel<T>         taps < 64, not 3x3x3 / 1x3x3
  prefix, 3x3x3                    pool_window_kernel<T, 3, 3, 3> + pool_prefix_kernel<T>
  prefix, 1x3x3                    pool_window_kernel<T, 1, 3, 3> + pool_prefix_kernel<T>
  prefix, 3x3x3 pool_window = 0,
  prefix, 2x2x2                    pool_direct_kernel<T>         + pool_prefix_kernel<T>
  prefix, 4x4x4                    pool_reduce_kernel<T>         + pool_prefix_kernel<T>
pv_ingest_ncdhw [pv_layout.hip]
  generic, six (src, dst) pairs    ingest_kernel<S, T>           c_p = 16: not the 4-channel layout
  c4, frame 9 x 11                 ingest_c4_kernel<S>           S = float | bf16_t | unsigned char; H*W % 8 != 0
  c4, frame 8 x 12                 ingest_c4_vec8_kernel<S>      H*W % 8 == 0, 16-byte aligned planes
  c4, frame 8 x 12, source + 1     ingest_c4_kernel<S>           source pointer not 16-byte aligned
pv_egress_ncdhw [pv_layout.hip]
  four (src, dst) pairs            egress_kernel<T, S>
pv_affine_rows [pv_rows.hip, as every entry below]
  C = 20, x_f32 -> bf16            affine_rows_kernel<float, bf16_t>
  C = 20, fp32 / bf16              affine_rows_kernel<float, float> / <bf16_t, bf16_t>
  8200 x 2048 bf16 in place        affine_rows_kernel<bf16_t, bf16_t>   8200 blocks asked, 8192 launched: second grid trip
pv_layernorm (CG = round_up(C, 8) / 8; same dtype T in and out unless x_f32)
  C = 20, 100; trip C = 24; g_period 16 / 8    layernorm16_kernel<T, T, 16>        CG <= 16
  trip C = 136 (g_period 0 / 16); 51 x 16 rows
  of 136 with g_period 16                      layernorm16_kernel<T, T, 32>        CG <= 32
  C = 260, 384                                 layernorm_kernel<T, T, 1>           CG <= 64
  C = 516                                      layernorm_kernel<T, T, 2>           CG <= 128
  C = 1028                                     layernorm_kernel<T, T, 4>           CG <= 256
  x_f32 C = 48, trip C = 48                    layernorm_f32in_kernel<bf16_t, 16, 1>   2 CG <= 16
  x_f32 C = 100                                layernorm_f32in_kernel<bf16_t, 32, 1>   2 CG <= 32
  x_f32 trip C = 192                           layernorm_f32in_kernel<bf16_t, 64, 1>   2 CG <= 64
  x_f32 C = 260                                layernorm_f32in_kernel<bf16_t, 64, 2>   2 CG <= 128
  x_f32 trip C = 520                           layernorm_f32in_kernel<bf16_t, 64, 4>   CG <= 128
  x_f32 C = 1032, 1536                         layernorm_kernel<float, bf16_t, 4>      CG > 128
  layernorm_kernel<float, bf16_t, 1 | 2> and layernorm16_kernel<float, bf16_t, 16 | 32> do not exist: an x_f32 row of
  CG <= 128 is taken by layernorm_f32in_kernel first, and g_period > 1 refuses x_f32.
pv_softmax_rows   every case       softmax_rows_kernel<T>
pv_mean_rows      every case       mean_rows_kernel<T>
pv_add_posenc     every case       posenc_kernel<T>
pv_add_act        every case       add_act_kernel<T>
pv_ensemble_scores both modes      ensemble_kernel               (no plan op: the entry launches nothing else)
"""
import ctypes as C
import json
import os

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
PV = {torch.float32: L.PV_F32, torch.bfloat16: L.PV_BF16, torch.uint8: L.PV_U8}
_WORST = {}                     # (symbol, dtype) -> worst error any case measured


def _note(symbol, dtype, err):
    key = (symbol, str(dtype).replace("torch.", ""))
    _WORST[key] = max(_WORST.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _record():
    """PV_PARITY_RECORD=path: leave the worst measured error per (symbol, dtype) there (profiles/r11/misc_kernel_parity.md)."""
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump([[k[0], k[1], v] for k, v in sorted(_WORST.items())], f, indent=1)


def _dev(inputs):
    """The case's tensors on the device; one tensor under two names (an in-place launch) stays one tensor."""
    moved, out = {}, {}
    for k, t in inputs.items():
        if t is None:
            out[k] = None
            continue
        if id(t) not in moved:
            moved[id(t)] = t.cuda()
        out[k] = moved[id(t)]
    return out


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(fn, op, fill, inputs, out="y0"):
    """Route on one set of buffers (profiling a plan launches the op twice: in-place ops would run on their own output),
    launch once on a fresh set, return (what the launch left, routed symbol)."""
    d1 = _dev(inputs)
    routed = _routed_kernel(op, fill(d1))
    d2 = _dev(inputs)
    desc = fill(d2)
    call(fn, desc)
    return d2[out], routed


def _status(fn, desc):
    rc = getattr(L.lib(), fn)(C.byref(desc), U.stream())
    torch.cuda.synchronize()
    return rc


def _rows_desc(i, p, dtype):
    d = L.RowsDesc()
    d.x, d.y, d.gamma, d.beta = i["x"].data_ptr(), i["y0"].data_ptr(), _ptr(i.get("gamma")), _ptr(i.get("beta"))
    d.rows, d.C, d.ldx, d.ldy, d.dtype = p["rows"], p["C"], p["ldx"], p["ldy"], PV[dtype]
    d.rows_per_batch, d.eps, d.x_f32, d.g_period = p.get("rows_per_batch", 0), p.get("eps", 0.0), p.get("x_f32", 0), p.get("g_period", 0)
    d.act, d.n_prefix = p.get("act", 0), p.get("n_prefix", 0)
    return d


# ------------------------------------------------------------------ 1. pv_softmax_rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("Cc", [1, 63, 64, 65, 174, 400])
def test_softmax_rows(Cc, rows, inplace, dtype):
    i, p = U.make_softmax(dtype, rows, Cc, inplace)
    got, routed = _run("pv_softmax_rows", L.OP_SOFTMAX_ROWS, lambda t: _rows_desc(t, p, dtype), i)
    assert routed == "softmax_rows_kernel", routed
    _note(routed, dtype, U.check_softmax(got, i, p))


# ------------------------------------------------------------------ 2. pv_mean_rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rpb", [1, 7, 3137])
@pytest.mark.parametrize("Cc", [174, 400])
def test_mean_rows(Cc, rpb, dtype):
    i, p = U.make_mean(dtype, 3, rpb, Cc)
    got, routed = _run("pv_mean_rows", L.OP_MEAN_ROWS, lambda t: _rows_desc(t, p, dtype), i)
    assert routed == "mean_rows_kernel", routed
    _note(routed, dtype, U.check_mean(got, i, p))


def test_mean_rows_refuses_a_ragged_batch_without_a_launch():
    i, p = U.make_mean(torch.float32, 3, 7, 174)
    t = _dev(i)
    d = _rows_desc(t, dict(p, rows=p["rows"] - 1), torch.float32)
    assert _status("pv_mean_rows", d) == L.PV_ERR_INVALID
    assert torch.equal(t["y0"].cpu(), i["y0"])


# ------------------------------------------------------------------ 3. pv_add_posenc
def _posenc_desc(i, p, dtype):
    d = L.PosencDesc()
    d.x, d.cls_token, d.pos_spatial = i["x"].data_ptr(), _ptr(i["cls_token"]), _ptr(i["pos_spatial"])
    d.pos_temporal, d.pos_class = _ptr(i["pos_temporal"]), _ptr(i["pos_class"])
    d.B, d.T, d.HW, d.C, d.ld, d.dtype, d.cls_only = p["B"], p["T"], p["HW"], p["C"], p["ld"], PV[dtype], p["cls_only"]
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc,ld", [(96, 104), (20, 24)])
@pytest.mark.parametrize("form,cls_only", [(f, 0) for f in U.POSENC_FORMS] + [("sep_cls_posclass", 1), ("full_cls", 1)])
def test_add_posenc(form, cls_only, Cc, ld, dtype):
    i, p = U.make_posenc(dtype, form, Cc, ld, cls_only)
    got, routed = _run("pv_add_posenc", L.OP_POSENC, lambda t: _posenc_desc(t, p, dtype), i, out="x")
    assert routed == "posenc_kernel", routed
    _note(routed, dtype, U.check_posenc(got, i, p))      # cls_only: every other row is bit-identical to its input


def test_add_posenc_cls_only_needs_a_cls_token():
    i, p = U.make_posenc(torch.float32, "sep_nocls", 20, 24, cls_only=1)
    t = _dev(i)
    assert _status("pv_add_posenc", _posenc_desc(t, p, torch.float32)) == L.PV_ERR_INVALID
    assert torch.equal(t["x"].cpu(), i["x"])


# ------------------------------------------------------------------ 4. pv_add_act
def _add_desc(i, p, dtype):
    d = L.AddDesc()
    d.a, d.b, d.y = i["a"].data_ptr(), i["b"].data_ptr(), i["y0"].data_ptr()
    d.rows, d.C, d.lda, d.ldb, d.ldy, d.act, d.dtype = p["rows"], p["C"], p["lda"], p["ldb"], p["ldy"], p["act"], PV[dtype]
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [L.ACT_NONE, L.ACT_RELU, L.ACT_SWISH, L.ACT_GELU, L.ACT_SIGMOID])
@pytest.mark.parametrize("Cc", [8, 20, 100])
def test_add_act(Cc, act, dtype):
    for rows, alias in ((1, False), (1031, False), (1031, True)):
        i, p = U.make_add_act(dtype, rows, Cc, act, alias)
        got, routed = _run("pv_add_act", L.OP_ADD_ACT, lambda t: _add_desc(t, p, dtype), i)
        assert routed == "add_act_kernel", routed
        _note(routed, dtype, U.check_add_act(got, i, p))


# ------------------------------------------------------------------ 5 / 6. pv_pool3d
def _pool_desc(i, p, dtype, n_prefix=None):
    To, Ho, Wo = U.pool_out_dims(p)
    d = L.Pool3dDesc()
    d.x, d.y, d.x_bs, d.y_bs, d.ldx, d.ldy = i["x"].data_ptr(), i["y0"].data_ptr(), p["x_bs"], p["y_bs"], p["ldx"], p["ldy"]
    d.B, d.Ti, d.Hi, d.Wi, d.C, d.To, d.Ho, d.Wo = p["B"], p["T"], p["H"], p["W"], p["C"], To, Ho, Wo
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw, d.pt, d.ph, d.pw = (*p["k"], *p["s"], *p["p"])
    d.mode, d.n_prefix, d.dtype = p["mode"], p["n_prefix"] if n_prefix is None else n_prefix, PV[dtype]
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [L.POOL_MAX, L.POOL_AVG])
@pytest.mark.parametrize("B,T,H,W,Cc,k,s,pad,kernel", [
    (2, 16, 7, 7, 432, (16, 7, 7), (1, 1, 1), (0, 0, 0), "pool_reduce_kernel"),    # X3D head: seven channel slabs, the last partial
    (1, 8, 7, 7, 2048, (8, 7, 7), (1, 1, 1), (0, 0, 0), "pool_reduce_kernel"),     # SlowFast head
    (2, 6, 6, 6, 40, (4, 4, 4), (2, 2, 2), (1, 1, 1), "pool_reduce_kernel"),       # 64 taps, padded windows, 256 / 5 not whole
    (1, 4, 4, 4, 4, (4, 4, 4), (1, 1, 1), (0, 0, 0), "pool_reduce_kernel"),        # more tap splits than taps
    (1, 8, 5, 5, 24, (7, 3, 3), (1, 1, 1), (3, 1, 1), "pool_direct_kernel"),       # 63 taps stay on the per-voxel kernel
])
def test_pool3d_large_windows(B, T, H, W, Cc, k, s, pad, kernel, mode, dtype):
    i, p = U.make_pool(dtype, B, T, H, W, Cc, k, s, pad, mode, gap=16)
    got, routed = _run("pv_pool3d", L.OP_POOL3D, lambda t: _pool_desc(t, p, dtype), i)
    assert routed == kernel, routed
    _note(routed, dtype, U.check_pool(got, i, p))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [L.POOL_MAX, L.POOL_AVG])
@pytest.mark.parametrize("T,H,W,Cc,k,s,pad,window,kernel", [
    (4, 6, 6, 96, (3, 3, 3), (1, 2, 2), (1, 1, 1), 1, "pool_window_kernel"),       # MViT's skip-path pool
    (3, 7, 5, 40, (1, 3, 3), (1, 2, 2), (0, 1, 1), 1, "pool_window_kernel"),
    (4, 6, 6, 96, (3, 3, 3), (1, 2, 2), (1, 1, 1), 0, "pool_direct_kernel"),
    (4, 6, 6, 20, (2, 2, 2), (2, 2, 2), (0, 0, 0), 1, "pool_direct_kernel"),
    (6, 6, 6, 40, (4, 4, 4), (2, 2, 2), (1, 1, 1), 1, "pool_reduce_kernel"),
])
def test_pool3d_token_tensor_with_cls_prefix(T, H, W, Cc, k, s, pad, window, kernel, mode, dtype):
    """n_prefix = 1 on (B, 1 + T*H*W, C) tokens with a gap behind each item: the cls row is copied bit-exactly, the pooled rows
    equal the reference of the grid without it."""
    i, p = U.make_pool(dtype, 2, T, H, W, Cc, k, s, pad, mode, n_prefix=1, gap=16)
    try:
        L.tune(pool_window=window)
        got, routed = _run("pv_pool3d", L.OP_POOL3D, lambda t: _pool_desc(t, p, dtype), i)
        pooling = _routed_kernel(L.OP_POOL3D, _pool_desc(_dev(i), p, dtype, n_prefix=0))
    finally:
        L.tune(pool_window=1)
    assert routed == "pool_prefix_kernel" and pooling == kernel, (routed, pooling)
    err = U.check_pool(got, i, p)
    _note(pooling, dtype, err)
    _note(routed, dtype, 0.0)


# ------------------------------------------------------------------ 7. pv_layernorm
def _layernorm_case(dtype, kernel, **kw):
    i, p = U.make_layernorm(dtype, **kw)
    got, routed = _run("pv_layernorm", L.OP_LAYERNORM, lambda t: _rows_desc(t, p, dtype), i)
    assert routed == kernel, routed
    _note(routed + ("(x_f32)" if p["x_f32"] else ""), dtype, U.check_layernorm(got, i, p))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,Cc,kernel", [
    (9, 20, "layernorm16_kernel"), (9, 100, "layernorm16_kernel"), (9, 260, "layernorm_kernel"),   # C not a multiple of 8
    (9, 384, "layernorm_kernel"),                                                                  # MViT's 384: MAXC = 1
    (5, 516, "layernorm_kernel"), (5, 1028, "layernorm_kernel"),                                   # MAXC = 2, 4
])
def test_layernorm_same_dtype_widths(rows, Cc, kernel, dtype):
    _layernorm_case(dtype, kernel, rows=rows, Cc=Cc)


@pytest.mark.parametrize("rows,Cc,kernel", [
    (9, 48, "layernorm_f32in_kernel"), (9, 100, "layernorm_f32in_kernel"), (9, 260, "layernorm_f32in_kernel"),
    (9, 1032, "layernorm_kernel"), (5, 1536, "layernorm_kernel"),          # above 1024 channels: the one-wave-per-row kernel
])
def test_layernorm_fp32_stream_widths(rows, Cc, kernel):
    _layernorm_case(torch.bfloat16, kernel, rows=rows, Cc=Cc, x_f32=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tokens,hd", [(50, 64), (51, 136)])
def test_layernorm_table_of_sixteen_periods(tokens, hd, dtype):
    """heads = 16, hd = 64, 50 tokens; and the one pairing in which the table's alignment rests on the dispatcher rounding the
    grid up to a multiple of g_period: G = 32 (two rows per wave, hd = 136) with sixteen table rows and a row count that
    asks for an odd number of blocks -- a wave's second row group is 8 * gridDim.x rows after its first."""
    _layernorm_case(dtype, "layernorm16_kernel", rows=tokens * 16, Cc=hd, g_period=16, ramp=hd > 64)


@pytest.mark.parametrize("gamma,beta", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("dtype,Cc,x_f32,kernel", [
    (torch.float32, 100, False, "layernorm16_kernel"), (torch.bfloat16, 100, False, "layernorm16_kernel"),
    (torch.float32, 260, False, "layernorm_kernel"), (torch.bfloat16, 260, False, "layernorm_kernel"),
    (torch.bfloat16, 100, True, "layernorm_f32in_kernel")])
def test_layernorm_without_gamma_or_beta(dtype, Cc, x_f32, kernel, gamma, beta):
    _layernorm_case(dtype, kernel, rows=9, Cc=Cc, x_f32=x_f32, gamma=gamma, beta=beta)


# rows of the first grid trip: 4096 blocks (the dispatcher's clamp) x 4 waves x (64 / G) rows per wave x 2 groups in flight
def _first_trip(G):
    return 4096 * 4 * (64 // G) * 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,extra,Cc,g_period", [(16, 37, 24, 0), (32, 5, 136, 0), (16, 37, 24, 8), (32, 5, 136, 16)])
def test_layernorm_narrow_rows_second_grid_trip(G, extra, Cc, g_period, dtype):
    """More rows than one pass of the clamped grid covers, plus a ragged remainder; with a periodic table whose rows differ
    (gamma row i = 1 + i) a lane group that kept the wrong table row on its second trip is off by a factor."""
    _layernorm_case(dtype, "layernorm16_kernel", rows=_first_trip(G) + extra, Cc=Cc, g_period=g_period, ramp=g_period > 0)


@pytest.mark.parametrize("G,Cc", [(16, 48), (64, 192), (64, 520)])        # (G, NL) = (16, 1), (64, 1), (64, 4)
def test_layernorm_fp32_stream_second_grid_trip(G, Cc):
    _layernorm_case(torch.bfloat16, "layernorm_f32in_kernel", rows=_first_trip(G) + 3, Cc=Cc, x_f32=True)


# ------------------------------------------------------------------ 8. pv_affine_rows
@pytest.mark.parametrize("dtype,x_f32,rows,Cc,inplace,act,n_prefix,rpb", [
    (torch.bfloat16, False, 8200, 2048, True, L.ACT_GELU, 1, 41),     # 8200 blocks of work on the 8192-block grid
    (torch.bfloat16, True, 37, 20, False, L.ACT_NONE, 0, 0),
    (torch.float32, False, 37, 20, False, L.ACT_GELU, 0, 0),
    (torch.bfloat16, False, 37, 20, False, L.ACT_RELU, 1, 37),        # out of place: the prefix row is copied through
])
def test_affine_rows(dtype, x_f32, rows, Cc, inplace, act, n_prefix, rpb):
    i, p = U.make_affine(dtype, rows, Cc, x_f32, inplace, act, n_prefix, rpb)
    got, routed = _run("pv_affine_rows", L.OP_AFFINE_ROWS, lambda t: _rows_desc(t, p, dtype), i)
    assert routed == "affine_rows_kernel", routed
    _note(routed + ("(x_f32)" if x_f32 else ""), dtype, U.check_affine(got, i, p))


# ------------------------------------------------------------------ 9. pv_se_gate
def _se_desc(i, p):
    d = L.SeGateDesc()
    d.psum, d.gate, d.w1, d.b1, d.w2, d.b2 = (i[k].data_ptr() for k in ("psum", "y0", "w1", "b1", "w2", "b2"))
    d.B, d.C, d.c_p, d.cr, d.nblk, d.inv_count = p["B"], p["C"], p["c_p"], p["cr"], p["nblk"], p["inv_count"]
    return d


@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("Cc,cr,extra_pad", [
    (64, 8, 0), (65, 8, 0), (128, 8, 0), (129, 8, 0), (48, 16, 0), (256, 16, 0), (257, 16, 0),     # template boundaries
    (448, 32, 0), (449, 32, 0), (448, 33, 0),                                                      # hand-over to the generic kernel
    (54, 6, 0), (24, 1, 0),                                                                        # cr not a multiple of 4
    (448, 32, 8), (20, 8, 8),                                                                      # c_p above round_up(C, 8)
])
def test_se_gate_template_boundaries(Cc, cr, extra_pad, nblk):
    i, p = U.make_se_gate(2, Cc, cr, nblk, extra_pad)
    got, routed = _run("pv_se_gate", L.OP_SE_GATE, lambda t: _se_desc(t, p), i)
    fast = Cc <= 448 and cr <= 32 and p["c_p"] <= 512          # the dispatcher's condition
    assert routed == ("se_gate_fast_kernel" if fast else "se_gate_kernel"), routed
    _note(routed, torch.float32, U.check_se_gate(got, i, p))


# ------------------------------------------------------------------ 10. pv_ingest_ncdhw / pv_egress_ncdhw
def _layout_desc(src, dst, p, src_dtype, dst_dtype, i=None):
    d = L.LayoutDesc()
    d.src, d.dst = src.data_ptr(), dst.data_ptr()
    d.B, d.C, d.T, d.H, d.W, d.c_p, d.ld, d.bs = p["B"], p["C"], p["T"], p["H"], p["W"], p["c_p"], p["ld"], p["bs"]
    d.src_dtype, d.dst_dtype = PV[src_dtype], PV[dst_dtype]
    if i is not None and i["t_index"] is not None:
        d.t_index, d.src_T = i["t_index"].data_ptr(), p["src_T"]
    if i is not None:
        d.ch_scale, d.ch_shift = _ptr(i["ch_scale"]), _ptr(i["ch_shift"])
    return d


def _ingest(i, p, misalign=False):
    src_dtype, dst_dtype = i["src"].dtype, i["y0"].dtype

    def fill(t):
        if misalign:                       # the same values one element past the start of an allocation
            base = torch.empty(i["src"].numel() + 1, dtype=src_dtype, device="cuda")
            base[1:].copy_(t["src"].reshape(-1))
            t["src"] = base[1:].view(i["src"].shape)
            assert t["src"].data_ptr() % 16 != 0
        return _layout_desc(t["src"], t["y0"], p, src_dtype, dst_dtype, t)
    return _run("pv_ingest_ncdhw", L.OP_INGEST, fill, i)


@pytest.mark.parametrize("src_dtype,dst_dtype", [
    (torch.uint8, torch.float32), (torch.uint8, torch.bfloat16), (torch.float32, torch.float32),
    (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("affine,shift", [(False, False), (True, True), (True, False)])
def test_ingest_generic_every_dtype_pair(src_dtype, dst_dtype, affine, shift):
    i, p = U.make_ingest(src_dtype, dst_dtype, 11, 5, 7, 16, 24, affine, shift)
    got, routed = _ingest(i, p)
    assert routed == "ingest_kernel", routed
    _note(routed + ("(affine)" if affine else ""), "%s->%s" % (src_dtype, dst_dtype), U.check_ingest(got, i, p))


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16, torch.uint8])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("Cc", [3, 1])
@pytest.mark.parametrize("H,W,misalign,kernel", [
    (9, 11, False, "ingest_c4_kernel"), (8, 12, False, "ingest_c4_vec8_kernel"), (8, 12, True, "ingest_c4_kernel")])
def test_ingest_first_layer_layout(H, W, misalign, kernel, Cc, affine, src_dtype):
    i, p = U.make_ingest(src_dtype, torch.bfloat16, Cc, H, W, 4, 4, affine)
    got, routed = _ingest(i, p, misalign)
    assert routed == kernel, routed
    _note(routed + ("(affine)" if affine else ""), "%s->%s" % (src_dtype, torch.bfloat16), U.check_ingest(got, i, p))
    if misalign:                           # and the same bits as the 8-voxel kernel on the aligned source
        aligned, routed = _ingest(i, p)
        assert routed == "ingest_c4_vec8_kernel" and torch.equal(aligned, got), routed


@pytest.mark.parametrize("src_dtype,dst_dtype", [
    (torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)])
def test_egress_every_dtype_pair(src_dtype, dst_dtype):
    i, p = U.make_egress(src_dtype, dst_dtype)
    got, routed = _run("pv_egress_ncdhw", L.OP_EGRESS, lambda t: _layout_desc(t["src"], t["y0"], p, src_dtype, dst_dtype), i)
    assert routed == "egress_kernel", routed
    _note(routed, "%s->%s" % (src_dtype, dst_dtype), U.check_egress(got, i, p))


def test_ingest_then_egress_round_trip_is_bit_exact_in_fp32():
    i, p = U.make_ingest(torch.float32, torch.float32, 11, 5, 7, 16, 24, False)
    mid, _ = _ingest(i, p)
    back = torch.full((i["src"].numel() + 16,), U.CANARY, device="cuda")
    call("pv_egress_ncdhw", _layout_desc(mid, back, p, torch.float32, torch.float32))
    assert torch.equal(back[:-16].cpu(), i["src"].reshape(-1)) and torch.all(back[-16:] == U.CANARY)


# ------------------------------------------------------------------ 11. pv_ensemble_scores
@pytest.mark.parametrize("mode", [0, 1])
def test_ensemble_scores_interleaved_videos(mode):
    """Eleven clips in three workgroups, the clips of a video spread over them; indices -1 and V are ignored and counted
    nowhere; accum / counts start non-zero; video 3 receives no clip and keeps its bits."""
    i, p = U.make_ensemble(mode)
    t = _dev(i)
    d = L.EnsembleDesc()
    d.logits, d.video_index, d.accum, d.counts = (t[k].data_ptr() for k in ("logits", "video_index", "accum0", "counts0"))
    d.N, d.C, d.ld, d.V, d.mode = p["N"], p["C"], p["ld"], p["V"], mode
    call("pv_ensemble_scores", d)
    _note("ensemble_kernel(%s)" % ("max" if mode else "sum"), torch.float32, U.check_ensemble((t["accum0"], t["counts0"]), i, p))
