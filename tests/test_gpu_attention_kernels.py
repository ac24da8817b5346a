"""Direct parity of the attention kernels of csrc/pv_attn64.hip and csrc/pv_attn.hip on the MI355X, through pv_attention, per key,
per tile step and across rescales.  Every case runs for each route and asserts the routed symbol:

    bf16, head_dim 96        attn_w64_kernel            K in a 2-slot ring, V in a 3-slot ring, two staging sets, loads 5 tiles ahead
    bf16, head_dim 64, 32    attn_pipe_kernel<D>        scores one tile ahead, K and V double buffers
    bf16, head_dim 128       attn_kernel<bf16_t, 128>   NBUF = 2
    fp32, 32 / 64 / 96 / 128 attn_kernel<float, D>      KT = 32, one buffer

(attn_kernel<bf16_t, 32 | 64 | 96> takes over only where K / V lie beyond 2 GiB: out of reach here, named in the record.)

tests/test_gpu_kernels.py launches them on randn operands under one number per launch, max|got - want| / max|want| <= 1e-2: with unit
score variance no tile's maximum exceeds the held one by more than kDefer after start-up, so `l_run *= alpha` can be missing from
every later rescale without moving that number, and the spiked cases rescale by 2^-60 only.  Here every reference is a float64
softmax of the operands the kernel reads (gpu_util.ref_attention), built on the CPU, and a failure names batch item, head, query
row, work item, wave, lane, channel, channel block and the key tile and step form of the row's dominant key (gpu_util.AttnExpect).

A  selection (gpu_util.make_attn_select): K rows are +-1 codes, q_i = 64 k_t(i) with t(i) = (a i + b) mod Nk, V distinct integer
   rows, scale 0.0866... whose fp32 product with log2 e is exactly 0.125: the selected exponent argument is 8 D, every other at
   least 40 below (asserted before the launch).  bf16: output row i is bit-equal to v[t(i)], with residual_q to v[t(i)] + q_i.
   fp32: |got - want| <= 2^-21 |want| per element.  Nk = 1, 3, 37, 64, 65, 128, 192, 256, 448, 485, 512 (fp32: the same tile counts
   at KT = 32): every key position, every ring slot, staging set and tail form, the ragged mask at keys Nk - 1 and Nk, the lane
   half exchange, a rescale by at least 2^-40 at every tile index
B  integer score levels (gpu_util.make_attn_levels): exponent arguments are integers that follow a per-tile schedule (flat, +7, +8,
   +9 per tile, falling, saw, one lane alone tripping __any); V in [1, 8].  The mirror of the rescale rule (gpu_util.attn_mirror)
   asserts before the launch that the cases of a route contain a held maximum at a rise of exactly 8, a rescale at 9, a stale P of
   2^8, the one-lane rescale, and a moderate rescale in a `more` step of each parity, a last and a ragged last step.
   bf16: |got - want| <= 2^-7 |want| per element; fp32: 2 (Nk + 8) 2^-24 |want|
C  normal operands at score variance 1, 4 and 12, the project's TOL applied per QUERY ROW (max|d| over the row / max|want| over it)
D  where the data lies: ld all different and wider than the row, q / k / v as channel slices of one buffer, gaps between items;
   NaN in every element of Q, K and V that is no operand (pad channels, gap rows, 6 key tiles of rows behind the last item -- in
   EVERY case of this file), the canary in every element of O the launch does not own.  Edges: Nk = 1 .. 4, Nq = 1, 31, 32, 33,
   127, 128, 129, B heads nqb = 1, 7, 9, 17 (the XCD order's remainder branch)
E  sub-launches through offset pointers (whole query blocks, single heads, single batch items) give the full launch's bits

PV_PARITY_RECORD=path leaves the table of the run there (profiles/r34/attention_kernel_parity.md)."""
import functools
import os
import time

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
CFGS = sorted(U.ATTN_ROUTES, key=lambda c: (c[0] == F32, c[1]))
CFG_IDS = ["%s_%d" % ("bf16" if c[0] == BF16 else "fp32", c[1]) for c in CFGS]
_REC, _FORMS = [], set()


@pytest.fixture(scope="module", autouse=True)
def _record():
    t0 = time.perf_counter()
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if not path:
        return
    with open(path, "w") as f:
        f.write("| case | routed kernel | Nk | tiles, step forms reached | worst error | bound | bit checks |\n|---|---|---|---|---|---|---|\n")
        for r in _REC:
            f.write("| %s | `%s` | %s | %s | %s | %s | %s |\n" % (r["case"], r["kernel"], r["Nk"], r["forms"], r["err"], r["bound"], r["bits"]))
        f.write("\ninstantiations launched (%d):\n" % len(_FORMS))
        for k in sorted(_FORMS):
            f.write("- `%s`\n" % k)
        f.write("\nnot launched (K / V beyond 2 GiB only):\n")
        for k in U.ATTN_NOT_LAUNCHED:
            f.write("- `%s`\n" % k)
        f.write("\nwhole module: %.1f s\n" % (time.perf_counter() - t0))


def _forms(Nk, KT):
    nt = U.cdiv(Nk, KT)
    more = sorted({(t & 1, t % 3) for t in range(nt - 1)})
    last = "ragged last" if Nk % KT else "last"
    return "%d: prologue%s, %s" % (nt, "".join(", more p%d v%d" % m for m in more), last)


def _rec(case, cfg, Nk, err=None, bound=None, bits="-"):
    kernel, form = U.ATTN_ROUTES[cfg]
    _FORMS.add(form)
    nks = Nk if isinstance(Nk, (tuple, list)) else (Nk,)
    _REC.append(dict(case=case, kernel=kernel, Nk=", ".join(str(n) for n in nks), forms="; ".join(_forms(n, U.attn_kt(cfg[0])) for n in nks),
                     err="-" if err is None else "%.2e" % err, bound=bound or "-", bits=bits))


class _Attn:
    """The operands of one pv_attention case on the device, in a layout; run() launches a sub-range into a fresh canary buffer."""

    def __init__(self, o, cfg, kind="packed"):
        self.o, self.cfg, (self.dtype, self.D) = o, cfg, cfg
        B, Nq, H, D = o["q"].shape
        assert D == self.D
        self.lay = U.AttnLayout(kind, B, H, D, Nq, o["k"].shape[1], self.dtype)
        host = self.lay.inputs(o["q"], o["k"], o["v"])
        self.dev = {}
        for x in "qkv":                      # fused: one device buffer under three names
            self.dev[x] = next((self.dev[y] for y in self.dev if host[y] is host[x]), None)
            if self.dev[x] is None:
                self.dev[x] = host[x].cuda()
        self.keep = []

    def run(self, residual, b=None, h=None, rows=None):
        lay = self.lay
        b, h, rows = b or (0, lay.B), h or (0, lay.H), rows or (0, lay.Nq)
        out = lay.output().cuda()
        d = L.AttentionDesc()
        es = out.element_size()
        at = lambda t, x, r0: t.data_ptr() + (lay.off[x] + b[0] * lay.bs[x] + r0 * lay.ld[x] + h[0] * lay.D) * es
        d.q, d.k, d.v, d.o = at(self.dev["q"], "q", rows[0]), at(self.dev["k"], "k", 0), at(self.dev["v"], "v", 0), at(out, "o", rows[0])
        d.q_bs, d.k_bs, d.v_bs, d.o_bs = (lay.bs[x] for x in "qkvo")
        d.ldq, d.ldk, d.ldv, d.ldo = (lay.ld[x] for x in "qkvo")
        d.B, d.heads, d.head_dim, d.Nq, d.Nk = b[1] - b[0], h[1] - h[0], lay.D, rows[1] - rows[0], lay.Nk
        d.scale, d.residual_q, d.dtype = self.o["scale"], int(residual), U.pv_dtype(out)
        call("pv_attention", d)
        res = out.cpu()
        self.last, self.keep = d, [out]      # routed() launches the descriptor once more: its buffers stay allocated
        return res

    def routed(self):
        k = _routed_kernel(L.OP_ATTENTION, self.last)
        assert k == U.ATTN_ROUTES[self.cfg][0], (k, self.cfg)
        return k

    def expect(self, residual, mode, bound=None, log2_scale=None, **sub):
        o = self.o
        ls = U.attn_log2_scale(o["scale"]) if log2_scale is None else log2_scale
        want, dom = _reference(self, ls, residual)
        return U.AttnExpect(want, dom, self.lay, U.ATTN_ROUTES[self.cfg][0], mode, bound, **sub)


def _reference(k, ls, residual):
    """one float64 reference per case, shared by its launches (the residual is added to a copy)"""
    if not hasattr(k, "_ref"):
        k._ref = U.ref_attention(k.o["q"], k.o["k"], k.o["v"], ls, False)
    want, dom = k._ref
    return (want + k.o["q"] if residual else want), dom


def _float_scale(o):
    """normal operands: the exact product of the fp32 scale and log2 e, in float64 (the kernel's one fp32 rounding of it is part
    of what is measured)"""
    return float(torch.tensor(o["scale"], dtype=F32)) * 1.4426950408889634


def _bh(Nk, KT):
    return (2, 3) if Nk <= KT + 1 else (1, 2)


# ------------------------------------------------------------------ A
A_CASES = [(cfg, i) for cfg in CFGS for i in range(len(U.ATTN_TILES))]


@pytest.mark.parametrize("cfg,i", A_CASES, ids=["%s_nk%d" % (CFG_IDS[CFGS.index(c)], U.ATTN_NK[U.attn_kt(c[0])][i]) for c, i in A_CASES])
def test_a_selection_returns_the_selected_row_of_v(cfg, i):
    dtype, D = cfg
    KT = U.attn_kt(dtype)
    Nk = U.ATTN_NK[KT][i]
    assert U.cdiv(Nk, KT) == U.ATTN_TILES[i]
    B, H = _bh(Nk, KT)
    o = U.make_attn_select(B, H, D, U.attn_select_nq(Nk), Nk)
    gap = U.attn_select_conditions(o)
    k = _Attn(o, cfg)
    for residual in (False, True):
        what = "A selection %s D %d Nk %d%s" % (CFG_IDS[CFGS.index(cfg)], D, Nk, " + q" if residual else "")
        got = k.run(residual)
        if not residual:
            k.routed()
        e = k.expect(residual, "bits") if dtype == BF16 else k.expect(residual, "elem", 2.0 ** -21)
        sel_v = torch.stack([torch.stack([o["v"][b, o["sel"][b, h], h] for h in range(H)], 1) for b in range(B)])
        assert torch.equal(e.want.to(dtype), (sel_v + (o["q"] if residual else 0)).to(dtype))      # the reference IS the selected row
        err = e.check(got, what)
        print("%s: worst %.3e (gap %g)" % (what, err, gap))
        _rec(what, cfg, Nk, err, "0 (bits)" if dtype == BF16 else "2^-21 per element",
             "v[t(i)]%s: equal" % (" + q" if residual else "") if dtype == BF16 else "-")


# ------------------------------------------------------------------ B
def _b_nks(KT):
    return U.ATTN_NK[KT][-3], U.ATTN_NK[KT][-2]          # 7 full tiles; 8 tiles, the last ragged


B_NQ = 165


@functools.lru_cache(maxsize=None)
def _b_coverage(dtype, w64):
    KT = U.attn_kt(dtype)
    got = set()
    for Nk in _b_nks(KT):
        for sch in U.ATTN_B_SCHEDULES:
            o = U.make_attn_levels(sch, 1, 2, 32, B_NQ, Nk, KT)       # the levels do not depend on D beyond the seed
            got |= U.attn_mirror_coverage(U.attn_mirror(U.attn_level_args(o), KT, w64), Nk, KT)
    return got


@pytest.mark.parametrize("schedule", U.ATTN_B_SCHEDULES)
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_b_integer_score_levels_across_the_rescale_rule(cfg, schedule):
    dtype, D = cfg
    KT = U.attn_kt(dtype)
    w64 = U.ATTN_ROUTES[cfg][0] == "attn_w64_kernel"
    missing = U.ATTN_B_COVER - _b_coverage(dtype, w64)
    assert not missing, "the schedules of this route do not contain: %s" % sorted(missing)
    worst = 0.0
    for Nk in _b_nks(KT):
        o = U.make_attn_levels(schedule, 1, 2, D, B_NQ, Nk, KT)
        U.attn_level_args(o)
        k = _Attn(o, cfg)
        what = "B %s %s D %d Nk %d" % (schedule, CFG_IDS[CFGS.index(cfg)], D, Nk)
        got = k.run(False)
        k.routed()
        e = k.expect(False, "elem", U.attn_level_bound(dtype, Nk), log2_scale=0.125)
        vals = e.values(got).double()
        print("%s: worst %.3e of bound %.3e" % (what, ((vals - e.want).abs() / e.want.abs()).max().item(), e.bound))
        worst = max(worst, e.check(got, what) / e.bound)
    _rec("B %s %s D %d" % (schedule, CFG_IDS[CFGS.index(cfg)], D), cfg, _b_nks(KT), worst,
         "1 = 2^-7 |want| (one bf16 ulp)" if dtype == BF16 else "1 = 2 (Nk + 8) 2^-24 |want|")


# ------------------------------------------------------------------ C
C_CASES = [(cfg, var, j) for cfg in CFGS for var in U.ATTN_C_VARIANCES for j in range(3)]


@pytest.mark.parametrize("cfg,variance,j", C_CASES, ids=["%s_var%d_nk%d" % (CFG_IDS[CFGS.index(c)], v, U.ATTN_C_NK[U.attn_kt(c[0])][j])
                                                         for c, v, j in C_CASES])
def test_c_normal_operands_judged_per_query_row(cfg, variance, j):
    dtype, D = cfg
    Nk = U.ATTN_C_NK[U.attn_kt(dtype)][j]
    o = U.make_attn_float(1, 2, D, U.ATTN_C_NQ, Nk, variance, dtype)
    k = _Attn(o, cfg)
    what = "C variance %d %s D %d Nk %d" % (variance, CFG_IDS[CFGS.index(cfg)], D, Nk)
    got = k.run(False)
    k.routed()
    e = k.expect(False, "row", U.TOL[dtype], log2_scale=_float_scale(o))
    vals = e.values(got).double()
    print("%s: worst row %.3e" % (what, ((vals - e.want).abs().amax(-1) / e.want.abs().amax(-1)).max().item()))
    err = e.check(got, what)
    _rec(what, cfg, Nk, err, "%.0e per query row" % U.TOL[dtype])


# ------------------------------------------------------------------ D
def _d_check(k, residual, what, family):
    got = k.run(residual)
    if family == "A":
        e = k.expect(residual, "bits") if k.dtype == BF16 else k.expect(residual, "elem", 2.0 ** -21)
    else:
        e = k.expect(residual, "row", U.TOL[k.dtype], log2_scale=_float_scale(k.o))
    return e.check(got, what)


@pytest.mark.parametrize("kind", ["wide", "fused"])
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_d_strides_slices_and_gaps_with_nan_behind_every_operand(cfg, kind):
    dtype, D = cfg
    KT = U.attn_kt(dtype)
    NkA, NkC = U.ATTN_NK[KT][4], U.ATTN_C_NK[KT][1]
    oa = U.make_attn_select(2, 3, D, U.attn_select_nq(NkA), NkA)
    U.attn_select_conditions(oa)
    oc = U.make_attn_float(2, 3, D, U.ATTN_C_NQ, NkC, 4, dtype)
    errs = []
    for fam, o, Nk in (("A", oa, NkA), ("C", oc, NkC)):
        k = _Attn(o, cfg, kind)
        ld, bs = k.lay.ld, k.lay.bs
        assert min(ld.values()) > 3 * D and (kind == "fused" or len(set(ld.values())) == 4)
        assert all(bs[x] > (k.lay.Nq if x in "qo" else Nk) * ld[x] for x in "qkvo")
        for residual in (False, True):
            errs.append(_d_check(k, residual, "D %s %s %s D %d Nk %d res %d" % (kind, fam, CFG_IDS[CFGS.index(cfg)], D, Nk, residual), fam))
        k.routed()
    _rec("D %s layout, A and C, with and without q %s D %d" % (kind, CFG_IDS[CFGS.index(cfg)], D), cfg, (NkA, NkC), max(errs),
         "A: %s; C: %.0e per row" % ("0 (bits)" if dtype == BF16 else "2^-21", U.TOL[dtype]), "NaN gaps, O canaries: clean")


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_d_fewer_keys_than_a_staging_group(cfg):
    """Nk = 1 .. 4: the V staging groups 4 keys; every key past Nk is NaN in memory (wide layout, guard rows)."""
    dtype, D = cfg
    errs = []
    for Nk in (1, 2, 3, 4):
        oa = U.make_attn_select(1, 2, D, U.attn_select_nq(Nk), Nk)
        U.attn_select_conditions(oa)
        oc = U.make_attn_float(1, 2, D, 70, Nk, 1, dtype)
        for fam, o in (("A", oa), ("C", oc)):
            k = _Attn(o, cfg, "wide")
            errs.append(_d_check(k, fam == "C", "D Nk %d %s %s D %d" % (Nk, fam, CFG_IDS[CFGS.index(cfg)], D), fam))
            k.routed()
    _rec("D Nk = 1 .. 4, A and C, wide layout %s D %d" % (CFG_IDS[CFGS.index(cfg)], D), cfg, (1, 2, 3, 4), max(errs),
         "A: %s; C: %.0e per row" % ("0 (bits)" if dtype == BF16 else "2^-21", U.TOL[dtype]), "NaN gaps, O canaries: clean")


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_d_query_counts_around_a_wave_and_a_workgroup(cfg):
    dtype, D = cfg
    Nk = U.ATTN_C_NK[U.attn_kt(dtype)][0]
    errs = []
    for Nq in (1, 31, 32, 33, 127, 128, 129):
        k = _Attn(U.make_attn_float(1, 2, D, Nq, Nk, 4, dtype), cfg, "wide")
        errs.append(_d_check(k, True, "D Nq %d %s D %d" % (Nq, CFG_IDS[CFGS.index(cfg)], D), "C"))
        k.routed()
    _rec("D Nq = 1, 31, 32, 33, 127, 128, 129, wide layout %s D %d" % (CFG_IDS[CFGS.index(cfg)], D), cfg, Nk, max(errs),
         "%.0e per row" % U.TOL[dtype], "NaN gaps, O canaries: clean")


D_TOTALS = {1: (1, 1, 100), 7: (1, 7, 100), 9: (3, 3, 100), 17: (1, 1, 16 * 128 + 1)}        # total -> (B, heads, Nq)


@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_d_work_item_counts_on_both_sides_of_the_xcd_remainder(cfg):
    dtype, D = cfg
    Nk = U.ATTN_C_NK[U.attn_kt(dtype)][0]
    errs = []
    for total, (B, H, Nq) in D_TOTALS.items():
        assert B * H * U.cdiv(Nq, U.ATTN_WG_ROWS) == total
        k = _Attn(U.make_attn_float(B, H, D, Nq, Nk, 4, dtype), cfg)
        errs.append(_d_check(k, False, "D total %d %s D %d" % (total, CFG_IDS[CFGS.index(cfg)], D), "C"))
        k.routed()
    _rec("D B heads nqb = 1, 7, 9, 17 %s D %d" % (CFG_IDS[CFGS.index(cfg)], D), cfg, Nk, max(errs), "%.0e per row" % U.TOL[dtype])


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("cfg", CFGS, ids=CFG_IDS)
def test_e_a_rows_bits_do_not_depend_on_where_it_is_launched(cfg):
    """Sub-ranges keep every wave's composition (whole query blocks, whole heads, whole items): __any makes a lane's rescale points
    depend on the other 31 rows of its wave, and the kernels fill the lanes past Nq differently."""
    dtype, D = cfg
    B, H, Nq = 2, 3, 2 * U.ATTN_WG_ROWS + 37
    Nk = U.ATTN_C_NK[U.attn_kt(dtype)][1]
    o = U.make_attn_float(B, H, D, Nq, Nk, 12, dtype)
    k = _Attn(o, cfg, "wide")
    full = k.run(True)
    k.routed()
    err = k.expect(True, "row", U.TOL[dtype], log2_scale=_float_scale(o)).check(full, "E full launch")
    subs = [dict(rows=r) for r in ((0, 128), (128, 256), (256, Nq), (128, Nq))]
    subs += [dict(h=(h, h + 1)) for h in range(H)] + [dict(b=(b, b + 1)) for b in range(B)] + [dict(b=(1, 2), h=(2, 3), rows=(128, Nq))]
    for sub in subs:
        what = "E %s D %d sub-launch %s" % (CFG_IDS[CFGS.index(cfg)], D, sub)
        part = k.run(True, **sub)
        e = k.expect(True, "row", U.TOL[dtype], log2_scale=_float_scale(o), **sub)
        e.check(part, what)                  # the reference and the canaries around the sub-range
        e.same_bits(full, part, what)
    _rec("E %d sub-launches (query blocks, heads, items) %s D %d" % (len(subs), CFG_IDS[CFGS.index(cfg)], D), cfg, Nk, err,
         "%.0e per row" % U.TOL[dtype], "full launch: equal x %d" % len(subs))
