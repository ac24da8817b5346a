"""Direct parity of the two kernels of csrc/pv_mlp.hip on the MI355X, through the C ABI: mlp_rows16_kernel (pv_mlp_rows) and
ln_linear_rows_kernel (pv_ln_linear_rows), with the routed symbol asserted for every case.

What is delicate in them is hand-scheduled: a three-buffer LDS ring fed by LDS-DMA from inline asm, counted s_waitcnt vmcnt(N)
waits that depend on which wave issues the bias piece and on whether a wave stores at all, a fragment ring in registers, phase B
one hidden block behind phase A, a host-packed weight image with a permuted K order.  tests/test_gpu_kernels.py launches both at
the MViT-B shapes against fp32 torch under max|got - want| / max|want|; in LayerNorm mode want carries the residual stream
(abs-max 14-16) and the MLP branch (abs-max 3-4) is a fifth of the bound's room: b1 of the last hidden block may be missing.

Metric here: MlpExpect (gpu_util) subtracts the base (residual + b2; LayerNorm mode: x + b2) and measures the BRANCH against the
float64 reference's branch, relative to the branch's abs-max, under the project's bf16 bound 1e-2 (gpu_util.BRANCH_TOL).  The
reference alone costs at most a third of that (an fp32 replay with the kernel's rounding points, tests/test_mlp_kernel_checks.py),
and b1 of the last hidden block missing exceeds it at every A2 shape (same file).  A failure names row, workgroup, wave, lane row
and channel, and in the integer cases the hidden unit or block whose columns of W2 explain the row's error.

A  pv_mlp_rows -> mlp_rows16_kernel<KS2, NOB16, LN, ACT>; (C, Cout) -> <KS2, NOB16> is gpu_util.MLP_FORMS, ACT is GELU or -1 (the
   activation read from the descriptor at run time)
  A1 integer operands, ZERO tolerance: every pre-activation a multiple of 16 (pv_gelu_fast2 is exact at 0 and from 16 on), every
     value exact in its format, every sum below 2^24 (gpu_util.mlp_int_conditions, asserted before the launch).  LayerNorm mode:
     gamma = 0, beta an integer per channel, x an integer row per token (the residual).  5 pairs in operand mode + 3 in LayerNorm
     mode, each at H = 32, 64, 96, 160, 224 (1, 2, 3, 5, 7 hidden blocks) with GELU, NONE and RELU; M = 273
  A2 seeded normal operands under the branch metric: gpu_util.MLP_A2
  A3 LayerNorm edges at C = 96, 384: a constant row, a row of variance 1e-6 (at ln_eps 1e-6 and 1e-5), an outlier of 1e3 in the
     first / the last channel
  A4 ldx, ldr, ldy = row + 8 with NaN behind the input rows and canaries behind the output rows; b2 NULL; b1 None in the packer;
     the image's two trailing padding blocks filled with 0x7f bytes (3.4e38 as bf16 and as fp32): same bits as with zeros
  A5 yn (the next block's norm1) with GELU and with the runtime activation, ldyn = Cout + 8: y bit-equal to the launch without yn,
     |yn - LN64(the kernel's own y)| <= 2^-8 |want| + Cout 2^-23 max|want| (one bf16 rounding; the fp32 sum for elements near zero)
  A6 rows [1, M), [129, M), [272, M) launched alone through offset pointers: every row's y and yn bit-equal to the full launch
B  pv_ln_linear_rows -> ln_linear_rows_kernel<KS, MINW>; C -> <KS, MINW> is gpu_util.LNL_FORMS
  B1 gamma = 0, integer beta, W in {-1, 0, 1}, integer bias: bit-equal; C = 96, 192, 384, 768 x N = 32, 64, 96, 160
  B2 W one-hot under a permutation, gamma = 1, beta = 0: y[m][n] is the normalised channel sigma(n);
     |got - bf16(xn64)| <= 2^-7 |want| + C 2^-23 max|want| (one bf16 ulp: a rounding boundary can be crossed); the edge rows of A3,
     the outlier in channel 0 being the kernel's shift of its one-pass statistics
  B3 random weights, 1e-2 of the abs-max, every activation at C = 96 and 384
  B4 M = 1, 31, 33, 97, 128, 129, 161, 193 at N = 96: both store-counting terms of `allow` live; integer operands, bit-equal
  B5 ldx = C + 4, ldy = N + 8;  B6 rows [1, M) and [129, M) alone, and a second launch: same bits

PV_PARITY_RECORD=path leaves the table of the run there (profiles/r33/mlp_kernel_parity.md)."""
import ctypes as C
import os
import time

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U
from gpu_util import call, _routed_kernel

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
ACT_NAME = {L.ACT_NONE: "NONE", L.ACT_RELU: "RELU", L.ACT_SWISH: "SWISH", L.ACT_GELU: "GELU", L.ACT_SIGMOID: "SIGMOID"}
_REC, _FORMS = [], set()


@pytest.fixture(scope="module", autouse=True)
def _record():
    t0 = time.perf_counter()
    yield
    path = os.environ.get("PV_PARITY_RECORD")
    if not path:
        return
    with open(path, "w") as f:
        f.write("| case | routed kernel | instantiation | M | worst error | bound | bit checks |\n|---|---|---|---|---|---|---|\n")
        for r in _REC:
            f.write("| %s | `%s` | `<%s>` | %d | %s | %s | %s |\n" % (r["case"], r["kernel"], r["form"], r["M"], r["err"], r["bound"], r["bits"]))
        f.write("\ninstantiations launched (%d):\n" % len(_FORMS))
        for k in sorted(_FORMS):
            f.write("- `%s`\n" % k)
        f.write("\nwhole module: %.1f s\n" % (time.perf_counter() - t0))


def _rec(case, kernel, form, M, err=None, bound=None, bits="-"):
    _FORMS.add("%s<%s>" % (kernel, form))
    _REC.append(dict(case=case, kernel=kernel, form=form, M=M, err="-" if err is None else "%.2e" % err, bound=bound or "-", bits=bits))


def _ptr(t, elems=0):
    return t.data_ptr() + elems * t.element_size()


def _rows_dev(data, ld, dtype):
    """(M, C) values -> (M, ld) device rows; NaN behind every row: a kernel that reads past the row poisons its result"""
    buf = torch.full((data.shape[0], ld), float("nan"), dtype=dtype)
    buf[:, :data.shape[1]] = data.to(dtype)
    return buf.cuda()


def _out(M, ld, dtype):
    return torch.full((M + U.MLP_EXTRA_ROWS, ld), U.CANARY, dtype=dtype)


class _Mlp:
    """The operands of one pv_mlp_rows case on the device; run() launches rows [r0, M) into fresh canary buffers."""

    def __init__(self, o, wide=False, img=None):
        from pytorchvideo_amd.accelerator.mi355x.emit_mvit import pack_mlp_weights
        self.o, self.M = o, o["M"]
        pad = 8 if wide else 0
        self.ldx, self.ldr, self.ldy, self.ldyn = o["C"] + pad, o["Cout"] + pad, o["Cout"] + pad, o["Cout"] + 8
        self.x = _rows_dev(o["x"], self.ldx, F32 if o["ln"] else BF16)
        self.res = _rows_dev(o["res"], self.ldr, F32) if o["res"] is not None else None
        self.img = (pack_mlp_weights(o["w1"], o["b1"], o["w2"]) if img is None else img).cuda()
        dev = lambda t: None if t is None else t.float().cuda()
        self.b2, self.gamma, self.beta, self.ng, self.nb = (dev(o[k]) for k in ("b2", "gamma", "beta", "nn_gamma", "nn_beta"))
        self.form = "%d, %d, %s" % (*U.MLP_FORMS[(o["C"], o["Cout"])], "true" if o["ln"] else "false")

    def run(self, act, r0=0, yn=False):
        o, n = self.o, self.M - r0
        y = _out(self.M, self.ldy, F32).cuda()
        d = L.MlpDesc()
        d.x, d.w12, d.y = _ptr(self.x, r0 * self.ldx), self.img.data_ptr(), _ptr(y, r0 * self.ldy)
        d.b2 = self.b2.data_ptr() if self.b2 is not None else None
        d.residual = _ptr(self.res, r0 * self.ldr) if self.res is not None else None
        if o["ln"]:
            d.ln_gamma, d.ln_beta, d.ln_eps = self.gamma.data_ptr(), self.beta.data_ptr(), o["eps"]
        d.M, d.C, d.H, d.Cout, d.ldx, d.ldr, d.ldy, d.act, d.dtype = n, o["C"], o["H"], o["Cout"], self.ldx, self.ldr, self.ldy, act, L.PV_BF16
        ynb = None
        if yn:
            ynb = _out(self.M, self.ldyn, BF16).cuda()
            d.yn, d.nn_gamma, d.nn_beta, d.ldyn, d.nn_eps = _ptr(ynb, r0 * self.ldyn), self.ng.data_ptr(), self.nb.data_ptr(), self.ldyn, 1e-6
        assert L.lib().pv_mlp_rows_supported(C.byref(d)) == 1
        call("pv_mlp_rows", d)
        self.last, self.keep = d, (y, ynb)        # routed() launches the descriptor once more: its buffers stay allocated
        return y.cpu(), (ynb.cpu() if yn else None)

    def routed(self):
        k = _routed_kernel(L.OP_MLP_ROWS, self.last)
        assert k == "mlp_rows16_kernel"
        return k

    def expect(self, act, r0=0, tol=U.BRANCH_TOL, **kw):
        base, branch = U.ref_mlp_rows(self.o, act)
        return U.MlpExpect(base, branch, _out(self.M, self.ldy, F32), self.ldy, self.M, r0=r0, tol=tol, **kw)

    def expect_yn(self, y, r0=0):
        """norm1 of the next block against float64 LayerNorm of the kernel's OWN y"""
        Cout = self.o["Cout"]
        want = torch.zeros(self.M, Cout, dtype=torch.float64)
        want[r0:] = U.ref_ln64(y[r0:self.M, :Cout], self.o["nn_gamma"], self.o["nn_beta"], 1e-6)
        return U.MlpExpect(None, want, _out(self.M, self.ldyn, BF16), self.ldyn, self.M, r0=r0,
                           per_elem=(2.0 ** -8, Cout * 2.0 ** -23))

    def act_form(self, act):
        return "%s, %s" % (self.form, "PV_ACT_GELU" if act == L.ACT_GELU else "-1")


A1_CASES = [(c, co, ln, h) for ln in (False, True) for (c, co) in (U.MLP_LN_PAIRS if ln else U.MLP_FORMS) for h in U.MLP_A1_H]


@pytest.mark.parametrize("Cin,Cout,ln,H", A1_CASES, ids=["%s_%d_%d_h%d" % ("ln" if c[2] else "op", c[0], c[1], c[3]) for c in A1_CASES])
def test_a1_integer_operands_come_back_bit_exact(Cin, Cout, ln, H):
    """A1: weight, b1, b2 and residual routing of every instantiation at zero tolerance; M = 273 is two full workgroups, then one
    with wave 0 full, wave 1 holding one row and waves 2-7 empty."""
    o = U.make_mlp_int(Cin, H, Cout, ln, U.MLP_A1_M)
    U.mlp_int_conditions(o, U.MLP_A1_ACTS)
    assert U.row_layout(U.MLP_A1_M, U.MLP_WAVE_ROWS) == (3, [16, 1, 0, 0, 0, 0, 0, 0])
    k = _Mlp(o)
    for act in U.MLP_A1_ACTS:
        what = "A1 %s %d -> %d -> %d act %s" % ("LayerNorm" if ln else "operand", Cin, H, Cout, ACT_NAME[act])
        y, _ = k.run(act)
        kernel = k.routed()
        err = k.expect(act, tol=None, w2=o["w2"]).check(y, what)
        assert err == 0.0
        _rec(what, kernel, k.act_form(act), o["M"], err, "0 (bits)", "reference: equal")


@pytest.mark.parametrize("case", sorted(U.MLP_A2))
def test_a2_normal_operands_under_the_branch_metric(case):
    Cin, H, Cout, ln, res, act, M = U.MLP_A2[case]
    k = _Mlp(U.make_mlp_float(Cin, H, Cout, ln, res, M))
    y, _ = k.run(act)
    kernel = k.routed()
    e = k.expect(act)
    err = e.check(y, "A2 " + case)
    print("A2 %s: branch error %.3e of its abs-max (bound %.0e)" % (case, err, U.BRANCH_TOL))
    y2, _ = k.run(act)
    e.same_bits(y, y2, "A2 %s, second launch" % case)
    _rec("A2 %s (%d -> %d -> %d, %s)" % (case, Cin, H, Cout, ACT_NAME[act]), kernel, k.act_form(act), M, err, "%.0e" % U.BRANCH_TOL,
         "second launch: equal")


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("Cin", [96, 384])
def test_a3_layernorm_edge_rows(Cin, eps):
    """A3: variance 0, variance about ln_eps, an outlier in the first and in the last channel.  The two ln_eps values expect
    different branches on the variance-eps row (asserted), so an eps that is not read from the descriptor shows."""
    o = U.make_mlp_edges(Cin, 96, eps)
    k = _Mlp(o)
    e = k.expect(L.ACT_GELU)
    other = U.ref_mlp_rows(o, L.ACT_GELU, eps=1e-5 if eps == 1e-6 else 1e-6)[1]
    m = [r for r, kind in U.MLP_A3_ROWS.items() if kind == "variance_eps"][0]
    assert (other[m] - e.branch[m]).abs().max() > 3 * U.BRANCH_TOL * e.branch.abs().max()
    y, _ = k.run(L.ACT_GELU)
    kernel = k.routed()
    err = e.check(y, "A3 C %d eps %g" % (Cin, eps))
    print("A3 C %d eps %g: branch error %.3e" % (Cin, eps, err))
    _rec("A3 edges C %d ln_eps %g" % (Cin, eps), kernel, k.act_form(L.ACT_GELU), o["M"], err, "%.0e" % U.BRANCH_TOL)


@pytest.mark.parametrize("case,M", [("op_96_192", 129), ("ln_192", 130), ("op_384_384", 17)])
def test_a4_wide_strides_with_canaries(case, M):
    Cin, H, Cout, ln, res, act, _ = U.MLP_A2[case]
    k = _Mlp(U.make_mlp_float(Cin, H, Cout, ln, True, M), wide=True)
    assert k.ldx == Cin + 8 and k.ldy == Cout + 8 and (ln or k.ldr == Cout + 8)
    y, _ = k.run(act)
    kernel = k.routed()
    err = k.expect(act).check(y, "A4 strides " + case)
    _rec("A4 ldx, ldr, ldy + 8: " + case, kernel, k.act_form(act), M, err, "%.0e" % U.BRANCH_TOL, "pad columns, rows >= M: intact")


@pytest.mark.parametrize("res", [False, True])
def test_a4_operand_mode_without_b2(res):
    o = U.make_mlp_float(96, 96, 192, False, res, 130)
    o["b2"] = None
    k = _Mlp(o)
    y, _ = k.run(L.ACT_GELU)
    kernel = k.routed()
    err = k.expect(L.ACT_GELU).check(y, "A4 b2 NULL, residual %s" % res)
    _rec("A4 b2 NULL, residual %s" % res, kernel, k.act_form(L.ACT_GELU), o["M"], err, "%.0e" % U.BRANCH_TOL)


def test_a4_packer_without_b1():
    o = U.make_mlp_float(192, 64, 192, True, False, 130)
    o["b1"] = None
    k = _Mlp(o)
    y, _ = k.run(L.ACT_GELU)
    kernel = k.routed()
    err = k.expect(L.ACT_GELU).check(y, "A4 b1 None")
    _rec("A4 pack_mlp_weights(b1=None)", kernel, k.act_form(L.ACT_GELU), o["M"], err, "%.0e" % U.BRANCH_TOL)


@pytest.mark.parametrize("case", ["op_96_96", "ln_384"])
def test_a4_padding_blocks_may_hold_anything_finite(case):
    """The image ends in two blocks that are prefetched and never used; the header allows any finite values there."""
    from pytorchvideo_amd.accelerator.mi355x.emit_mvit import pack_mlp_weights
    Cin, H, Cout, ln, res, act, _ = U.MLP_A2[case]
    o = U.make_mlp_float(Cin, H, Cout, ln, res, 130)
    img = pack_mlp_weights(o["w1"], o["b1"], o["w2"])
    stage = Cin // 16 * 1024 + Cout // 32 * 2048 + 256
    assert img.numel() == (H // 32 + 3) * stage and not img[-2 * stage:].any()
    dirty = img.clone()
    dirty[-2 * stage:] = 0x7f
    assert torch.isfinite(dirty[-2 * stage:].view(BF16)).all() and torch.isfinite(dirty[-2 * stage:].view(F32)).all()
    assert dirty[-2 * stage:].view(BF16).float().min() > 3e38
    clean, k = _Mlp(o), _Mlp(o, img=dirty)
    y0, _ = clean.run(act)
    y1, _ = k.run(act)
    kernel = k.routed()
    e = k.expect(act)
    err = e.check(y1, "A4 dirty padding " + case)
    e.same_bits(y0, y1, "A4 %s: zero padding against 0x7f padding" % case)
    _rec("A4 padding blocks of 0x7f bytes: " + case, kernel, k.act_form(act), o["M"], err, "%.0e" % U.BRANCH_TOL, "zero padding: equal")


@pytest.mark.parametrize("case,act", [("op_96_192", L.ACT_GELU), ("op_96_192", L.ACT_SWISH), ("ln_192", L.ACT_GELU),
                                      ("ln_192", L.ACT_RELU)])
def test_a5_norm1_of_the_next_block(case, act):
    Cin, H, Cout, ln, res, _, M = U.MLP_A2[case]
    assert M == 273
    k = _Mlp(U.make_mlp_float(Cin, H, Cout, ln, res, M))
    y0, _ = k.run(act)
    y, yn = k.run(act, yn=True)
    kernel = k.routed()
    e = k.expect(act)
    err = e.check(y, "A5 " + case)
    e.same_bits(y0, y, "A5 %s: y without and with yn" % case)
    assert k.ldyn == Cout + 8
    k.expect_yn(y).check(yn, "A5 %s act %s: yn" % (case, ACT_NAME[act]))
    _rec("A5 yn: %s act %s" % (case, ACT_NAME[act]), kernel, k.act_form(act), M, err, "%.0e" % U.BRANCH_TOL,
         "y without yn: equal; yn within one bf16 rounding")


@pytest.mark.parametrize("case", ["op_96_192", "ln_384"])
def test_a6_a_row_does_not_depend_on_its_lane_wave_workgroup_or_m(case):
    """A6: rows [r0, M) launched alone through offset pointers.  From row 1 every row sits in another lane and the boundary rows
    in another wave; from 129 and 272 in another workgroup.  y and yn are bit-equal to the full launch."""
    Cin, H, Cout, ln, res, act, M = U.MLP_A2[case]
    assert M == 273
    k = _Mlp(U.make_mlp_float(Cin, H, Cout, ln, res, M))
    y, yn = k.run(act, yn=True)
    kernel = k.routed()
    e = k.expect(act)
    err = e.check(y, "A6 " + case)
    y2, yn2 = k.run(act, yn=True)
    e.same_bits(y, y2, "A6 %s: second launch, y" % case)
    k.expect_yn(y).same_bits(yn, yn2, "A6 %s: second launch, yn" % case)
    for r0 in U.MLP_RANGES:
        ys, yns = k.run(act, r0=r0, yn=True)
        es = k.expect(act, r0=r0)
        es.check(ys, "A6 %s rows [%d, %d)" % (case, r0, M))
        es.same_bits(ys, y, "A6 %s rows [%d, %d) alone against the full launch, y" % (case, r0, M), r0_b=0)
        eyn = k.expect_yn(ys, r0=r0)
        eyn.check(yns, "A6 %s rows [%d, %d): yn" % (case, r0, M))
        eyn.same_bits(yns, yn, "A6 %s rows [%d, %d) alone against the full launch, yn" % (case, r0, M), r0_b=0)
    _rec("A6 row ranges from %s: %s" % (", ".join(map(str, U.MLP_RANGES)), case), kernel, k.act_form(act), M, err, "%.0e" % U.BRANCH_TOL,
         "second launch: equal; %d sub-launches, y and yn: equal" % len(U.MLP_RANGES))


# ------------------------------------------------------------------ pv_ln_linear_rows
class _Lnl:
    def __init__(self, o, wide=False):
        from pytorchvideo_amd.accelerator.mi355x.emit_mvit import pack_ln_linear_weights
        self.o, self.M = o, o["M"]
        self.ldx, self.ldy = o["C"] + (4 if wide else 0), o["N"] + (8 if wide else 0)
        self.x = _rows_dev(o["x"], self.ldx, F32)
        self.img = pack_ln_linear_weights(o["w"], o["b"]).cuda()
        self.gamma, self.beta = o["gamma"].float().cuda(), o["beta"].float().cuda()
        self.form = "%d, %d" % U.LNL_FORMS[o["C"]]

    def run(self, act, r0=0):
        o = self.o
        y = _out(self.M, self.ldy, BF16).cuda()
        d = L.LnLinearDesc()
        d.x, d.wb, d.y = _ptr(self.x, r0 * self.ldx), self.img.data_ptr(), _ptr(y, r0 * self.ldy)
        d.ln_gamma, d.ln_beta, d.ln_eps = self.gamma.data_ptr(), self.beta.data_ptr(), o["eps"]
        d.M, d.C, d.N, d.ldx, d.ldy, d.act, d.dtype = self.M - r0, o["C"], o["N"], self.ldx, self.ldy, act, L.PV_BF16
        assert L.lib().pv_ln_linear_rows_supported(C.byref(d)) == 1
        call("pv_ln_linear_rows", d)
        self.last, self.keep = d, y               # routed() launches the descriptor once more: its buffer stays allocated
        return y.cpu()

    def routed(self):
        k = _routed_kernel(L.OP_LN_LINEAR, self.last)
        assert k == "ln_linear_rows_kernel"
        return k

    def expect(self, act, r0=0, **kw):
        return U.MlpExpect(None, U.ref_ln_linear(self.o, act), _out(self.M, self.ldy, BF16), self.ldy, self.M, r0=r0,
                           wave_rows=U.LNL_WAVE_ROWS, **kw)


@pytest.mark.parametrize("N", U.LNL_B1_N)
@pytest.mark.parametrize("Cin", sorted(U.LNL_FORMS))
def test_b1_integer_weight_bias_and_store_routing(Cin, N):
    o = U.make_lnl_int(Cin, N, 161)
    U.lnl_int_conditions(o)
    k = _Lnl(o)
    y = k.run(L.ACT_NONE)
    kernel = k.routed()
    assert k.expect(L.ACT_NONE).check(y, "B1 C %d N %d" % (Cin, N)) == 0.0
    _rec("B1 integers C %d N %d" % (Cin, N), kernel, k.form, o["M"], 0.0, "0 (bits)", "reference: equal")


@pytest.mark.parametrize("Cin", sorted(U.LNL_FORMS))
def test_b2_selection_matrix_shows_the_normalised_rows(Cin):
    o = U.make_lnl_select(Cin, 130)
    k = _Lnl(o)
    y = k.run(L.ACT_NONE)
    kernel = k.routed()
    e = k.expect(L.ACT_NONE, per_elem=(2.0 ** -7, Cin * 2.0 ** -23))
    assert torch.equal(e.branch, U.bf16_of(U.ref_ln64(o["x"], o["gamma"], o["beta"], o["eps"]))[:, o["sigma"]])
    err = e.check(y, "B2 C %d" % Cin)
    print("B2 C %d: worst error %.3e of the abs-max" % (Cin, err))
    _rec("B2 selection matrix C %d (edge rows %s)" % (Cin, sorted(o["edges"])), kernel, k.form, o["M"], err, "2^-7 |want| + C 2^-23 max|want|")


@pytest.mark.parametrize("act", U.LNL_ACTS, ids=[ACT_NAME[a] for a in U.LNL_ACTS])
@pytest.mark.parametrize("Cin", [96, 384])
def test_b3_random_weights_with_every_activation(Cin, act):
    k = _Lnl(U.make_lnl_float(Cin, 96, 161))
    y = k.run(act)
    kernel = k.routed()
    err = k.expect(act, tol=U.TOL[BF16]).check(y, "B3 C %d act %s" % (Cin, ACT_NAME[act]))
    print("B3 C %d act %s: error %.3e of the abs-max" % (Cin, ACT_NAME[act], err))
    _rec("B3 random C %d act %s" % (Cin, ACT_NAME[act]), kernel, k.form, 161, err, "%.0e" % U.TOL[BF16])


@pytest.mark.parametrize("M", U.LNL_B4_M)
@pytest.mark.parametrize("Cin", [96, 192])
def test_b4_wave_accounting(Cin, M):
    """B4: the counted wait of a block allows the DMA pieces of the next block and the stores of the two blocks before; the wave
    that issues the bias piece (wave KS & 3: wave 2 at C = 96, wave 0 at 192, 384, 768) counts one piece more, a wave without a row
    counts no stores.  N = 96 is three output blocks, so both store terms are live.  With 32 rows per wave, at C = 96: M = 129 and
    161 leave the bias wave (wave 2 of the second workgroup) without a row, M = 193 gives it one row; M = 1, 31 and 33 leave it
    without a row in the first workgroup, M = 97 and 128 fill it (97: wave 3 holds one row)."""
    assert {c: ks & 3 for c, (ks, _) in U.LNL_FORMS.items()} == {96: 2, 192: 0, 384: 0, 768: 0}
    bias_wave = U.LNL_FORMS[Cin][0] & 3
    held = U.row_layout(M, U.LNL_WAVE_ROWS)[1]
    if Cin == 96:
        assert (held[2] == 0) == (M in (1, 31, 33, 129, 161)) and (M != 193 or held[2] == 1)
    o = U.make_lnl_int(Cin, 96, M)
    U.lnl_int_conditions(o)
    k = _Lnl(o)
    y = k.run(L.ACT_NONE)
    kernel = k.routed()
    assert k.expect(L.ACT_NONE).check(y, "B4 C %d M %d" % (Cin, M)) == 0.0
    _rec("B4 C %d M %d: last workgroup holds %s, bias wave %d" % (Cin, M, held, bias_wave), kernel, k.form, M, 0.0, "0 (bits)", "reference: equal")


@pytest.mark.parametrize("Cin,N", [(96, 96), (384, 64), (768, 32)])
def test_b5_wide_strides_with_canaries(Cin, N):
    k = _Lnl(U.make_lnl_float(Cin, N, 130), wide=True)
    assert k.ldx == Cin + 4 and k.ldy == N + 8
    y = k.run(L.ACT_NONE)
    kernel = k.routed()
    err = k.expect(L.ACT_NONE, tol=U.TOL[BF16]).check(y, "B5 C %d" % Cin)
    _rec("B5 ldx + 4, ldy + 8: C %d N %d" % (Cin, N), kernel, k.form, 130, err, "%.0e" % U.TOL[BF16], "pad columns, rows >= M: intact")


@pytest.mark.parametrize("Cin", [96, 192])
def test_b6_row_ranges_and_a_second_launch_give_the_same_bits(Cin):
    M = 273
    k = _Lnl(U.make_lnl_float(Cin, 96, M))
    y = k.run(L.ACT_GELU)
    kernel = k.routed()
    e = k.expect(L.ACT_GELU, tol=U.TOL[BF16])
    err = e.check(y, "B6 C %d" % Cin)
    e.same_bits(y, k.run(L.ACT_GELU), "B6 C %d: second launch" % Cin)
    for r0 in U.LNL_RANGES:
        ys = k.run(L.ACT_GELU, r0=r0)
        es = k.expect(L.ACT_GELU, r0=r0, tol=U.TOL[BF16])
        es.check(ys, "B6 C %d rows [%d, %d)" % (Cin, r0, M))
        es.same_bits(ys, y, "B6 C %d rows [%d, %d) alone against the full launch" % (Cin, r0, M), r0_b=0)
    _rec("B6 row ranges from %s: C %d" % (", ".join(map(str, U.LNL_RANGES)), Cin), kernel, k.form, M, err, "%.0e" % U.TOL[BF16],
         "second launch: equal; %d sub-launches: equal" % len(U.LNL_RANGES))
