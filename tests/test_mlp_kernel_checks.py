"""The checks of tests/test_gpu_mlp_kernels.py can fail, and the claims its case tables make hold.  No GPU: the references, the
operands and gpu_util.MlpExpect are CPU code.

  - MlpExpect passes on its own float64 reference, and on an fp32 replay of mlp_rows16_kernel's arithmetic (its rounding points,
    the A&S erf of pv_gelu_fast2) with at least two thirds of the bound to spare, at every A2 shape: the bound is not spent on the
    reference.
  - b1 of the last hidden block missing passes the metric of tests/test_gpu_kernels.py at the MViT-B shape and exceeds the branch
    metric's bound at every A2 shape.
  - Each of these defects, applied to the reference, raises -- on normal operands under the bound, and on integer operands at zero
    tolerance with the hidden block or unit named: b1 of the last hidden block dropped; b1 shifted by one block; the last hidden
    block dropped; the first block's activations stale from the second; the two units of a packed pair swapped; one row copied from
    its neighbour; b2 missing; the residual of row m - 1; a touched pad column; a touched row >= M; one bf16 ulp in one yn element,
    which passes the tolerance and fails the bit check.
  - Every integer case of A1, B1 and B4 meets its exactness conditions; every M has the workgroup, wave and row layout the GPU
    tests say it has; H gives the hidden-block counts 1, 2, 3, 5, 7.
  - The launcher lines those shapes rest on are still in csrc/pv_mlp.hip."""
import os

import pytest
import torch
import torch.nn.functional as F

from pytorchvideo_amd import _lib as L
import gpu_util as U

F32, BF16 = torch.float32, torch.bfloat16
GELU = L.ACT_GELU
FLOAT_CASES = ["op_96_192", "ln_384"]                      # H = 96: three hidden blocks, M = 273
INT_CASES = [(96, 96, 192, False), (192, 160, 192, True)]  # (C, H, Cout, LayerNorm mode), M = 273


def _before(M, ld, dtype=F32):
    return torch.full((M + U.MLP_EXTRA_ROWS, ld), U.CANARY, dtype=dtype)


def _float_case(case):
    Cin, H, Cout, ln, res, act, M = U.MLP_A2[case]
    o = U.make_mlp_float(Cin, H, Cout, ln, res, M)
    base, branch = U.ref_mlp_rows(o, act)
    return o, act, U.MlpExpect(base, branch, _before(M, Cout + 8), Cout + 8, M, tol=U.BRANCH_TOL)


def _int_case(Cin, H, Cout, ln):
    o = U.make_mlp_int(Cin, H, Cout, ln, U.MLP_A1_M)
    base, branch = U.ref_mlp_rows(o, GELU)
    return o, GELU, U.MlpExpect(base, branch, _before(o["M"], Cout + 8), Cout + 8, o["M"], w2=o["w2"])


def _cases():
    return [("float", c) for c in FLOAT_CASES] + [("int", c) for c in INT_CASES]


def _make(kind, c):
    return _float_case(c) if kind == "float" else _int_case(*c)


@pytest.mark.parametrize("case", sorted(U.MLP_A2))
def test_the_checker_passes_on_the_reference_and_on_an_fp32_replay_with_margin(case):
    o, act, e = _float_case(case)
    assert e.check(e.ideal()) <= 2.0 ** -23 * (e.base + e.branch).abs().max() / e.branch.abs().max()    # the fp32 rounding of y
    buf = e.before.clone()
    buf[:o["M"], :o["Cout"]] = U.replay_mlp_rows(o, act)
    err = e.check(buf, "fp32 replay " + case)
    assert err <= U.BRANCH_TOL / 3, "the reference alone spends %.2e of the bound %.0e at %s" % (err, U.BRANCH_TOL, case)


@pytest.mark.parametrize("case", sorted(U.MLP_A2))
def test_b1_of_the_last_hidden_block_missing_exceeds_the_bound_at_every_a2_shape(case):
    o, act, e = _float_case(case)
    b1 = o["b1"].clone()
    b1[-32:] = 0
    bad = U.ref_mlp_rows(o, act, b1=b1)[1]
    assert (bad - e.branch).abs().max() > U.BRANCH_TOL * e.branch.abs().max()
    with pytest.raises(AssertionError, match="of the branch abs-max > 1.0e-02; worst at row"):
        e.check(e.ideal(branch=bad))


def test_the_same_defect_passes_the_sum_metric_at_the_mvit_b_shape():
    """tests/test_gpu_kernels.py::test_fused_mlp_rows at (130, 384, 1536, 384) in LayerNorm mode, its seed, its metric."""
    o = U.make_mlp_float(384, 1536, 384, True, False, 130, seed=77)
    base, branch = U.ref_mlp_rows(o, GELU)
    b1 = o["b1"].clone()
    b1[-32:] = 0
    bad = U.ref_mlp_rows(o, GELU, b1=b1)[1]
    assert U.rel_err(base + bad, base + branch) <= 1e-2                               # the residual stream hides it
    assert (bad - branch).abs().max() > U.BRANCH_TOL * branch.abs().max()             # the branch metric does not


def _hidden_defects(o):
    H = o["H"]
    b1_last = o["b1"].clone()
    b1_last[-32:] = 0

    def drop_last(h):
        h = h.clone()
        h[:, -32:] = 0
        return h

    def stale_first(h):
        h = h.clone()
        h[:, :32] = h[:, 32:64]
        return h

    def swap_pair(h):                      # units 36, 37: one packed bf16 pair of hidden block 1
        h = h.clone()
        h[:, [36, 37]] = h[:, [37, 36]]
        return h
    assert H >= 64
    return {
        "b1_last_dropped": (dict(b1=b1_last), None, "hidden block %d alone" % (H // 32 - 1)),
        "b1_shifted_a_block": (dict(b1=torch.roll(o["b1"], 32)), None, None),
        "last_block_dropped": ({}, drop_last, "hidden block %d alone" % (H // 32 - 1)),
        "first_block_stale": ({}, stale_first, "hidden block 0 alone"),
        "pair_swapped": ({}, swap_pair, "hidden block 1 alone"),
    }


@pytest.mark.parametrize("defect", ["b1_last_dropped", "b1_shifted_a_block", "last_block_dropped", "first_block_stale", "pair_swapped"])
@pytest.mark.parametrize("kind,c", _cases(), ids=lambda v: str(v).replace(" ", ""))
def test_a_defect_on_the_hidden_values_is_seen_and_localised(kind, c, defect):
    o, act, e = _make(kind, c)
    changed, edit, names = _hidden_defects(o)[defect]
    bad = U.ref_mlp_rows(o, act, edit_hidden=edit, **changed)[1]
    assert not torch.equal(bad, e.branch)
    with pytest.raises(AssertionError, match=r"worst at row \d+ \(workgroup \d, wave \d, lane row \d+ of the launch from row 0\), channel \d+") as info:
        e.check(e.ideal(branch=bad), defect)
    if kind == "int" and names:
        assert names in str(info.value), str(info.value)


def test_a_single_wrong_hidden_unit_is_named():
    o, act, e = _int_case(*INT_CASES[0])

    def one_unit(h):
        h = h.clone()
        h[200, 70] += 16
        return h
    bad = U.ref_mlp_rows(o, act, edit_hidden=one_unit)[1]
    with pytest.raises(AssertionError, match=r"worst at row 200 \(workgroup 1, wave 4, lane row 8 .*hidden unit 70 alone \(hidden block 2, unit 6 of it\) being off by 16"):
        e.check(e.ideal(branch=bad))


@pytest.mark.parametrize("kind,c", _cases(), ids=lambda v: str(v).replace(" ", ""))
def test_row_and_base_defects_are_seen_and_name_the_row(kind, c):
    o, act, e = _make(kind, c)
    M, W = o["M"], o["Cout"]
    m = 2 * U.WG_ROWS + 16                                               # the single row of wave 1 of the last workgroup
    assert U.row_place(m, U.MLP_WAVE_ROWS) == (2, 1, 0) and m == M - 1
    bad = e.ideal()
    bad[m, :W] = bad[m - 1, :W]                                          # one row copied from its neighbour
    with pytest.raises(AssertionError, match=r"1 rows .*worst at row %d \(workgroup 2, wave 1, lane row 0" % m):
        e.check(bad)
    with pytest.raises(AssertionError, match="worst at row"):            # b2 missing
        e.check(e.ideal(base=e.base - o["b2"].double()))
    shifted = e.base.clone()                                             # the residual (LayerNorm mode: x) of row m - 1
    shifted[m] = e.base[m - 1]
    with pytest.raises(AssertionError, match=r"worst at row %d " % m):
        e.check(e.ideal(base=shifted))


def test_a_touched_pad_column_and_a_touched_row_behind_m_are_seen():
    o, act, e = _float_case("op_96_192")
    M, W = o["M"], o["Cout"]
    bad = e.ideal()
    bad[5, W] = 0.0
    with pytest.raises(AssertionError, match=r"first at row 5, column %d \(a pad column\)" % W):
        e.check(bad)
    bad = e.ideal()
    bad[M, 3] = 1.0
    with pytest.raises(AssertionError, match=r"first at row %d, column 3 \(a row at or behind M = %d\)" % (M, M)):
        e.check(bad)
    sub = U.MlpExpect(e.base, e.branch, e.before, e.ld, M, r0=129, tol=U.BRANCH_TOL)
    sub.check(sub.ideal())
    bad = sub.ideal()
    bad[128, 0] = 1.0
    with pytest.raises(AssertionError, match="a row below the launch's first"):
        sub.check(bad)
    assert "row 129 (workgroup 0, wave 0, lane row 0 of the launch from row 129)" in sub.where(129, 0)


def test_one_bf16_ulp_in_one_yn_element_passes_the_tolerance_and_fails_the_bit_check():
    o, act, e = _float_case("op_96_192")
    M, W = o["M"], o["Cout"]
    y = e.ideal()[:M, :W]
    want = U.ref_ln64(y, o["nn_gamma"], o["nn_beta"], 1e-6)
    rel, floor = 2.0 ** -8, W * 2.0 ** -23
    eyn = U.MlpExpect(None, want, _before(M, W + 8, BF16), W + 8, M, per_elem=(rel, floor))
    good = eyn.ideal()
    eyn.check(good)
    # the bf16 neighbour on the other side of the float64 value is one ulp from the rounded one; it is within one rounding of
    # the float64 value where that lies near the middle of the two (and its magnitude near the top of the binade)
    g = good[:M, :W].double()
    ulp = 2.0 ** (torch.floor(torch.log2(g.abs())) - 7)
    other = g + torch.sign(want - g) * ulp
    ok = ((other - want).abs() <= 0.99 * (rel * want.abs() + floor * want.abs().max())) & (want.abs() > 1.0) & (g != want)
    assert ok.sum() > 10
    m, c = (int(v) for v in ok.nonzero()[5])
    bad = good.clone()
    bad[m, c] = other[m, c]
    assert bad[m, c].double() == other[m, c] and abs(int(bad[m, c:c + 1].view(torch.int16)) - int(good[m, c:c + 1].view(torch.int16))) == 1
    eyn.check(bad)
    with pytest.raises(AssertionError, match=r"1 elements of 1 rows differ; first at row %d, channel %d" % (m, c)):
        eyn.same_bits(good, bad)
    two = good.clone()
    two[m, c] = g[m, c] + torch.sign(want[m, c] - g[m, c]) * 2 * ulp[m, c]
    with pytest.raises(AssertionError, match="beyond"):
        eyn.check(two)
    eyn.same_bits(good, good.clone())


def test_the_bit_check_names_both_places_of_a_row():
    """a row range launched alone sits in other lanes, waves and workgroups: the message carries both places"""
    e = U.MlpExpect(None, torch.ones(273, 32, dtype=torch.float64), _before(273, 32, BF16), 32, 273)
    a, b = e.ideal(), e.ideal()
    b[128, 0] = 2.0
    with pytest.raises(AssertionError, match=r"first at row 128, channel 0: .*\(1, 0, 0\) against .* as \(0, 7, 15\)"):
        e.same_bits(a, b, r0_b=1)


# ------------------------------------------------------------------ the case tables
A1_CASES = [(c, co, ln, h) for ln in (False, True) for (c, co) in (U.MLP_LN_PAIRS if ln else U.MLP_FORMS) for h in U.MLP_A1_H]


def test_the_a1_table_is_the_one_the_issue_asks_for():
    assert sorted(U.MLP_FORMS) == [(96, 96), (96, 192), (192, 192), (192, 384), (384, 384)]
    assert sorted(U.MLP_LN_PAIRS) == [(96, 96), (192, 192), (384, 384)] and len(A1_CASES) == 40
    assert [h // 32 for h in U.MLP_A1_H] == [1, 2, 3, 5, 7]
    assert set(U.MLP_A1_ACTS) == {L.ACT_GELU, L.ACT_NONE, L.ACT_RELU}
    for (c, co), (ks2, nob16) in U.MLP_FORMS.items():
        assert (ks2, nob16) == (c // 32, co // 16)
    assert {c: ks for c, (ks, _) in U.LNL_FORMS.items()} == {c: c // 16 for c in (96, 192, 384, 768)}
    # 16 instantiations outside PV_DEV_ABLATION: 5 pairs x {GELU, -1} in operand mode, 3 x {GELU, -1} in LayerNorm mode
    assert len({(c, co, ln, a == GELU) for (c, co, ln, _) in A1_CASES for a in U.MLP_A1_ACTS}) == 16


@pytest.mark.parametrize("Cin,Cout,ln,H", A1_CASES)
def test_every_a1_case_is_exact(Cin, Cout, ln, H):
    o = U.make_mlp_int(Cin, H, Cout, ln, U.MLP_A1_M)
    assert U.mlp_int_conditions(o, U.MLP_A1_ACTS) < 2 ** 24
    if ln:
        assert len(set(o["beta"].tolist())) == min(Cin, 193) and (o["x"][0] != o["x"][1]).any()
        for gap in (8, 16, 32):
            assert (o["beta"][gap:] != o["beta"][:-gap]).all()
    base, branch = U.ref_mlp_rows(o, GELU)
    assert (branch % 16 == 0).all() and branch.abs().max() > 0
    assert torch.equal((base + branch).float().double(), base + branch)


def test_the_integer_conditions_can_fail():
    o = U.make_mlp_int(96, 64, 96, False, 20)
    o["b1"] = o["b1"] + 8.0                                            # pre-activations of 8 mod 16: GELU is not exact there
    with pytest.raises(AssertionError):
        U.mlp_int_conditions(o, [GELU])
    o = U.make_lnl_int(96, 64, 20)
    o["b"] = o["b"] + 300.0
    with pytest.raises(AssertionError):
        U.lnl_int_conditions(o)


def test_the_a2_table_covers_pairs_modes_activations_h_and_m():
    t = U.MLP_A2
    gelu = {(c, co, ln) for c, h, co, ln, res, act, m in t.values() if act == GELU}
    assert gelu == {(c, co, False) for c, co in U.MLP_FORMS} | {(c, co, True) for c, co in U.MLP_LN_PAIRS}
    assert {act for *_, act, m in t.values()} == {GELU, L.ACT_SWISH, L.ACT_SIGMOID}
    assert {h for _, h, *_ in t.values()} == {32, 96, 160}
    assert {m for *_, m in t.values()} == {1, 15, 17, 127, 128, 129, 273}
    assert all(m <= 273 and h <= 224 for _, h, *_, m in t.values())
    for case in FLOAT_CASES + ["ln_192"]:
        assert t[case][6] == 273


def test_every_m_has_the_layout_the_gpu_tests_say():
    lay = lambda M: U.row_layout(M, U.MLP_WAVE_ROWS)
    assert lay(273) == (3, [16, 1, 0, 0, 0, 0, 0, 0])
    assert lay(1) == (1, [1, 0, 0, 0, 0, 0, 0, 0]) and lay(15)[1][0] == 15 and lay(17)[1][:2] == [16, 1]
    assert lay(127) == (1, [16] * 7 + [15]) and lay(128) == (1, [16] * 8) and lay(129) == (2, [1] + [0] * 7)
    # A6: from row 1, row m sits one lane row lower and the rows 16 k in the wave before; from 129 and 272, in another workgroup
    assert U.row_place(16 - 1, 16) == (0, 0, 15) and U.row_place(16, 16) == (0, 1, 0)
    for r0 in U.MLP_RANGES:
        assert 0 < r0 < 273 and r0 % 8 != 0 or r0 == 272
    assert U.row_place(272, 16) == (2, 1, 0) and U.row_place(272 - 272, 16) == (0, 0, 0) and U.row_place(272 - 129, 16) == (1, 0, 15)
    lnl = lambda M: U.row_layout(M, U.LNL_WAVE_ROWS)[1]
    assert [lnl(M) for M in U.LNL_B4_M] == [[1, 0, 0, 0], [31, 0, 0, 0], [32, 1, 0, 0], [32, 32, 32, 1], [32] * 4, [1, 0, 0, 0],
                                             [32, 1, 0, 0], [32, 32, 1, 0]]
    assert {c: ks & 3 for c, (ks, _) in U.LNL_FORMS.items()} == {96: 2, 192: 0, 384: 0, 768: 0}      # the wave that issues the bias piece
    assert [n // 32 for n in U.LNL_B1_N] == [1, 2, 3, 5] and set(U.LNL_ACTS) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("Cin", [96, 384])
def test_the_a3_edge_rows_are_what_they_are_called(Cin):
    o6, o5 = U.make_mlp_edges(Cin, 96, 1e-6), U.make_mlp_edges(Cin, 96, 1e-5)
    assert torch.equal(o6["x"], o5["x"])
    rows = {kind: m for m, kind in U.MLP_A3_ROWS.items()}
    x = o6["x"].double()
    assert x[rows["constant"]].var(unbiased=False) == 0
    assert abs(x[rows["variance_eps"]].var(unbiased=False).item() / 1e-6 - 1) < 1e-3
    assert x[rows["outlier_first"]][0] == 1e3 and x[rows["outlier_last"]][-1] == 1e3 and x[rows["outlier_first"]][1:].abs().max() < 6
    assert len({U.row_place(m, 16)[1] for m in rows.values()}) == 2 and 0 in rows.values()          # two waves; row 0 stands in for absent rows
    b6, b5 = U.ref_mlp_rows(o6, GELU)[1], U.ref_mlp_rows(o5, GELU)[1]
    m = rows["variance_eps"]
    assert (b6[m] - b5[m]).abs().max() > 3 * U.BRANCH_TOL * b6.abs().max()        # a hard-coded eps shows
    others = [r for r in range(U.MLP_A3_M) if r != m and r != rows["constant"]]
    assert (b6[others] - b5[others]).abs().max() < U.BRANCH_TOL * b6.abs().max() / 3
    # variance 0: xn is beta, the branch comes from beta alone
    only_beta = U.ref_mlp_rows(o6, GELU, x=torch.zeros_like(o6["x"]))[1]
    assert torch.equal(b6[rows["constant"]], only_beta[rows["constant"]])


@pytest.mark.parametrize("Cin", sorted(U.LNL_FORMS))
def test_every_integer_ln_linear_case_is_exact_and_the_selection_selects(Cin):
    for N in U.LNL_B1_N:
        o = U.make_lnl_int(Cin, N, 161)
        assert 48 < U.lnl_int_conditions(o) <= 256                   # more than one term reaches the output
        for gap in (8, 16, 32):
            assert (o["beta"][gap:] != o["beta"][:-gap]).all()
    for M in U.LNL_B4_M:
        U.lnl_int_conditions(U.make_lnl_int(Cin, 96, M))
    o = U.make_lnl_select(Cin, 130)
    assert sorted(o["sigma"].tolist()) == list(range(Cin)) and (o["w"].sum(1) == 1).all() and (o["w"].sum(0) == 1).all()
    want = U.ref_ln_linear(o, L.ACT_NONE)
    assert torch.equal(want, U.bf16_of(U.ref_ln64(o["x"], o["gamma"], o["beta"], o["eps"]))[:, o["sigma"]])
    assert o["x"][0, 0] == 1e3 and set(o["edges"].values()) == set(U.MLP_A3_ROWS.values())
    e = U.MlpExpect(None, want, _before(130, Cin, BF16), Cin, 130, wave_rows=U.LNL_WAVE_ROWS, per_elem=(2.0 ** -7, Cin * 2.0 ** -23))
    e.check(e.ideal())
    bad = e.ideal()
    bad[:, [3, 4]] = bad[:, [4, 3]]                                    # two output channels swapped
    with pytest.raises(AssertionError, match=r"workgroup \d, wave \d, lane row \d+ of the launch from row 0\), channel [34]"):
        e.check(bad)


def test_the_references_agree_with_torch():
    o = U.make_mlp_float(96, 64, 192, False, True, 20)
    base, branch = U.ref_mlp_rows(o, GELU)
    want = o["b2"] + F.linear(F.gelu(F.linear(o["x"].float(), o["w1"], o["b1"])), o["w2"]) + o["res"]
    assert U.rel_err(base + branch, want) < 5e-3                        # torch keeps the hidden values in fp32
    o = U.make_mlp_float(96, 64, 96, True, False, 20)
    base, branch = U.ref_mlp_rows(o, GELU)
    xn = F.layer_norm(o["x"], (96,), o["gamma"], o["beta"], 1e-6)
    want = o["x"] + o["b2"] + F.linear(F.gelu(F.linear(xn, o["w1"], o["b1"])), o["w2"])
    assert U.rel_err(base + branch, want) < 5e-3
    o = U.make_lnl_float(96, 64, 20)
    want = F.linear(F.layer_norm(o["x"], (96,), o["gamma"], o["beta"], 1e-6), o["w"], o["b"])
    assert U.rel_err(U.ref_ln_linear(o, L.ACT_NONE), want) < 5e-3
    assert U.rel_err(U.ref_ln_linear(o, L.ACT_SWISH), F.silu(want)) < 5e-3
    x = U.randn((1000,), 9, 3.0)
    assert (U._gelu_as_f32(x) - F.gelu(x)).abs().max() < 1e-4           # A&S 7.1.25: |erf error| <= 2.5e-5
    big = torch.tensor([-48.0, -16.0, 0.0, 16.0, 32.0, 112.0])
    assert torch.equal(U._gelu_as_f32(big), big.clamp_min(0))           # exact at 0 and from |x| = 16 on


# ------------------------------------------------------------------ the launcher text the shapes rest on
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorchvideo_amd", "csrc")
PINNED = [
    "const long m = (long)blockIdx.x * 128 + wave * 16 + n16;",
    "const long m = (long)blockIdx.x * 128 + wave * 32 + l31;",
    "const unsigned grid = (unsigned)pv_ceil_div(d.M, 128);",
    "PV_LAUNCH((mlp_rows16_kernel<KS2, NOB16, true, ACTv>), dim3(grid), dim3(512), 0, s, d);",
    "PV_LAUNCH((mlp_rows16_kernel<KS2, NOB16, false, ACTv>), dim3(grid), dim3(512), 0, s, d);",
    "PV_LAUNCH((ln_linear_rows_kernel<KS, MINW>), dim3((unsigned)pv_ceil_div(d.M, 128)), dim3(256), 0, s, d);",
    "if (d.act == PV_ACT_GELU) PV16_GO(PV_ACT_GELU);",
    "else PV16_GO(-1);",
    "if (d.C == 96 && d.Cout == 96) return launch16<3, 6>(d, s);",
    "if (d.C == 96 && d.Cout == 192) return launch16<3, 12>(d, s);",
    "if (d.C == 192 && d.Cout == 192) return launch16<6, 12>(d, s);",
    "if (d.C == 192 && d.Cout == 384) return launch16<6, 24>(d, s);",
    "if (d.C == 384 && d.Cout == 384) return launch16<12, 24>(d, s);",
    "case 96: return launch_ln_linear<6, 2>(*dp, s);",
    "case 192: return launch_ln_linear<12, 2>(*dp, s);",
    "case 384: return launch_ln_linear<24, 2>(*dp, s);",
    "case 768: return launch_ln_linear<48, 1>(*dp, s);",
    "if (wave == (KS & 3))",
    "const int dma_next = (wave == (KS & 3)) ? NPW + 1 : NPW;",
    "const int nxt = cur == 0 ? 2 : cur - 1;",
    "const int NH = d.H >> 5;",
    "const int NB = d.N >> 5;",
]


def test_the_launchers_still_say_what_the_shapes_assume():
    """tests/test_gpu_mlp_kernels.py derives its row counts, hidden-block counts and the instantiation of each case from these
    lines.  If one changes, revisit the tables of gpu_util (MLP_FORMS, LNL_FORMS, WG_ROWS, the wave rows)."""
    with open(os.path.join(CSRC, "pv_mlp.hip")) as f:
        text = f.read()
    for line in PINNED:
        assert text.count(line) >= 1, "pv_mlp.hip no longer says `%s`" % line
    for (c, co), (ks2, nob16) in U.MLP_FORMS.items():
        assert "if (d.C == %d && d.Cout == %d) return launch16<%d, %d>(d, s);" % (c, co, ks2, nob16) in text
    for c, (ks, minw) in U.LNL_FORMS.items():
        assert "case %d: return launch_ln_linear<%d, %d>(*dp, s);" % (c, ks, minw) in text
