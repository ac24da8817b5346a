"""The checks of tests/test_gpu_attention_kernels.py can fail, and the claims its families make hold.  No GPU: the references, the
operand families, the mirror of the rescale rule, the fp32 replay of the kernels' arithmetic (gpu_util.replay_attention: KT-key
tiles, P rounded to bf16 for the PV product, l from the unrounded p, kDefer decided per 32-row wave) and gpu_util.AttnExpect are
CPU code.

  - fp32(0.08664339780807495) * fp32(1.44269504088896340736) is exactly 0.125: families A and B have integer exponent arguments.
  - The correct replay passes every family's check on every route: A bit for bit (bf16) or within 2^-21 (fp32); B within 0.6 of
    the one bf16 ulp the bound allows; C at most 7e-3 on the worst query row of every shape the GPU file uses.
  - Each defect, applied to the replay, fails the check of the family it is aimed at, and the failure names the place:
      two keys of V swapped inside a 16-key slot, a tile's V from three tiles earlier, the two lane halves each with their own
      maximum, head h reading head h + 1, the mask one key short                       -> A (bits)
      alpha not applied to l (every rising schedule), one p pair missing from l (every schedule)   -> B
      the mask one key long (key Nk, a zero row, scored 0)                              -> C at Nk = KT + 1, and Nk = 1 .. 4
    while `alpha not applied to l` reads exactly the correct replay's number under the metric of tests/test_gpu_kernels.py on its
    randn operands: that is the gap.
  - The construction conditions of A and B hold for every case and can fail; the mirror finds, per route, everything B must
    contain; the tile counts are the ones the step forms need.
  - Splitting a wave changes a rescale point (the caveat of family E), shown with the mirror.
  - AttnExpect tells a wrong value, a NaN, a touched pad channel and a touched row of another sub-range apart.
  - The source lines the constructions rest on are still in csrc/pv_attn64.hip, pv_attn.hip and pv_attn.h."""
import os

import numpy as np
import pytest
import torch

import gpu_util as U

F32, BF16 = torch.float32, torch.bfloat16
CFGS = sorted(U.ATTN_ROUTES, key=lambda c: (c[0] == F32, c[1]))
IDS = ["%s_%d" % ("bf16" if c[0] == BF16 else "fp32", c[1]) for c in CFGS]
ROUTE_CFGS = [(BF16, 96), (BF16, 64), (BF16, 128), (F32, 32)]          # one head_dim per kernel body
ROUTE_IDS = ["w64", "pipe", "attn_bf16", "attn_fp32"]


def _w64(cfg):
    return U.ATTN_ROUTES[cfg][0] == "attn_w64_kernel"


def _float_scale(o):
    return float(torch.tensor(o["scale"], dtype=F32)) * 1.4426950408889634


def _expect(o, cfg, mode, bound=None, log2_scale=0.125, residual=False, kind="packed", **sub):
    B, Nq, H, D = o["q"].shape
    lay = U.AttnLayout(kind, B, H, D, Nq, o["k"].shape[1], cfg[0])
    want, dom = U.ref_attention(o["q"], o["k"], o["v"], log2_scale, residual)
    return U.AttnExpect(want, dom, lay, U.ATTN_ROUTES[cfg][0], mode, bound, **sub)


def _replay(o, cfg, defect=None, residual=False):
    return U.replay_attention(o["q"], o["k"], o["v"], U.attn_log2_scale(o["scale"]), residual, cfg[0], _w64(cfg), defect)


def _a_case(cfg, Nk, B=1, H=2):
    o = U.make_attn_select(B, H, cfg[1], U.attn_select_nq(Nk), Nk)
    U.attn_select_conditions(o)
    e = _expect(o, cfg, "bits") if cfg[0] == BF16 else _expect(o, cfg, "elem", 2.0 ** -21)
    return o, e


def test_the_integer_scale_times_log2e_is_exactly_an_eighth_in_fp32():
    assert np.float32(U.ATTN_INT_SCALE) * np.float32(U.ATTN_LOG2E_F32) == np.float32(0.125)
    assert U.attn_log2_scale(U.ATTN_INT_SCALE) == 0.125
    assert U.attn_log2_scale(96 ** -0.5) != 96 ** -0.5 * 1.4426950408889634          # the general case does round


def test_the_tile_counts_reach_every_step_form():
    for KT, nks in U.ATTN_NK.items():
        assert tuple(U.cdiv(n, KT) for n in nks) == U.ATTN_TILES
        assert {n % KT == 0 for n in nks} == {True, False} and nks[-2] % KT and not nks[-1] % KT and not nks[-3] % KT
    nt = max(U.ATTN_TILES)
    assert {(t & 1, t % 3) for t in range(nt - 1)} == {(p, s) for p in (0, 1) for s in (0, 1, 2)}      # every pair in a `more` step
    assert {t % 2 for t in U.ATTN_TILES} == {0, 1}               # both tail forms of the loop unrolled by two
    assert (nt - 1) // 2 >= 2 and 7 in U.ATTN_TILES              # at least two trips of it, at an odd and an even count
    assert "parity 1, V slot 2" in U.attn_step_form(5, 512, 64) and U.attn_step_form(7, 485, 64) == "ragged last step"
    assert U.attn_step_form(0, 64, 64) == "last step, scores from the prologue"
    assert set(U.ATTN_C_NK) == set(U.ATTN_NK) and all(n[0] == kt + 1 for kt, n in U.ATTN_C_NK.items())


# ------------------------------------------------------------------ the correct replay passes
@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_the_correct_replay_passes_family_a_on_every_route(cfg):
    KT = U.attn_kt(cfg[0])
    for Nk in (U.ATTN_NK[KT][2], U.ATTN_NK[KT][4], U.ATTN_NK[KT][-2]):
        for residual in (False, True):
            o = U.make_attn_select(1, 2, cfg[1], U.attn_select_nq(Nk), Nk)
            assert U.attn_select_conditions(o) >= U.ATTN_A_GAP
            e = _expect(o, cfg, "bits", residual=residual) if cfg[0] == BF16 else _expect(o, cfg, "elem", 2.0 ** -21, residual=residual)
            buf = e.ideal(_replay(o, cfg, residual=residual))
            assert e.check(buf) == 0.0                            # the fp32 replay too returns the selected row exactly


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_every_family_a_case_meets_its_conditions(cfg):
    KT = U.attn_kt(cfg[0])
    for Nk in U.ATTN_NK[KT]:
        B, H = (2, 3) if Nk <= KT + 1 else (1, 2)
        o = U.make_attn_select(B, H, cfg[1], U.attn_select_nq(Nk), Nk)
        assert U.attn_select_conditions(o) >= U.ATTN_A_GAP
        assert o["q"].shape[1] >= Nk + U.ATTN_WG_ROWS and o["q"].abs().max() == 64
        hi = (o["sel"] >> 2) & 1
        assert Nk < 8 or 0.3 < hi.double().mean() < 0.7           # half of the selected positions live in lane half 1
        if Nk > 1:
            assert {int(x) for x in o["sel"][0, 0]} >= {Nk - 1, 0}        # the last key before the mask is selected


def test_the_family_a_conditions_can_fail():
    o = U.make_attn_select(1, 1, 32, U.attn_select_nq(37), 37)
    o["k"][0, 5, 0] = o["k"][0, 9, 0]                            # two equal codes: no gap between them
    with pytest.raises(AssertionError):
        U.attn_select_conditions(o)
    o = U.make_attn_select(1, 1, 32, U.attn_select_nq(37), 37)
    o["v"][0, 5, 0] = o["v"][0, 9, 0]
    with pytest.raises(AssertionError, match="two rows of V are equal"):
        U.attn_select_conditions(o)


@pytest.mark.parametrize("cfg", ROUTE_CFGS, ids=ROUTE_IDS)
def test_the_correct_replay_stays_inside_family_b_with_room(cfg):
    KT = U.attn_kt(cfg[0])
    for Nk in U.ATTN_NK[KT][-3:-1]:
        for sch in U.ATTN_B_SCHEDULES:
            o = U.make_attn_levels(sch, 1, 2, cfg[1], 165, Nk, KT)
            a = U.attn_level_args(o)
            assert o["v"].min() == 1 and o["v"].max() == 8 and a.max() - a.min() < 120      # exp2 of the spread stays a normal fp32
            e = _expect(o, cfg, "elem", U.attn_level_bound(cfg[0], Nk))
            err = e.check(e.ideal(_replay(o, cfg)), "replay %s Nk %d" % (sch, Nk))
            assert err <= 0.6 * e.bound, "the replay spends %.2f of the bound at %s, Nk %d" % (err / e.bound, sch, Nk)


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_the_mirror_finds_everything_family_b_must_contain(cfg):
    KT = U.attn_kt(cfg[0])
    got, per = set(), {}
    for Nk in U.ATTN_NK[KT][-3:-1]:
        for sch in U.ATTN_B_SCHEDULES:
            o = U.make_attn_levels(sch, 1, 2, cfg[1], 165, Nk, KT)
            per[sch, Nk] = U.attn_mirror_coverage(U.attn_mirror(U.attn_level_args(o), KT, _w64(cfg)), Nk, KT)
            got |= per[sch, Nk]
    assert got >= U.ATTN_B_COVER, sorted(U.ATTN_B_COVER - got)
    assert all(not per["flat", n] and not per["falling", n] and not per["plus7", n] for n in U.ATTN_NK[KT][-3:-1])   # never rescale after start-up
    assert all("no rescale at a rise of exactly 8" in per["plus8", n] for n in U.ATTN_NK[KT][-3:-1])


@pytest.mark.parametrize("cfg", ROUTE_CFGS, ids=ROUTE_IDS)
def test_the_correct_replay_is_at_most_7e_3_on_the_worst_row_of_every_family_c_shape(cfg):
    KT = U.attn_kt(cfg[0])
    for var in U.ATTN_C_VARIANCES:
        for Nk in U.ATTN_C_NK[KT]:
            o = U.make_attn_float(1, 2, cfg[1], U.ATTN_C_NQ, Nk, var, cfg[0])
            e = _expect(o, cfg, "row", U.TOL[cfg[0]], log2_scale=_float_scale(o))
            err = e.check(e.ideal(_replay(o, cfg)), "replay variance %d Nk %d" % (var, Nk))
            assert err <= (7e-3 if cfg[0] == BF16 else 1e-5), (var, Nk, err)
            s = torch.einsum("bqhd,bkhd->bhqk", o["q"], o["k"]) * _float_scale(o) / 1.4426950408889634
            assert 0.8 * var < s.var().item() < 1.25 * var


# ------------------------------------------------------------------ the defects fail the check aimed at them
@pytest.mark.parametrize("defect", ["swap_v", "stale_v", "halves", "head", "mask_short"])
@pytest.mark.parametrize("cfg", ROUTE_CFGS, ids=ROUTE_IDS)
def test_family_a_fails_on_defects_of_pairing_slots_halves_heads_and_mask(cfg, defect):
    KT = U.attn_kt(cfg[0])
    Nk = U.ATTN_NK[KT][-2]                                       # 8 tiles, the last ragged
    o, e = _a_case(cfg, Nk)
    with pytest.raises(AssertionError, match=r"batch item \d, head \d, query row \d+ \(work item \d+ of the launch, query block \d, wave \d, "
                                             r"lane \d+\), channel \d+ \(channel block \d, lane half \d\).*dominant key \d+ is in key tile \d") as info:
        e.check(e.ideal(_replay(o, cfg, defect)), defect)
    msg = str(info.value)
    if defect == "mask_short":
        assert "dominant key %d is in key tile 7" % (Nk - 1) in msg and "ragged last step" in msg
    if defect == "stale_v":
        bad = (e.values(e.ideal(_replay(o, cfg, defect))).double() != e.want).any(-1)       # (B, Nq, H): the rows of tiles >= 3, only
        assert {int(t) for t in (e.dom.permute(0, 2, 1)[bad] // KT)} == set(range(3, 8))


@pytest.mark.parametrize("cfg", ROUTE_CFGS, ids=ROUTE_IDS)
def test_family_b_fails_when_alpha_misses_l_or_a_pair_of_p_does(cfg):
    KT = U.attn_kt(cfg[0])
    for Nk in U.ATTN_NK[KT][-3:-1]:
        for sch in U.ATTN_B_SCHEDULES:
            o = U.make_attn_levels(sch, 1, 2, cfg[1], 165, Nk, KT)
            e = _expect(o, cfg, "elem", U.attn_level_bound(cfg[0], Nk))
            with pytest.raises(AssertionError, match=r"beyond .* \|want\|"):
                e.check(e.ideal(_replay(o, cfg, "pair_l")), "pair_l %s" % sch)
            if sch in ("plus7", "plus8", "plus9", "saw"):        # every rising schedule
                with pytest.raises(AssertionError, match=r"beyond .* \|want\|"):
                    e.check(e.ideal(_replay(o, cfg, "alpha_l")), "alpha_l %s" % sch)


@pytest.mark.parametrize("cfg", ROUTE_CFGS, ids=ROUTE_IDS)
def test_family_c_and_the_short_key_counts_fail_on_a_mask_one_key_long(cfg):
    KT = U.attn_kt(cfg[0])
    cases = [U.make_attn_float(1, 2, cfg[1], U.ATTN_C_NQ, KT + 1, 1, cfg[0])] + [U.make_attn_float(1, 2, cfg[1], 70, n, 1, cfg[0]) for n in (1, 2, 3, 4)]
    for o in cases:
        e = _expect(o, cfg, "row", U.TOL[cfg[0]], log2_scale=_float_scale(o))
        e.check(e.ideal(_replay(o, cfg)))
        with pytest.raises(AssertionError, match="query row beyond"):
            e.check(e.ideal(_replay(o, cfg, "mask_long")), "mask_long")


@pytest.mark.parametrize("hd,Nq,Nk", [(96, 129, 65), (96, 1000, 197), (64, 40, 192), (96, 40, 384)])
def test_alpha_missing_from_l_is_invisible_on_randn_operands_at_unit_variance(hd, Nq, Nk):
    """The operands and the metric of tests/test_gpu_kernels.py::test_attention_matches_reference: no tile's maximum exceeds the
    held one by more than kDefer after start-up, so the defect never executes.  At variance 12 it is above 0.3 of the worst row and above 0.1 of the launch's abs-max."""
    cfg = (BF16, hd)
    o = dict(q=U.randn((1, Nq, 1, hd), 1).bfloat16().double(), k=U.randn((1, Nk, 1, hd), 2).bfloat16().double(),
             v=U.randn((1, Nk, 1, hd), 3).bfloat16().double(), scale=hd ** -0.5)
    assert torch.equal(_replay(o, cfg), _replay(o, cfg, "alpha_l"))
    want = U.ref_attention(o["q"], o["k"], o["v"], _float_scale(o), False)[0]
    assert U.rel_err(_replay(o, cfg), want) <= 1e-2
    o12 = U.make_attn_float(1, 2, hd, U.ATTN_C_NQ, 485, 12, BF16)
    want12 = U.ref_attention(o12["q"], o12["k"], o12["v"], _float_scale(o12), False)[0]
    d12 = (_replay(o12, cfg, "alpha_l").double() - want12).abs()
    assert (d12.amax(-1) / want12.abs().amax(-1)).max() > 0.3 and d12.max() / want12.abs().max() > 0.1     # per row; per launch


# ------------------------------------------------------------------ the caveat of family E
def test_splitting_a_wave_changes_a_rescale_point():
    """__any: a lane's rescale points depend on the other 31 rows of its wave.  Rows 16 .. 31 launched alone lose lane 13, the one
    that trips: the same rows rescale at the late key's tile in the full launch and hold their maximum in the sub-launch.  A
    sub-range of family E therefore starts and ends on whole waves (it starts at a multiple of 128 and ends at one or at Nq)."""
    for w64 in (True, False):
        o = U.make_attn_levels("one_lane", 1, 1, 32, 32, 448, 64)
        a = U.attn_level_args(o)
        full, part = U.attn_mirror(a, 64, w64), U.attn_mirror(a[16:], 64, w64)
        assert [e["rescaled"] for e in full][1:] == [False] * 5 + [True]
        assert [e["rescaled"] for e in part][1:] == [False] * 6
    # and what lies in the idle lanes differs by kernel: row Nq - 1 again for attn_w64_kernel, zeros for the others
    x = torch.arange(6.0).view(3, 2)
    assert torch.equal(U._attn_pad_rows(x, True)[3:], x[2:].expand(29, 2)) and (U._attn_pad_rows(x, False)[3:] == 0).all()


# ------------------------------------------------------------------ AttnExpect itself
def test_attn_expect_tells_values_nan_pads_and_foreign_rows_apart():
    cfg = (BF16, 32)
    o = U.make_attn_float(2, 3, 32, 2 * 128 + 37, 65, 4, BF16)
    e = _expect(o, cfg, "row", 1e-2, log2_scale=_float_scale(o), kind="wide")
    lay, good = e.lay, e.ideal()
    assert e.check(good) <= 2.0 ** -8
    assert len(set(lay.ld.values())) == 4 and all(lay.ld[x] > 96 and lay.bs[x] > lay.ld[x] * (293 if x in "qo" else 65) for x in "qkvo")
    bad = good.clone()
    lay.view(bad, "o")[1, 200, 2, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"batch item 1, head 2, query row 200 \(work item 16 of the launch, query block 1, wave 2, lane 40\), "
                                             r"channel 7 \(channel block 0, lane half 1\)"):
        e.check(bad)
    for off in (96, lay.ld["o"] * 293, lay.bs["o"] - 1, good.numel() - 1):         # a pad channel, the row behind Nq, the gap, the tail
        bad = good.clone()
        bad[off] = 1.0
        with pytest.raises(AssertionError, match="does not own changed"):
            e.check(bad)
    sub = _expect(o, cfg, "row", 1e-2, log2_scale=_float_scale(o), kind="wide", b=(1, 2), h=(2, 3), rows=(128, 293))
    part = sub.ideal()
    sub.check(part)
    sub.same_bits(good, part)
    assert (sub.values(part) == lay.view(good, "o")[1:2, 128:293, 2:3]).all()
    assert (part != U.CANARY).sum() <= 165 * 32
    assert "work item 0 of the launch, query block 0, wave 0, lane 0" in sub.where(1, 128, 2, 0)
    bad = part.clone()
    lay.view(bad, "o")[1, 127, 2, 0] = 1.0                        # a row below the sub-range
    with pytest.raises(AssertionError, match="does not own changed"):
        sub.check(bad)
    bad = part.clone()
    lay.view(bad, "o")[1, 130, 2, 5] += 1.0
    with pytest.raises(AssertionError, match="differ between the full launch and the sub-launch"):
        sub.same_bits(good, bad)


def test_every_operand_gap_is_nan_and_fused_slices_share_one_buffer():
    o = U.make_attn_float(2, 3, 32, 40, 65, 1, BF16)
    for kind in ("packed", "wide", "fused"):
        lay = U.AttnLayout(kind, 2, 3, 32, 40, 65, BF16)
        bufs = lay.inputs(o["q"], o["k"], o["v"])
        assert (bufs["q"] is bufs["k"] is bufs["v"]) == (kind == "fused")
        for x in "qkv":
            assert torch.equal(lay.view(bufs[x], x).double(), o[x])
        seen = sum(b.numel() for b in ({id(b): b for b in bufs.values()}).values())
        finite = sum(int(torch.isfinite(b).sum()) for b in ({id(b): b for b in bufs.values()}).values())
        assert finite == o["q"].numel() + 2 * o["k"].numel() and seen > finite
        guard = U.ATTN_GUARD_TILES * 64 * lay.ld["k"]
        assert torch.isnan(bufs["k"][-guard:]).all() and torch.isnan(bufs["v"][-guard:]).all()     # 6 key tiles behind the last item
        assert (lay.output() == U.CANARY).all()
    with pytest.raises(AssertionError, match="is not exact"):
        U.AttnLayout("packed", 2, 3, 32, 40, 65, BF16).inputs(o["q"] * 1.001, o["k"], o["v"])


# ------------------------------------------------------------------ the source lines the constructions rest on
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorchvideo_amd", "csrc")
PINNED = {
    "pv_attn.hip": [
        ("constexpr int kQB = 128;  // query rows per workgroup", 1),
        ("static constexpr int KT = 64;          // keys per tile", 1),
        ("static constexpr int KT = 32;", 1),
        ("static constexpr int NBUF = 2;", 1),
        ("static constexpr int NBUF = 1;", 1),
        ("const int q_row = it.qblk * kQB + wave * 32 + l31;", 2),
        ("const float sc = d.scale * 1.44269504088896340736f;", 2),
        ("constexpr float kDefer = 8.0f;", 2),
        ("if (__any(mx > m_run + kDefer)) {", 2),
        ("float m_run = -1e30f, l_run = 0.f;", 2),
        ("l_run *= alpha;", 2),
        ("else qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};", 2),
        ("if ((t * KT + sub * 32 + crow(r, hi)) >= d.Nk) s[sub][r] = -INFINITY;", 1),
        ("if ((t * KT + sub * 32 + crow(r, hi)) >= d.Nk) sc_[sub][r] = -1e30f;", 1),
        ("if constexpr (sizeof(T) == 2 && D <= 64) {", 1),
        ("if (kv_bytes < 0x7fffffffL) {", 1),
        ("PV_LAUNCH((attn_pipe_kernel<D>), dim3((unsigned)total), dim3(kThreads), 0, s, d, nqb, (int)total);", 1),
        ("PV_LAUNCH((attn_kernel<T, D>), dim3((unsigned)total), dim3(kThreads), 0, s, d, nqb, (int)total);", 1),
        ("const int nqb = (d.Nq + kQB - 1) / kQB;", 1),
        ("const int r = pv_attn_w64_try(d, s);", 1),
        ("if (r != PV_ERR_UNSUPPORTED) return r;", 1),
        ("if (d.dtype == PV_BF16) return launch_attn_d<bf16_t>(d, s);", 1),
        ("if (d.dtype == PV_F32) return launch_attn_d<float>(d, s);", 1),
        ("const int align = d.dtype == PV_BF16 ? 8 : 4;", 1),
        ("if (!(d.scale > 0.f) || isinf(d.scale)) return PV_ERR_INVALID;", 1),
    ] + [("case %d: return launch_attn<T, %d>(d, s);" % (hd, hd), 1) for hd in (32, 64, 96, 128)],
    "pv_attn64.hip": [
        ("constexpr int D = 96;          // head dim", 1),
        ("constexpr int KT = 64;         // keys per tile", 1),
        ("constexpr int kRowsWG = 128;   // query rows per workgroup: 32 per wave", 1),
        ("const int q_row = qblk * kRowsWG + wave * 32 + l31;", 1),
        ("const int r = q_ok ? q_row : d.Nq - 1;", 1),
        ("constexpr float kDefer = 8.0f;", 1),
        ("if (__builtin_expect(__any(mxs > m_run + kDefer), 0)) {", 1),
        ("l_run *= alpha;", 1),
        ("if (KT <= d.Nk) m_run = attn_max_swap32(mx * sc);", 1),
        ("const float sc = d.scale * 1.44269504088896340736f;", 1),
        ("if ((t * KT + sub * 32 + crow(r, hi)) >= d.Nk) sc_[sub][r] = -1e30f;", 1),
        ("__shared__ __attribute__((aligned(16))) char smem[2 * K_BYTES + 3 * V_BYTES];", 1),
        ("const lds_ptr_t vslot = lds_base(vsm + (t % 3) * V_BYTES + v_rd);", 1),
        ("const lds_ptr_t kslot = lds_base(ksm + ((t + 1) & 1) * K_BYTES + k_rd);", 1),
        ("u32x4 kreg[2][NDB], vreg[2][NDB];", 1),
        ("if (f == 2 + NDB) load_k(par, t + 5);", 1),
        ("for (; t + 2 < ntiles; t += 2) {", 1),
        ("if (ntiles - t == 2) {", 1),
        ("if (d.dtype != PV_BF16 || d.head_dim != D) return PV_ERR_UNSUPPORTED;", 1),
        ("if (kv_bytes >= 0x7fffffffL) return PV_ERR_UNSUPPORTED;", 1),
        ("const int nqb = (d.Nq + kRowsWG - 1) / kRowsWG;", 1),
    ],
    "pv_attn.h": [
        ("__device__ __forceinline__ int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }", 1),
        ("return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p), 0, (int)(((long)(Nk - 1) * ld + D) * 2), 0x00020000);", 1),
        ("const int xcd = id & 7, slot = id >> 3;", 1),
        ("const int qn = total >> 3, rn = total & 7;", 1),
    ],
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_the_kernels_still_say_what_the_constructions_assume(name):
    """tests/test_gpu_attention_kernels.py derives its tile counts, step forms, wave composition, the start of m_run, the fill of
    idle lanes and the route of each case from these lines.  If one changes, revisit the attention tables of gpu_util."""
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    for line, count in PINNED[name]:
        assert text.count(line) == count, "%s says `%s` %d times, not %d" % (name, line, text.count(line), count)
    assert (U.ATTN_WG_ROWS, U.ATTN_WAVE_ROWS, U.ATTN_DEFER, U.attn_kt(BF16), U.attn_kt(F32)) == (128, 32, 8.0, 64, 32)
    assert {c: k for c, (k, _) in U.ATTN_ROUTES.items()} == {
        (dt, hd): ("attn_w64_kernel" if (dt, hd) == (BF16, 96) else "attn_pipe_kernel" if dt == BF16 and hd <= 64 else "attn_kernel")
        for dt in (BF16, F32) for hd in (32, 64, 96, 128)}
    assert 1.44269504088896340736 == U.ATTN_LOG2E_F32 and "%.17g" % U.ATTN_INT_SCALE == "0.086643397808074951"
