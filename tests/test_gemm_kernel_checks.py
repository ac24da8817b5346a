"""The checks of tests/test_gpu_gemm_kernels.py can fail, and its tile order is the kernels'.

The tile-order mirror (gpu_util.gemm_tile_of / gemm_item_of / gemm_place) is a bijection for every tile count 1..2100 and 1..4
channel tiles, and agrees with the formula as pv_gemm_tile.h writes it (the text is read, translated and evaluated).

On a reduced pointwise layer (9 clips of 23 voxels, 48 -> 44 channels, 16 x 16 tiles, K tiles of 16, a grid of R = 10 workgroups:
39 tiles = three whole trips and a ragged fourth, 39 % 8 = 7, an M tail, tiles that straddle clips) and a reduced (3,1,1) conv
whose frames are whole tiles (45 tiles), gpu_util.GemmExpect is fed its own float64 reference cast to the output dtype, which
passes both checks, then defective copies of it, each of which must raise with the tile named:

  - the scale / shift table of the workgroup's previous tile applied (the table double-buffered on the tile count's parity);
  - the previous tile's residual rows added;
  - a tile whose first K tile is the previous work item's (a DMA stream that was not advanced);
  - the first K step of a later tile read from the other LDS buffer (it holds the previous tile's LAST K tile);
  - a rotated reduction whose operand walk starts one tap off its weight columns;
  - two tiles swapped (a wrong remainder branch of the XCD order);
  - the ragged last trip left unwritten: the canary shows in a fresh output, old values in a reused one;
  - one bf16 ulp in one element: the tolerance check passes, the bit check raises;
  - a non-zero padding channel; a touched canary.

No GPU: the references and checks are CPU code.  The last tests pin the launcher text the shapes of the GPU cases rest on."""
import os
import re

import numpy as np
import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U

BF16 = torch.bfloat16
BM = BN = BK = 16
R = 10
B, S, CIN, COUT = 9, 23, 48, 44
M, CP = B * S, U.round_up8(COUT)


# ------------------------------------------------------------------ the tile-order mirror
def test_the_tile_order_mirror_is_a_bijection_and_its_inverse_is_the_inverse():
    for total in range(1, 2101):
        it = np.arange(total)
        tile = U.gemm_tile_of(it, total)
        assert np.array_equal(np.sort(tile), it), "total %d: not a permutation of the tiles" % total
        for tiles_n in (1, 2, 3, 4):
            m0, n0 = U.gemm_origin_of(it, total, tiles_n, 128, 256)
            assert np.array_equal(m0, tile // tiles_n * 128) and np.array_equal(n0, tile % tiles_n * 256)
            assert len(set(zip(m0.tolist(), n0.tolist()))) == total
        if total <= 300 or total % 97 == 0 or total > 2090:              # the scalar inverse, element by element
            for i, t in enumerate(tile.tolist()):
                assert U.gemm_item_of(t, total) == i and U.gemm_tile_of(i, total) == t, (total, i, t)


def test_a_place_is_voxel_and_channel_to_tile_work_item_workgroup_and_trip():
    total, tiles_n = 39, 3
    for it in range(total):
        m0, n0 = U.gemm_origin_of(it, total, tiles_n, BM, BN)
        for m, c in ((m0, n0), (m0 + BM - 1, n0 + BN - 1)):
            p = U.gemm_place(m, c, total, tiles_n, BM, BN, R)
            assert (p["item"], p["workgroup"], p["trip"], p["m0"], p["n0"]) == (it, it % R, it // R, m0, n0)
            assert p["tile"] == U.gemm_tile_of(it, total)
    assert U.gemm_place(5, 3, 7, 1, BM, BN, R)["workgroup"] == U.gemm_item_of(0, 7)      # fewer tiles than workgroups: one trip
    assert all(U.gemm_place(m, 0, 7, 1, BM, BN, R)["trip"] == 0 for m in range(0, 7 * BM, BM))


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorchvideo_amd", "csrc")
ORDER_TEXT = [
    "const int xcd = it & 7, slot = it >> 3;",
    "const int qn = total_tiles >> 3, rn = total_tiles & 7;",
    "const int tile = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;",
]


def _source(unit):
    with open(os.path.join(CSRC, unit)) as f:
        return f.read()


def _c_to_python(stmt):
    """`const int a = e1, b = e2;` -> [(a, e1), (b, e2)] with C's `p ? x : y` rewritten as Python's `(x) if (p) else (y)`"""
    body = stmt.strip().rstrip(";")
    body = re.sub(r"^const int ", "", body)
    out = []
    for part in body.split(", "):
        name, expr = part.split(" = ", 1)
        m = re.match(r"^\((.*) \? (.*) : (.*)\) \+ slot$", expr)
        if m:
            expr = "((%s) if (%s) else (%s)) + slot" % (m.group(2), m.group(1), m.group(3))
        out.append((name, expr.replace("/", "//")))
    return out


@pytest.mark.parametrize("unit", ["pv_gemm_tile.h", "pv_gemm.hip"])
def test_the_mirror_agrees_with_the_formula_as_the_source_writes_it(unit):
    """pv_gemm_tile.h (PvTileOrder: gemm8, gemm_quad, gemm_quad_half) and pv_gemm.hip (geom_of, its own copy) say the same three
    lines; evaluated as written they give gemm_tile_of for every work item of every tile count the GPU cases use and more."""
    text = _source(unit)
    for line in ORDER_TEXT:
        assert text.count(line) == 1, "%s no longer says `%s`" % (unit, line)
    prog = [pair for line in ORDER_TEXT for pair in _c_to_python(line)]
    assert [n for n, _ in prog] == ["xcd", "slot", "qn", "rn", "tile"]
    for total in list(range(1, 70)) + [516, 518, 525, 526, 530, 531, 537, 1028, 1030, 1038, 1047, 1054, 2100]:
        for it in range(total):
            env = dict(it=it, total_tiles=total)
            for name, expr in prog:
                env[name] = eval(expr, {"__builtins__": {}}, env)
            assert env["tile"] == U.gemm_tile_of(it, total), (total, it)


# ------------------------------------------------------------------ the reduced pointwise case
def _operands():
    return dict(x=U.randn((M, CIN), 11).to(BF16), w=U.randn((COUT, CIN), 12, CIN ** -0.5).to(BF16),
                res=U.randn((M, CP), 14).to(BF16), scale=U.randn((COUT,), 15, 0.2, 1.0), shift=U.randn((COUT,), 16))


def _finish(pre, scale, shift, res):
    return U.ref_act(pre * scale.double() + shift.double() + res.double(), L.ACT_RELU)


def _want(o):
    return U.ref_pointwise(o["x"], o["w"], o["scale"], o["shift"], L.ACT_RELU, res=o["res"][:, :COUT])


def _expect(want, filled=True, S_=S):
    m = want.shape[0]
    before = U.stream_buf(m, CP, BF16, fill=U.randn((m, CP), 17) if filled else None)
    return U.GemmExpect(want, before, CP, S_, BM, BN, R, U.TOL[BF16])


def _as_left_by(e, want):
    """The allocation a kernel leaves that computed `want` instead of the reference."""
    buf = e.ideal()
    e.rows(buf)[:, :COUT] = want.to(buf.dtype)
    return buf


def _later_full_tile(e, trip=2, other_channels=True, pred=None):
    """A work item on trip `trip` whose tile and whose workgroup's previous tile are both whole (16 x 16) and, if asked, lie in
    different channel tiles -> (item, tile, previous tile)"""
    for it in range(trip * R, min((trip + 1) * R, e.total)):
        t, tp = U.gemm_tile_of(it, e.total), U.gemm_tile_of(it - R, e.total)
        whole = all((b[0].stop - b[0].start, b[1].stop - b[1].start) == (BM, BN) for b in (e.tile_block(t), e.tile_block(tp)))
        if whole and (not other_channels or t % e.tiles_n != tp % e.tiles_n) and (pred is None or pred(t)):
            return it, t, tp
    raise AssertionError("no such tile")


def _named(it, t):
    return r"tile %d \(.*work item %d = workgroup %d on trip %d of %d workgroups" % (t, it, it % R, it // R, R)


def test_the_reduced_case_meets_the_trip_conditions_and_each_condition_can_fail():
    assert U.gemm_trip_conditions(M, S, COUT, BM, BN, R) == (13, 3, 39)
    assert 39 > 3 * R and 39 % R == 9 and 39 % 8 == 7 and M % BM == 15
    with pytest.raises(AssertionError, match="no more than 2 trips"):
        U.gemm_trip_conditions(4 * S, S, COUT, BM, BN, R)                        # 18 tiles
    with pytest.raises(AssertionError, match="whole number of trips"):
        U.gemm_trip_conditions(10 * BM - 3, S, COUT, BM, BN, R)                 # 30 tiles
    with pytest.raises(AssertionError, match="no remainder branch"):
        U.gemm_trip_conditions(12 * BM - 3, S, 24, BM, BN, R)                   # 24 tiles
    with pytest.raises(AssertionError, match="multiple of the tile"):
        U.gemm_trip_conditions(13 * BM, S, COUT, BM, BN, R)
    with pytest.raises(AssertionError, match="straddles"):
        U.gemm_trip_conditions(13 * BM - 1, 2 * BM, COUT, BM, BN, R)
    assert U.gemm_trip_conditions(15 * BM, 5 * BM, COUT, BM, BN, R, rotation=True) == (15, 3, 45)
    with pytest.raises(AssertionError, match="whole number of 16-voxel tiles"):
        U.gemm_trip_conditions(15 * BM, S, COUT, BM, BN, R, rotation=True)
    n = U.gemm_sub_clips(S, 3, BM, R)
    assert n == 2 and U.cdiv(n * S, BM) * 3 <= R < U.cdiv((n + 1) * S, BM) * 3


def test_both_checks_pass_on_the_reference():
    o = _operands()
    want = _want(o)
    pre = o["x"].double() @ o["w"].double().t()
    assert (_finish(pre, o["scale"], o["shift"], o["res"][:, :COUT]) - want).abs().max().item() <= 1e-12
    e = _expect(want)
    ideal = e.ideal()
    assert e.check(ideal) <= 2.0 ** -8                               # one bf16 rounding of the output
    e.check_trips(ideal, ideal.clone())


def _defective(o, e, it, t, tp, table=False, residual=False, k_tile=None):
    """The reference with tile t computed under a defect that takes state from the workgroup's previous tile tp.
    k_tile = j: the tile's FIRST K tile is the previous tile's K tile j (rows and weights)."""
    (rs, cs), (prs, pcs) = e.tile_block(t), e.tile_block(tp)
    x, w = o["x"].double(), o["w"].double()
    pre = x[rs] @ w[cs].t()
    if k_tile is not None:
        k0 = slice(0, BK)
        kj = slice(k_tile * BK, (k_tile + 1) * BK)
        pre = pre - x[rs, k0] @ w[cs, k0].t() + x[prs, kj] @ w[pcs, kj].t()
    tab = pcs if table else cs
    res = o["res"][prs, pcs] if residual else o["res"][rs, cs]
    bad = _want(o)
    bad[rs, cs] = _finish(pre, o["scale"][tab], o["shift"][tab], res)
    return bad


@pytest.mark.parametrize("defect", [dict(table=True), dict(residual=True), dict(k_tile=0), dict(k_tile=CIN // BK - 1)],
                         ids=["previous_tiles_tables", "previous_tiles_residual", "stale_first_k_tile", "other_lds_buffer"])
def test_state_of_the_previous_tile_on_a_later_trip_is_seen_and_the_tile_named(defect):
    o = _operands()
    e = _expect(_want(o))
    it, t, tp = _later_full_tile(e, trip=2, other_channels=defect == dict(table=True))
    assert it // R == 2 and tp != t
    bad = _as_left_by(e, _defective(o, e, it, t, tp, **defect))
    with pytest.raises(AssertionError, match=_named(it, t)):
        e.check(bad)
    with pytest.raises(AssertionError, match="first at voxel %d .*" % e.tile_block(t)[0].start + _named(it, t)):
        e.check_trips(e.ideal(), bad)


def test_two_tiles_swapped_by_a_wrong_remainder_branch_are_seen():
    o = _operands()
    want = _want(o)
    e = _expect(want)
    rn = e.total & 7
    # work items on either side of the remainder branch (xcd < rn and xcd >= rn) whose tiles have the same shape (the tiles of
    # the one XCD behind the branch, 35..38, are all ragged); the pair on the latest trips
    shape = lambda it: tuple(s.stop - s.start for s in e.tile_block(U.gemm_tile_of(it, e.total)))
    pairs = [(a, b) for a in range(e.total) for b in range(e.total) if (a & 7) < rn <= (b & 7) and shape(a) == shape(b)]
    a, b = max(pairs, key=lambda ab: (min(ab[0] // R, ab[1] // R), ab[0] // R + ab[1] // R))
    assert a // R >= 1 or b // R >= 1
    ta, tb = U.gemm_tile_of(a, e.total), U.gemm_tile_of(b, e.total)
    (ra, ca), (rb, cb) = e.tile_block(ta), e.tile_block(tb)
    bad = want.clone()
    bad[ra, ca], bad[rb, cb] = want[rb, cb], want[ra, ca]
    with pytest.raises(AssertionError, match="(%s|%s)" % (_named(a, ta), _named(b, tb))):
        e.check(_as_left_by(e, bad))
    with pytest.raises(AssertionError, match=r"first at .*tile %d \(.*last at .*tile %d \(" % (min(ta, tb), max(ta, tb))):
        e.check_trips(e.ideal(), _as_left_by(e, bad))


@pytest.mark.parametrize("filled", [False, True], ids=["canary_shows", "old_values_show"])
def test_an_unwritten_ragged_last_trip_is_seen(filled):
    e = _expect(_want(_operands()), filled)
    first = e.total // R * R
    assert 0 < e.total - first < R
    bad = e.ideal()
    tiles = [U.gemm_tile_of(it, e.total) for it in range(first, e.total)]
    for t in tiles:
        rs, cs = e.tile_block(t)
        wide = slice(cs.start, min(cs.start + BN, CP))                 # the padding channels of the last channel tile too
        e.rows(bad)[rs, wide] = e.rows(e.before)[rs, wide]
    assert filled or bool((e.rows(bad)[e.tile_block(tiles[0])] == U.CANARY).all())
    with pytest.raises(AssertionError, match=r"tile (%s) \(.* on trip %d of %d" % ("|".join(map(str, tiles)), e.total // R, R)):
        e.check(bad)
    with pytest.raises(AssertionError, match=r"on trip %d of %d" % (e.total // R, R)):
        e.check_trips(e.ideal(), bad)


def test_one_bf16_ulp_in_one_element_passes_the_tolerance_and_fails_the_bit_check():
    e = _expect(_want(_operands()))
    ideal, bad = e.ideal(), e.ideal()
    it, t, _ = _later_full_tile(e, trip=2)
    rs, cs = e.tile_block(t)
    m, c = rs.start + 5, cs.start + 3
    cell = e.rows(bad)[m, c:c + 1]
    cell.copy_((cell.view(torch.int16) + 1).view(BF16))
    assert not torch.equal(ideal, bad)
    e.check(bad)
    with pytest.raises(AssertionError, match=r"differ in 1 elements of 1 voxels; first at voxel %d .*channel %d, %s" % (m, c, _named(it, t))):
        e.check_trips(ideal, bad)
    with pytest.raises(AssertionError, match="differ in 1 elements"):
        e.check_trips(bad, ideal)


def test_a_non_zero_padding_channel_and_a_touched_canary_are_seen():
    e = _expect(_want(_operands()))
    assert e.written == CP == 48 and COUT < CP
    bad = e.ideal()
    e.rows(bad)[M - 1, COUT + 1] = 2.0 ** -10
    p = e.place(M - 1, COUT + 1)
    with pytest.raises(AssertionError, match=r"padding channels are not zero, first at voxel %d .*channel %d, tile %d \(" % (M - 1, COUT + 1, p["tile"])):
        e.check(bad)
    for where in (0, U.STREAM_GUARD - 1, U.STREAM_GUARD + M * CP, 2 * U.STREAM_GUARD + M * CP - 1):
        bad = e.ideal()
        bad[where] = 0.5
        with pytest.raises(AssertionError, match="canary elements"):
            e.check(bad)
        with pytest.raises(AssertionError, match="canaries differ"):
            e.check_trips(e.ideal(), bad)


# ------------------------------------------------------------------ the reduced rotation case
def test_a_rotated_reduction_that_starts_one_tap_off_is_seen():
    """(3,1,1), pt 1, frames of 4 x 4 = one 16-voxel tile, 3 clips of 5 frames: 15 x 3 = 45 tiles.  The tile of output frame t starts
    at tap (1 - t) mod 3; operands walked from the next tap on while the weight columns start where they should pair tap
    q's weights with tap q + 1's frame."""
    Bc, T, H, W, cin = 3, 5, 4, 4, 16
    Sr = T * H * W
    assert U.gemm_trip_conditions(Bc * Sr, Sr, COUT, BM, BN, R, rotation=True) == (15, 3, 45)
    x = U.randn((Bc, T, H, W, cin), 21).to(BF16)
    w = U.randn((COUT, cin, 3, 1, 1), 22, (3 * cin) ** -0.5).to(BF16)
    sc, sh = U.randn((COUT,), 23, 0.2, 1.0), U.randn((COUT,), 24)
    want = U.ref_tap_conv(x, w, (1, 1, 1), (1, 0, 0), sc, sh, L.ACT_RELU).reshape(-1, COUT)
    xp = torch.zeros(Bc, T + 2, H, W, cin, dtype=torch.float64)
    xp[:, 1:T + 1] = x
    frames = [xp[:, q:q + T].reshape(-1, cin) for q in range(3)]       # the operand rows of tap q
    wq = [w.double()[:, :, q, 0, 0] for q in range(3)]
    good = U.ref_act(sum(frames[q] @ wq[q].t() for q in range(3)) * sc.double() + sh.double(), L.ACT_RELU)
    assert (good - want).abs().max().item() <= 1e-12
    off = U.ref_act(sum(frames[(q + 1) % 3] @ wq[q].t() for q in range(3)) * sc.double() + sh.double(), L.ACT_RELU)
    e = _expect(want, S_=Sr)
    inner = lambda tile: (e.tile_block(tile)[0].start % Sr) // (H * W) in (1, 2, 3)      # all three taps inside the clip
    it, t, _ = _later_full_tile(e, trip=2, other_channels=False, pred=inner)
    rs, cs = e.tile_block(t)
    bad = want.clone()
    bad[rs, cs] = off[rs, cs]
    e.check(e.ideal())
    with pytest.raises(AssertionError, match=_named(it, t)):
        e.check(_as_left_by(e, bad))


# ------------------------------------------------------------------ the launcher text the GPU cases' shapes rest on
PINNED = {
    "pv_gemm_tile.h": ORDER_TEXT + [
        "m0 = (long)(tile / tiles_n) * BM;",
        "n0 = (tile % tiles_n) * BN;",
        "const long resident = 256;",
        "dim3 grid((unsigned)(total < resident ? total : resident)), block(threads);",
        "iss_it += gridDim.x;",
        "if (d.cin % 64 != 0 || K % k_mult != 0 || K < k_min) return false;",
    ],
    "pv_gemm.hip": ORDER_TEXT + [
        "constexpr int BM = 128;",
        "constexpr int BN = 128;",
        "constexpr int BMV = 64 * VT;",
        "gg.m0 = (long)(tile / tiles_n) * BMV;",
        "gg.n0 = tile_n * BN;",
        "const long resident = 2 * 256;",
        "const long t128 = pv_ceil_div(M, 128) * tiles_n;",
        "const int force_vt = pv_tune(\"gemm_vt\", 0);",
        "const int vt = force_vt ? force_vt : (2 * t128 <= resident ? 1 : 2);",
        "const long tiles_m = pv_ceil_div(M, 64 * vt);",
        "const int tiles_n = (int)pv_ceil_div(cout_p8, BN);",
        "dim3 grid((unsigned)(total < resident ? total : resident)), block(kThreads);",
        "for (; it < total_tiles; it += gridDim.x) {",
        "((long)d.Ho * d.Wo) % (64 * vt) == 0 && pv_tune(\"gemm_tap_rot\", 1)) ? 1 : 0;",
        "else if (!pw && taps > 1 && d.cin % 64 == 0 && pv_tune(\"gemm_umode\", 1))",
    ],
    "pv_gemm8.hip": [
        "constexpr int BMV8 = 256;",
        "constexpr int BN = 64 * CT;",
        "if (K < 3 * 64) return PV_ERR_UNSUPPORTED;",
        "const long tiles_m = pv_ceil_div(M, BMV8);",
        "const int tiles_n = (int)pv_ceil_div(cout_p8, 64 * ct);",
        "if (mode == 2 || mode == 4) {",
        "if (ct == 4) return pw ? launch8<true, 4, 32, 4>(d, tiles_n, total, s) : launch8<false, 4, 32, 4>(d, tiles_n, total, s);",
        "if (pv_tune(\"gemm8_bk\", 64) == 32)",
        "return pw ? launch8<true, 2, 32, 4>(d, tiles_n, total, s) : launch8<false, 2, 32, 4>(d, tiles_n, total, s);",
        "return pw ? launch8<true, 2, 64, 3>(d, tiles_n, total, s) : launch8<false, 2, 64, 3>(d, tiles_n, total, s);",
        "for (int it = blockIdx.x; it < total_tiles; it += gridDim.x) {",
    ],
    "pv_gemm9.hip": [
        "constexpr int BT9 = 256;",
        "if (!pv_gemm_stream_geometry_ok(d, 128, 256, M, K)) return false;",
        "tiles_m = pv_ceil_div(M, BT9);",
        "tiles_n = (int)pv_ceil_div(pv_round_up(d.cout, 8), BT9);",
        "const int mode = pv_tune(\"gemm9\", 1);",
        "if (mode != 2 && ((t256 < pv_tune(\"gemm9h_below\", 200) && !one_round_here) || padded_here || pv_tune(\"gemm9h\", 1) == 2)) {",
        "const bool rows = pw && d.x_bs == (long)d.To * d.Ho * d.Wo * d.ldx;",
        "if (var < 0) var = K >= 384 ? 2 : 0;",
        "const int tap_rot = !PW && d.kt > 1 && d.st == 1 && d.dil_t <= 1 && (d.Ho * d.Wo) % BT9 == 0 && pv_tune(\"gemm9_tap_rot\", 1);",
        "for (int it = blockIdx.x; it < total_tiles; it += gridDim.x, ++jt) {",
    ],
    "pv_gemm9h.hip": [
        "constexpr int BMH = 128, BNH = 256;",
        "constexpr int BM = TR ? 2 * BMH : BMH, BN = TR ? BNH / 2 : BNH;",
        "if (!pv_gemm_stream_geometry_ok(d, 192, 384, M, K)) return PV_ERR_UNSUPPORTED;",
        "int tr = pv_tune(\"gemm9h_tr\", -1);",
        "const long tiles_m = pv_ceil_div(M, tr ? 2 * BMH : BMH);",
        "const int tiles_n = (int)pv_ceil_div(cout_p8, tr ? BNH / 2 : BNH);",
        "const bool rows = pw && d.x_bs == (long)d.To * d.Ho * d.Wo * d.ldx;",
        "const int tap_rot = !PW && d.kt > 1 && d.st == 1 && d.dil_t <= 1 && (d.Ho * d.Wo) % (TR ? 2 * BMH : BMH) == 0 && pv_tune(\"gemm9_tap_rot\", 1);",
        "for (int it = blockIdx.x; it < total_tiles; it += gridDim.x, ++jt) {",
    ],
}


@pytest.mark.parametrize("unit", sorted(PINNED))
def test_the_launchers_still_size_their_grids_and_tiles_as_the_multi_trip_shapes_assume(unit):
    """tests/test_gpu_gemm_kernels.py derives its tile counts, its trip counts and the forced forms from these lines (it quotes
    them).  If one changes, a grid or a tile was resized: revisit those shapes, or the cases quietly go back to one trip."""
    text = _source(unit)
    for line in PINNED[unit]:
        assert text.count(line) >= 1, "%s no longer says `%s`" % (unit, line)
