"""The checks of tests/test_gpu_stream_kernels.py can fail.  On a reduced gated pointwise conv (9 clips of 75 voxels, 32-voxel
groups, 22 groups against candidate grids of 4 and 6 chunks: more than two whole trips and a ragged last one under both) and a
reduced tap conv -> pointwise pair, gpu_util.StreamExpect is fed its own float64 reference cast to the output dtype, which
passes both checks, then defective copies of it, each of which must raise:

  - the rows of a group g on a later trip hold the values of group g - nchunks (a stale prefetched operand), per candidate grid;
  - the rows of a later trip take the previous clip's gate row (a gate cache that was not refreshed);
  - in a tile that straddles two clips, the rows of the second clip take the first clip's gate row;
  - the previous group's residual is added;
  - the ragged last trip is not written: the canary shows in an output that went in as canaries, the old values in a wide buffer;
  - one voxel is one bf16 ulp off in one channel: the tolerance check passes, the bit check raises;
  - a non-zero padding channel; a touched canary; a changed element of the slice the launch does not own.

The failure messages are asserted to name the group of the defect.  No GPU: the references and checks are CPU code.  The last
test pins the launcher text the shapes of the GPU cases were derived from."""
import os

import pytest
import torch

from pytorchvideo_amd import _lib as L
import gpu_util as U

B, S, CIN, COUT, GVOX, CHUNKS = 9, 75, 16, 12, 32, [4, 6]
M = B * S
NGROUPS = U.cdiv(M, GVOX)
LD, C_OFF = 32, 8


def _operands():
    x = U.randn((M, CIN), 11).to(torch.bfloat16)
    w = U.randn((COUT, CIN), 12, CIN ** -0.5).to(torch.bfloat16)
    gate = torch.sigmoid(U.randn((B, CIN), 13, 2.0))                 # a row per clip: another clip's row moves the result
    res = U.randn((M, COUT), 14).to(torch.bfloat16)
    return dict(x=x, w=w, gate=gate, res=res, scale=U.randn((COUT,), 15, 0.2, 1.0), shift=U.randn((COUT,), 16))


def _want(o, clip=None, res=None):
    clip = torch.arange(M) // S if clip is None else clip
    return U.ref_pointwise(o["x"], o["w"], o["scale"], o["shift"], L.ACT_RELU, gate=o["gate"], a_act=L.ACT_SWISH, clip=clip,
                           res=o["res"] if res is None else res)


def _expect(want, filled=True):
    """filled: the rows hold a neighbour's values before the launch (a wide buffer); else the canary, as a plain output does."""
    before = U.stream_buf(M, LD, torch.bfloat16, fill=U.randn((M, LD), 17) if filled else None)
    return U.StreamExpect(want, before, LD, S, GVOX, CHUNKS, U.TOL[torch.bfloat16], c_off=C_OFF)


def _as_left_by(e, want):
    """The allocation a kernel leaves that computed `want` instead of the reference."""
    buf = e.ideal()
    e.rows(buf)[:, C_OFF:C_OFF + COUT] = want.to(buf.dtype)
    return buf


def _rows_of(g):
    return slice(g * GVOX, min((g + 1) * GVOX, M))


def test_the_reduced_case_runs_two_whole_trips_and_a_ragged_one():
    U.assert_trips(NGROUPS, CHUNKS)
    assert S % 16 == 11 and M % 16 != 0
    with pytest.raises(AssertionError, match="whole number of trips"):
        U.assert_trips(24, CHUNKS)
    with pytest.raises(AssertionError, match="no more than 2 trips"):
        U.assert_trips(11, CHUNKS)
    assert U.stream_chunks(256, (1, 2, 3, 4), 3) == [86, 171, 256, 342]


def test_both_checks_pass_on_the_reference():
    e = _expect(_want(_operands()))
    ideal = e.ideal()
    assert e.check(ideal) <= 2.0 ** -8                              # one bf16 rounding of the output
    e.check_trips(ideal, ideal.clone())


@pytest.mark.parametrize("n", CHUNKS)
def test_a_stale_prefetched_operand_is_seen_and_named(n):
    o = _operands()
    want = _want(o)
    e = _expect(want)
    g = 2 * n + 1                                                    # third trip under this grid
    bad = want.clone()
    bad[_rows_of(g)] = want[_rows_of(g - n)][: _rows_of(g).stop - _rows_of(g).start]
    with pytest.raises(AssertionError, match=r"group g = %d, .*2 of nchunks %d" % (g, n)):
        e.check(_as_left_by(e, bad))
    with pytest.raises(AssertionError, match=r"first at voxel %d .*group g = %d," % (g * GVOX, g)):
        e.check_trips(e.ideal(), _as_left_by(e, bad))


def test_a_gate_row_of_the_previous_clip_on_a_later_trip_is_seen():
    o = _operands()
    e = _expect(_want(o))
    g = 2 * CHUNKS[1] + 2
    clip = torch.arange(M) // S
    assert clip[g * GVOX] > 0
    clip[_rows_of(g)] -= 1
    with pytest.raises(AssertionError, match=r"group g = %d," % g):
        e.check(_as_left_by(e, _want(o, clip=clip)))


def test_the_first_clips_gate_row_on_the_second_clips_rows_of_a_straddling_tile_is_seen():
    o = _operands()
    e = _expect(_want(o))
    clip = torch.arange(M) // S
    tiles = [t for t in range(M // GVOX) if clip[t * GVOX] != clip[t * GVOX + GVOX - 1] and t >= CHUNKS[1]]
    t = tiles[-1]
    rows = torch.arange(t * GVOX, (t + 1) * GVOX)
    second = rows[clip[rows] != clip[rows[0]]]
    clip[second] = int(clip[rows[0]])
    with pytest.raises(AssertionError, match=r"\(clip %d, .*group g = %d," % (second[0] // S, t)):
        e.check(_as_left_by(e, _want(o, clip=clip)))


def test_the_previous_groups_residual_is_seen():
    o = _operands()
    e = _expect(_want(o))
    g = CHUNKS[0] + 1
    res = o["res"].clone()
    res[_rows_of(g)] = o["res"][_rows_of(g - 1)]
    with pytest.raises(AssertionError, match=r"group g = %d," % g):
        e.check(_as_left_by(e, _want(o, res=res)))


@pytest.mark.parametrize("filled", [False, True], ids=["canary_shows", "old_values_show"])
@pytest.mark.parametrize("n", CHUNKS)
def test_an_unwritten_ragged_last_trip_is_seen(n, filled):
    e = _expect(_want(_operands()), filled)
    first = NGROUPS // n * n                                          # first group of the last trip
    bad = e.ideal()
    e.rows(bad)[first * GVOX:] = e.rows(e.before)[first * GVOX:]
    assert filled or bool((e.rows(bad)[first * GVOX:] == U.CANARY).all())
    with pytest.raises(AssertionError, match=r"trip g // nchunks = .*%d of nchunks %d" % (NGROUPS // n, n)):
        e.check(bad)


def test_one_bf16_ulp_in_one_channel_passes_the_tolerance_and_fails_the_bit_check():
    e = _expect(_want(_operands()))
    ideal, bad = e.ideal(), e.ideal()
    m = (2 * CHUNKS[1] + 3) * GVOX + 5
    cell = e.rows(bad)[m, C_OFF + 3:C_OFF + 4]
    cell.copy_((cell.view(torch.int16) + 1).view(torch.bfloat16))
    assert not torch.equal(ideal, bad)
    e.check(bad)
    with pytest.raises(AssertionError, match=r"differ in 1 elements of 1 voxels; first at voxel %d .*column %d" % (m, C_OFF + 3)):
        e.check_trips(ideal, bad)
    with pytest.raises(AssertionError, match="differ in 1 elements"):
        e.check_trips(bad, ideal)


def test_a_non_zero_padding_channel_a_touched_canary_and_a_touched_neighbour_slice_are_seen():
    e = _expect(_want(_operands()))
    assert e.written == 16 and COUT < e.written
    bad = e.ideal()
    e.rows(bad)[M - 1, C_OFF + COUT] = 2.0 ** -10
    with pytest.raises(AssertionError, match=r"padding channels are not zero, first at voxel %d " % (M - 1)):
        e.check(bad)
    for where in (0, U.STREAM_GUARD - 1, U.STREAM_GUARD + M * LD, 2 * U.STREAM_GUARD + M * LD - 1):
        bad = e.ideal()
        bad[where] = 0.5
        with pytest.raises(AssertionError, match="canary elements"):
            e.check(bad)
        with pytest.raises(AssertionError, match="canaries differ"):
            e.check_trips(e.ideal(), bad)
    for c in (C_OFF - 1, C_OFF + e.written, LD - 1):
        bad = e.ideal()
        e.rows(bad)[3, c] += 1.0
        with pytest.raises(AssertionError, match="does not own"):
            e.check(bad)
        with pytest.raises(AssertionError, match="differ in 1 elements"):
            e.check_trips(e.ideal(), bad)


def test_two_outputs_per_mfma_column_are_placed_by_their_column():
    """stem_c4_kernel<1, 4, 2>: a group is 256 columns of two W-adjacent outputs; `unit` maps a voxel to its column."""
    Wo, rows = 5, 40
    unit = (torch.arange(rows * Wo) // Wo) * 3 + (torch.arange(rows * Wo) % Wo) // 2
    e = U.StreamExpect(torch.zeros(rows * Wo, 8), U.stream_buf(rows * Wo, 8, torch.bfloat16), 8, rows * Wo, 16, [2, 3],
                       U.TOL[torch.bfloat16], unit=unit)
    assert e.group_of(0) == 0 and e.group_of(4) == 0 and e.group_of(5 * Wo) == 0 and e.group_of(5 * Wo + 2) == 1
    assert "group g = 7, trip g // nchunks = 3 of nchunks 2, 2 of nchunks 3" in e.where(39 * Wo + 4)


def test_the_tap_conv_references_agree_with_conv3d_and_round_the_inner_tensor():
    import torch.nn.functional as F
    x = U.randn((2, 5, 7, 6, 8), 21).to(torch.bfloat16)
    w = U.randn((12, 8, 3, 3, 3), 22, 216 ** -0.5).to(torch.bfloat16)
    sc, sh = U.randn((12,), 23, 0.2, 1.0), U.randn((12,), 24)
    got = U.ref_tap_conv(x, w, (2, 1, 2), (1, 1, 1), sc, sh, L.ACT_RELU)
    ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), stride=(2, 1, 2), padding=(1, 1, 1)).permute(0, 2, 3, 4, 1)
    ref = (ref * sc.double() + sh.double()).clamp_min(0)
    assert got.shape == ref.shape == (2, 3, 7, 3, 12) and (got - ref).abs().max().item() <= 1e-12
    w2 = U.randn((20, 12), 25, 12 ** -0.5).to(torch.bfloat16)
    s2, h2 = U.randn((20,), 26, 0.2, 1.0), U.randn((20,), 27)
    res = U.randn((got.numel() // 12, 20), 28).to(torch.bfloat16)
    pair = U.ref_tap_pw2(x, w, (2, 1, 2), (1, 1, 1), sc, sh, L.ACT_RELU, w2, s2, h2, L.ACT_RELU, res=res)
    mid = ref.to(torch.bfloat16).double().reshape(-1, 12)
    want = ((mid @ w2.double().t()) * s2.double() + h2.double() + res.double()).clamp_min(0)
    assert (pair - want).abs().max().item() <= 1e-12
    unrounded = ((ref.reshape(-1, 12) @ w2.double().t()) * s2.double() + h2.double() + res.double()).clamp_min(0)
    assert (pair - unrounded).abs().max().item() > 1e-6               # the rounding point is part of the reference


# ------------------------------------------------------------------ the launcher text the GPU cases' shapes rest on
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorchvideo_amd", "csrc")
PINNED = {
    "pv_pwconv.hip": [
        "return occ > 4 ? 4 : occ;",
        "const long resident = 256 * per_cu;",
        "long nchunks = pv_ceil_div(resident, nsplit);",
        "const long resident2 = 256 * per_cu2;",
        "long nchunks2 = pv_ceil_div(resident2, nsplit2);",
        "const long ngroups = pv_ceil_div(M, 4 * TM * 16);",
        "const int nsplit = (int)pv_ceil_div(pv_round_up(d.cout, 8), NT * 16);",
        "int NT = cout_p8 <= 32 ? 2 : (cout_p8 <= 64 ? 4 : 8);",
        "if (NT == 2) return launch_pw<2, 2>(d, ksteps, lds, s);",
        "if (NT == 4) return launch_pw<4, 2>(d, ksteps, lds, s);",
        "return launch_pw<8, 1>(d, ksteps, lds, s);",
        "if (d.a_gate && S_out < 64) return PV_ERR_UNSUPPORTED;",
    ],
    "pv_lateral.hip": [
        "constexpr int kLatThreads = 512;",
        "per_cu = per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu);",
        "long nchunks = pv_ceil_div(256 * per_cu, nsplit);",
        "const long ngroups = pv_ceil_div(M, (kLatThreads / 64) * TM * 16);",
        "const int nsplit = (int)pv_ceil_div(pv_round_up(d.cout, 8), NT * 16);",
        "int nt = cout_p8 <= 32 ? 2 : (cout_p8 <= 64 ? 4 : 8);",
        "while (nt > 2 && lds_of(nt) > 120 * 1024) nt >>= 1;",
        "if (nt == 2) return launch_lateral<2, 2>(d, ksteps, lds, xcont, s);",
        "if (nt == 4) return launch_lateral<4, 2>(d, ksteps, lds, xcont, s);",
        "return launch_lateral<8, 1>(d, ksteps, lds, xcont, s);",
        "if (nt == 2) return launch_lateral<2, 2, true>(d, ksteps, lds, xcont, s);",
        "return launch_lateral<4, 2, true>(d, ksteps, lds, xcont, s);",
    ],
    "pv_stem.hip": [
        "const long gx = ngroups < 4096 ? ngroups : 4096;",
        "const long ngroups = pv_ceil_div(M, 4 * TM * 16);",
        "const long M = (long)d.B * d.To * d.Ho * ((d.Wo + JP - 1) / JP);",
        "if (jp == 2) return launch_stem<1, 4, 2>(d, ksteps, s);",
        "if (cout_p8 <= 32) return launch_stem<2, 4>(d, ksteps, s);",
    ],
}


@pytest.mark.parametrize("unit", sorted(PINNED))
def test_the_launchers_still_size_their_grids_as_the_multi_trip_shapes_assume(unit):
    """tests/test_gpu_stream_kernels.py derives its group counts from these lines (it quotes them).  If one changes, a grid was
    resized: revisit those shapes, or the cases quietly go back to one trip of the loop."""
    with open(os.path.join(CSRC, unit)) as f:
        text = f.read()
    for line in PINNED[unit]:
        assert text.count(line) >= 1, "%s no longer says `%s`" % (unit, line)
