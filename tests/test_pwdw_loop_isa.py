"""Build-time check of the plane loop of pwdw_plane_kernel (conv_a + depthwise conv_b of X3D's squeeze-excitation blocks).

The kernel is bound by vector issue, so the instruction count of the loop over input planes is its cost.  This test compiles
pv_pwdw.hip to gfx950 assembly (hipcc cross-compiles without a GPU) and looks at the plane loops of the four instantiations X3D
runs, <S, NW, KS, ACT> = <2,4,1,0> (res2.0, res3.0), <2,4,2,0> (res4.0), <1,4,1,0> (res2.2), <1,4,2,0> (res3.2, res3.4).

Which loops: every loop (a label up to a backward branch to it) that holds MFMAs, a workgroup barrier and buffer stores; loops
that overlap are one region, and a region counts as a plane loop if it reads a whole plane of stencil inputs (3 rows of NC
columns) from LDS per barrier.  The kernel has one plane loop per value of its two launch-constant flags (act_a is ReLU, squeeze
sums wanted), each walking two planes per trip.  The start of a clip is peeled off in front of them and block placement lays it
out as textual loops too: the first plane alone stores nothing (no output plane is complete yet), and at stride 1 the first
trip (three column-tile phases, two planes of stencil, one output plane) is such a span; neither is a plane loop.  Counts are per
plane: the region's count over the number of barriers in it.  The first two points hold in every region, the others in every
plane loop:
  * no v_accvgpr_read / v_accvgpr_write: conv_a's MFMAs write arithmetic registers;
  * at most MT v_cndmask_b32 (MT = the wave's 16-voxel column tiles: what a halo mask would cost; the mask is folded into the
    LDS address, so the launch-constant flags and the mask cost no select at all);
  * fewer v_add_u32 + v_lshl_add_u32 than buffer accesses: the plane offset of a buffer access is its scalar offset, the K step
    its immediate, and an LDS access takes its buffer and row as immediates;
  * the MFMAs, LDS dwords read and buffer loads of the parent commit, and its buffer stores: the NW = 4 of the output plane
    that an input plane completes, and at stride 2 the 4 more of the place that writes the clip's last output plane (the parent
    had that second place in both loops; at stride 1 it now stands once behind the walk); at least 108 packed FMAs (the 27 taps
    of NW = 4 outputs);
  * at most as many instructions as the parent's loop less its accumulator reads and less its selects beyond MT.
And per kernel: no scratch, and no more registers (arithmetic + accumulator) than the parent commit used.
PWDW_ISA_DUMP=<file> appends the counts of every region to <file> (the figures of profiles/r28/isa_vs_parent.md)."""
import os
import re
from collections import Counter

import pytest

from test_prologue_isa import _LOAD, _asm, kernel_lines, kernel_meta, loops

# Per plane, at the parent commit: all instructions of the plane loop, its v_accvgpr_read_b32, v_cndmask_b32 and MFMAs, the
# dwords it reads from LDS, its buffer loads and stores; registers (arithmetic + accumulator) of the kernel.
PARENT = {
    (2, 1): dict(total=471, acc=40, cnd=44, mfma=10, lds=27, loads=5, stores=8, regs=246),
    (2, 2): dict(total=460, acc=40, cnd=44, mfma=20, lds=27, loads=10, stores=8, regs=276),
    (1, 1): dict(total=305, acc=16, cnd=21, mfma=4, lds=18, loads=2, stores=8, regs=214),
    (1, 2): dict(total=297, acc=16, cnd=20, mfma=8, lds=18, loads=4, stores=8, regs=240),
}
FORMS = sorted(PARENT)


def column_tiles(S, NW=4):
    """MT of the kernel: 16-voxel column tiles of the (3 S + 3) x ((4 NW - 1) S + 3) halo plane, per wave (4 waves)."""
    tiles = ((3 * S + 3) * ((4 * NW - 1) * S + 3) + 15) // 16
    return (tiles + 3) // 4


def frag(S, KS):
    return "pwdw_plane_kernelILi%dELi4ELi%dELi0EE" % (S, KS)


@pytest.fixture(scope="module")
def pwdw_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_pwdw")


def plane_loops(asm, S, KS, start_up_too=False):
    """Per-plane counts of every plane-loop region of the instantiation (start_up_too: of every region)."""
    lines = kernel_lines(asm, frag(S, KS))
    holds = lambda a, b, pat: any(re.match(r"^\s+" + pat, l) for l in lines[a:b + 1])
    spans = sorted((a, b) for a, b in loops(lines) if holds(a, b, "v_mfma") and holds(a, b, "s_barrier") and holds(a, b, "buffer_store"))
    # innermost such loops, each grown by the loops that overlap it without enclosing it (a second back edge of the same walk);
    # a span that encloses a whole region is block placement around the flag dispatch, not a plane loop
    regions = [[a, b] for a, b in spans if not any((c, d) != (a, b) and a <= c and d <= b for c, d in spans)]
    grown = True
    while grown:
        grown = False
        for a, b in spans:
            for r in regions:
                if a <= r[1] and r[0] <= b and not (a <= r[0] and r[1] <= b) and not (r[0] <= a and b <= r[1]):
                    r[0], r[1], grown = min(r[0], a), max(r[1], b), True
    regions = sorted(set(map(tuple, regions)))
    assert all(b < c for (_, b), (c, _) in zip(regions, regions[1:])), regions
    out = []
    for a, b in regions:
        ops = [l.split()[0] for l in lines[a:b + 1] if re.match(r"^\s+[a-z]", l)]
        c = Counter(ops)
        n = lambda *prefixes: sum(v for k, v in c.items() if k.startswith(prefixes))
        planes = c["s_barrier"]
        per = lambda v: v / float(planes)
        out.append(dict(planes=planes, total=per(len(ops)), acc=per(n("v_accvgpr_")), cnd=per(n("v_cndmask_b32")),
                        adds=per(n("v_add_u32", "v_lshl_add_u32")), mfma=per(n("v_mfma")), pk_fma=per(n("v_pk_fma_f32")),
                        lds=per(n("ds_read_b32") + 2 * n("ds_read2_b32", "ds_read2st64_b32")),
                        lds_other=n("ds_read") - n("ds_read_b32", "ds_read2_b32", "ds_read2st64_b32"),
                        loads=per(sum(1 for l in lines[a:b + 1] if _LOAD.match(l))), stores=per(n("buffer_store")),
                        relu=n("v_pk_max_i16") > 0))
    if not start_up_too:
        out = [r for r in out if r["lds"] == 3 * (3 * S + 3)]        # NC = (NW - 1) S + 3 columns, NW = 4
    dump = os.environ.get("PWDW_ISA_DUMP")
    if dump:
        meta = kernel_meta(asm, frag(S, KS))
        with open(dump, "a") as f:
            f.write("<%d,4,%d,0>: registers %d, scratch %d\n" % (S, KS, meta["vgpr_count"], meta["private_segment_fixed_size"]))
            for r in out:
                f.write("  plane loop (%(planes)d planes per trip, act_a ReLU %(relu)s), per plane: instructions %(total)g, packed FMAs "
                        "%(pk_fma)g, accumulator moves %(acc)g, v_cndmask %(cnd)g, v_add_u32 + v_lshl_add_u32 %(adds)g, MFMAs %(mfma)g, "
                        "LDS dwords read %(lds)g, buffer loads %(loads)g, buffer stores %(stores)g\n" % r)
    return out


@pytest.mark.parametrize("S,KS", FORMS)
def test_one_plane_loop_per_flag_pair(pwdw_asm, S, KS):
    regions = plane_loops(pwdw_asm, S, KS)
    print(regions)
    assert len(regions) == 4, regions
    assert sorted(r["relu"] for r in regions) == [False, False, True, True], regions


@pytest.mark.parametrize("S,KS", FORMS)
def test_conv_a_results_stay_in_arithmetic_registers(pwdw_asm, S, KS):
    for r in plane_loops(pwdw_asm, S, KS, start_up_too=True):
        assert r["acc"] == 0, r


@pytest.mark.parametrize("S,KS", FORMS)
def test_launch_constant_flags_and_halo_mask_cost_no_select_per_value(pwdw_asm, S, KS):
    for r in plane_loops(pwdw_asm, S, KS, start_up_too=True):
        assert r["cnd"] <= column_tiles(S), r


@pytest.mark.parametrize("S,KS", FORMS)
def test_plane_offsets_are_not_added_on_the_vector_pipe(pwdw_asm, S, KS):
    for r in plane_loops(pwdw_asm, S, KS):
        assert r["adds"] < r["loads"] + r["stores"], r


@pytest.mark.parametrize("S,KS", FORMS)
def test_necessary_work_is_the_parents(pwdw_asm, S, KS):
    want = PARENT[S, KS]
    for r in plane_loops(pwdw_asm, S, KS):
        assert r["lds_other"] == 0, r
        stores = want["stores"] if S == 2 else want["stores"] - 4      # stride 1: the clip's last plane is stored behind the walk
        assert (r["mfma"], r["lds"], r["loads"], r["stores"]) == (want["mfma"], want["lds"], want["loads"], stores), (r, want)
        assert r["pk_fma"] >= 108, r


@pytest.mark.parametrize("S,KS", FORMS)
def test_plane_loop_is_shorter_than_the_parents_by_what_was_wasted(pwdw_asm, S, KS):
    want = PARENT[S, KS]
    bound = want["total"] - want["acc"] - (want["cnd"] - column_tiles(S))
    for r in plane_loops(pwdw_asm, S, KS):
        assert r["total"] <= bound, (r, bound)


def _vregs(line):
    out = set(int(x) for x in re.findall(r"\bv(\d+)\b", line))
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", line):
        out.update(range(int(a), int(b) + 1))
    return out


def test_no_result_of_an_inline_mfma_is_touched_within_its_eight_wait_states(pwdw_asm):
    """The MFMAs that write arithmetic registers are inline assembly, which the compiler's hazard recogniser does not see: in
    every instantiation that has them (KS <= 2) nothing but the accumulating MFMA of the same chain may name a destination
    register of such an MFMA in the 8 wait states behind it (an instruction is one wait state, s_nop N is N + 1) -- that is
    the distance hipcc itself keeps between this MFMA and a read of its result.  Counted along the text, labels and all."""
    kernels = re.findall(r"^(_ZN\S*pwdw_plane_kernelILi\dELi\dELi(\d)ELi\dE\S*):[^\n]*\n(.*?)s_endpgm", pwdw_asm, re.S | re.M)
    assert len(kernels) == 60
    inline = 0
    for name, ks, body in kernels:
        lines = [l for l in body.split("\n") if re.match(r"^\s+[a-z]", l)]
        for i, l in enumerate(lines):
            m = re.match(r"\s+v_mfma\S+ (v\[(\d+):(\d+)\]),", l)
            if not m:
                continue
            assert int(ks) <= 2, (name, l)
            inline += 1
            dst, waited, j = set(range(int(m.group(2)), int(m.group(3)) + 1)), 0, i + 1
            while waited < 8 and j < len(lines):
                t = lines[j]
                if t.split()[0] == "s_nop":
                    waited += int(t.split()[1]) + 1
                else:
                    same_chain = t.split()[0].startswith("v_mfma") and t.split()[1] == m.group(1) + ","
                    assert same_chain or not (_vregs(t) & dst), (name, l, t, waited)
                    waited += 1
                j += 1
    assert inline > 0


@pytest.mark.parametrize("S,KS", FORMS)
def test_no_scratch_and_no_more_registers_than_the_parent(pwdw_asm, S, KS):
    meta = kernel_meta(pwdw_asm, frag(S, KS))
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["vgpr_count"] <= PARENT[S, KS]["regs"], meta
