"""Build-time check of the stride-2 plane walk of pwdw_plane_kernel: two input planes in flight, and a wait that says so.

<2, 4, 1, 0> (res2.0 and res3.0 of X3D-M, the most expensive launch of the step) requests plane p + 2 in front of the stencil of
plane p and converts plane p + 1 from the operand set requested one plane earlier.  That only overlaps anything if the wait in
front of a plane's conv_a is a COUNTED one: vector-memory operations retire in order, so `s_waitcnt vmcnt(N)` in front of the
first MFMA of a plane must leave at least the MT = 5 loads of the younger plane outstanding (N >= 5).  N = 0 -- what the compiler
emits when a load site stands behind a branch, since it must assume the loads were skipped -- waits for the plane just
requested as well, and the second operand set buys nothing.  This test compiles pv_pwdw.hip to gfx950 assembly (hipcc
cross-compiles without a GPU) and reads, in each of the four plane loops (one per pair of the launch-constant flags, two planes
per trip; found as tests/test_pwdw_loop_isa.py finds them):
  * per plane (a span that ends in a workgroup barrier): 5 buffer loads, all of them ahead of the plane's first MFMA;
  * the last wait on vmcnt in front of that first MFMA: its operand is at least 5.
And the registers, which are what this form lives on: the kernel holds 2 workgroups of 4 waves per CU only up to 256 registers
(arithmetic + accumulator) per lane.  <2, 4, 1, 0> carries a second operand set of 20 registers and must stay within 256 with
no accumulator registers and no scratch (tests/test_pwdw_loop_isa.py holds it to the parent's 246); <2, 4, 2, 0> (res4.0) keeps
one plane in flight precisely because the set would push it past 256 and cost the second wave per SIMD, and must stay within
256 without scratch too.  Instructions named here: MFMA, buffer load and store, s_waitcnt, s_barrier -- the ones counted."""
import re

import pytest

from test_prologue_isa import _LOAD, _asm, kernel_lines, kernel_meta, loops

MT = 5      # 16-voxel column tiles of the 9 x 33 halo plane per wave = buffer loads per plane at KS = 1


def frag(KS):
    return "pwdw_plane_kernelILi2ELi4ELi%dELi0EE" % KS


@pytest.fixture(scope="module")
def pwdw_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_pwdw")


def _is(line, pat):
    return re.match(r"^\s+" + pat, line) is not None


def plane_loop_spans(lines):
    """(first, last) line of every plane loop: loops that hold MFMAs, a barrier and buffer stores; the innermost of them, each
    grown by the loops that overlap it without enclosing it (the second back edge of a two-plane trip)."""
    holds = lambda a, b, pat: any(_is(l, pat) for l in lines[a:b + 1])
    spans = sorted((a, b) for a, b in loops(lines) if holds(a, b, "v_mfma") and holds(a, b, "s_barrier") and holds(a, b, "buffer_store"))
    regions = [[a, b] for a, b in spans if not any((c, d) != (a, b) and a <= c and d <= b for c, d in spans)]
    grown = True
    while grown:
        grown = False
        for a, b in spans:
            for r in regions:
                if a <= r[1] and r[0] <= b and not (a <= r[0] and r[1] <= b) and not (r[0] <= a and b <= r[1]):
                    r[0], r[1], grown = min(r[0], a), max(r[1], b), True
    return sorted(set(map(tuple, regions)))


def planes_of(lines, a, b):
    """The planes of a loop region, each a list of lines that ends in its barrier, in loop order: the region is rotated so
    that it starts behind a barrier (the text of a loop may begin in the middle of a plane)."""
    body = lines[a:b + 1]
    bars = [i for i, l in enumerate(body) if _is(l, r"s_barrier\b")]
    assert bars
    rot = body[bars[-1] + 1:] + body[:bars[-1] + 1]
    out, cur = [], []
    for l in rot:
        cur.append(l)
        if _is(l, r"s_barrier\b"):
            out.append(cur)
            cur = []
    assert not cur
    return [p for p in out if any(_is(l, "v_mfma") for l in p)]


def test_every_plane_loop_keeps_the_younger_planes_loads_outstanding_across_conv_a(pwdw_asm):
    lines = kernel_lines(pwdw_asm, frag(1))
    regions = plane_loop_spans(lines)
    assert len(regions) == 4, regions
    seen = 0
    for a, b in regions:
        planes = planes_of(lines, a, b)
        assert planes, (a, b)       # block placement may put one plane of a trip outside the textual loop: 1 or 2
        for plane in planes:
            first = next(i for i, l in enumerate(plane) if _is(l, "v_mfma"))
            loads = [i for i, l in enumerate(plane) if _LOAD.match(l)]
            waits = [int(m.group(1)) for l in plane[:first] for m in [re.match(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)", l)] if m]
            print("lines %d-%d: %d loads, %d ahead of the first MFMA, vmcnt waits in front of it %s" % (
                a, b, len(loads), sum(1 for i in loads if i < first), waits))
            assert len(loads) == MT and all(i < first for i in loads), (a, b, loads, first)
            assert waits, (a, b)
            assert waits[-1] >= MT, (a, b, waits)
            assert 0 not in waits, (a, b, waits)
            seen += 1
    assert 4 <= seen <= 8, seen


def test_deep_form_stays_within_two_waves_per_simd(pwdw_asm):
    meta = kernel_meta(pwdw_asm, frag(1))
    print(meta)
    assert meta["vgpr_count"] <= 256, meta
    assert meta.get("agpr_count", 0) == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta


def test_res4_form_keeps_its_second_wave(pwdw_asm):
    meta = kernel_meta(pwdw_asm, frag(2))
    print(meta)
    assert meta["vgpr_count"] <= 256, meta
    assert meta["private_segment_fixed_size"] == 0, meta
