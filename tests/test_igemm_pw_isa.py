"""Build-time check of the K loop of conv_igemm_kernel's buffer-addressed pointwise instantiations (bf16, 128 x 128 tiles).

The loop keeps two K tiles in flight in two fixed register sets: while the older set is transformed and written to LDS, the
loads of the younger one must stay outstanding.  The compiler can only leave them outstanding if it can count them, so every
load_global issues the same XCH + WCH = 4 loads with no branch around any of them, and the wait in front of each LDS store
phase comes out as vmcnt(n), n >= 4.  With the loads behind per-chunk tests every one of those waits was vmcnt(0): one memory
round trip per K step (profiles/r22/isa_vs_parent.md).  This test compiles pv_conv.hip to gfx950 assembly (hipcc cross-compiles
without a GPU) and looks at the loop that holds the MFMAs:
  * it holds 2 * 4 vector-memory loads and two LDS store phases, one per barrier;
  * every wait on vmcnt in it leaves at least 4 requests outstanding, and at least one stands in front of each store phase;
  * nothing in it writes the exec mask or branches on it, so no load sits behind an exec-masked branch;
  * the kernel uses no scratch.
IGEMM_ISA_DUMP=<file> appends the counts of every covered kernel to <file> (the figures of profiles/r22)."""
import os
import re

import pytest

from test_prologue_isa import _LOAD, _asm, kernel_lines, kernel_meta, loops

XCH, WCH = 2, 2          # 128 x 32 activation and 128 x 32 weight chunks of 8 over 256 threads
_VMCNT = re.compile(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)")
_EXEC = re.compile(r"^\s+(s_\w+saveexec\w*|v_cmpx\w*|s_cbranch_exec\w*)\b|^\s+s_\w+\s+exec(_lo|_hi)?,")
# <bf16, 128, 128, 2, 2, PW = true, FX>: FX 1 = no operand transform, 2 = gate from LDS + Swish (X3D res5's conv_c)
KERNELS = {"plain": "conv_igemm_kernelIDF16bLi128ELi128ELi2ELi2ELb1ELi1EE", "gated_swish": "conv_igemm_kernelIDF16bLi128ELi128ELi2ELi2ELb1ELi2EE"}


@pytest.fixture(scope="module")
def conv_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_conv")


def k_loop(asm, frag):
    """Lines of the innermost loop that holds MFMAs."""
    lines = kernel_lines(asm, frag)
    with_mfma = [(b - a, a, b) for a, b in loops(lines) if any("v_mfma" in l for l in lines[a:b + 1])]
    assert with_mfma, "%s has no loop with MFMAs" % frag
    _, a, b = min(with_mfma)
    return lines[a:b + 1]


def k_loop_counts(asm, frag):
    body = k_loop(asm, frag)
    ops = [l.split()[0] for l in body if re.match(r"^\s+[a-z]", l)]
    phases, cur = [], None          # per barrier-delimited stretch with LDS stores: the vmcnt waits in front of its last store
    for l in body:
        if re.match(r"^\s+s_barrier\b", l):
            if cur is not None and cur["stores"]:
                phases.append(cur["waits"])
            cur = None
            continue
        cur = cur or {"stores": 0, "waits": [], "pending": []}
        m = _VMCNT.match(l)
        if m:
            cur["pending"].append(int(m.group(1)))
        elif re.match(r"^\s+ds_write", l):
            cur["stores"] += 1
            cur["waits"] += cur["pending"]
            cur["pending"] = []
    meta = kernel_meta(asm, frag)
    counts = dict(kernel=frag, loads=sum(1 for l in body if _LOAD.match(l)), mfma=sum(1 for o in ops if o.startswith("v_mfma")),
                  valu=sum(1 for o in ops if o.startswith("v_") and not o.startswith("v_mfma")),
                  vmcnt=[int(m.group(1)) for m in map(_VMCNT.match, body) if m], store_phase_waits=phases,
                  exec_writes=sum(1 for l in body if _EXEC.match(l)), scratch=meta["private_segment_fixed_size"], vgprs=meta["vgpr_count"])
    dump = os.environ.get("IGEMM_ISA_DUMP")
    if dump:
        with open(dump, "a") as f:
            f.write("%(kernel)s: K loop (two steps) loads %(loads)d, MFMAs %(mfma)d, VALU %(valu)d, vmcnt waits %(vmcnt)s, waits per "
                    "store phase %(store_phase_waits)s, exec writes %(exec_writes)d; scratch %(scratch)d, vgprs %(vgprs)d\n" % counts)
    return counts


@pytest.mark.parametrize("form", list(KERNELS))
def test_k_loop_waits_leave_the_younger_tile_in_flight(conv_asm, form):
    c = k_loop_counts(conv_asm, KERNELS[form])
    print(c)
    assert c["loads"] == 2 * (XCH + WCH), c
    assert len(c["store_phase_waits"]) == 2, c
    assert all(w and max(w) >= XCH + WCH for w in c["store_phase_waits"]), c
    assert c["vmcnt"] and min(c["vmcnt"]) >= XCH + WCH, c


@pytest.mark.parametrize("form", list(KERNELS))
def test_k_loop_has_no_load_behind_an_exec_masked_branch(conv_asm, form):
    c = k_loop_counts(conv_asm, KERNELS[form])
    assert c["exec_writes"] == 0, c


@pytest.mark.parametrize("form", list(KERNELS))
def test_kernel_uses_no_scratch(conv_asm, form):
    assert k_loop_counts(conv_asm, KERNELS[form])["scratch"] == 0
