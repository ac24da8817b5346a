"""Build-time check of the kernels' start-up code (the part before the first workgroup barrier): every request goes out
before the first wait.

A staging loop written as `lds[i] = global[i]` compiles to load / s_waitcnt vmcnt(0) / ds_write / branch: one memory round
trip per iteration, 14 of them for the filter slab of the res4 conv_c, before the kernel has asked for a single activation.
The kernels checked here issue their whole start-up batch (filter slab, BatchNorm tables, the first group's operands, the
squeeze-excitation gate rows) and wait once.  This test compiles the files to gfx950 assembly (hipcc cross-compiles without a
GPU) and looks at what the compiler emitted -- loads, waits, barriers and the scratch metadata, nothing else:
  * between the kernel's entry and its first s_barrier no loop body (a label up to a backward branch to it) holds both a
    vector-memory load and a wait on vmcnt;
  * at most 3 waits on vmcnt stand before that barrier;
  * the kernel uses no scratch.
PROLOGUE_ISA_DUMP=<file> appends the counts of every covered kernel to <file> (the figures of profiles/r20)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_LOAD = re.compile(r"^\s+(global_load_|buffer_load_|flat_load_|scratch_load_)")
_VMWAIT = re.compile(r"^\s+s_waitcnt\b.*vmcnt\(")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)")


def _asm(tmp_path_factory, name):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    out = str(tmp_path_factory.mktemp("isa_" + name) / (name + ".s"))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "pytorchvideo_amd", "csrc"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(ROOT, "pytorchvideo_amd", "csrc", name + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope="module")
def pwconv_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_pwconv")


@pytest.fixture(scope="module")
def lateral_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_lateral")


@pytest.fixture(scope="module")
def block_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "pv_block")


def kernel_lines(asm, frag):
    m = re.search(r"^(_ZN\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % re.escape(frag), asm, re.S | re.M)
    assert m, "kernel %s not found in the assembly" % frag
    return m.group(2).split("\n")


def kernel_meta(asm, frag):
    m = re.search(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % re.escape(frag), asm, re.S)
    assert m, "metadata of %s not found" % frag
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}


def loops(lines):
    """(first, last) line index of every loop body: a label up to a backward branch to that label."""
    seen, out = {}, []
    for i, l in enumerate(lines):
        m = _LABEL.match(l)
        if m:
            seen[m.group(1)] = i
            continue
        m = _BRANCH.match(l)
        if m and m.group(1) in seen:
            out.append((seen[m.group(1)], i))
    return out


def prologue_counts(asm, frag):
    lines = kernel_lines(asm, frag)
    bar = next((i for i, l in enumerate(lines) if re.match(r"^\s+s_barrier\b", l)), None)
    assert bar is not None, "%s has no barrier" % frag
    pro = lines[:bar]
    waiting_loops = sum(1 for a, b in loops(pro)
                        if any(_LOAD.match(l) for l in pro[a:b + 1]) and any(_VMWAIT.match(l) for l in pro[a:b + 1]))
    meta = kernel_meta(asm, frag)
    counts = dict(kernel=frag, loads=sum(1 for l in pro if _LOAD.match(l)), vmcnt_waits=sum(1 for l in pro if _VMWAIT.match(l)),
                  loops_that_load_and_wait=waiting_loops, scratch=meta["private_segment_fixed_size"], vgprs=meta["vgpr_count"])
    dump = os.environ.get("PROLOGUE_ISA_DUMP")
    if dump:
        with open(dump, "a") as f:
            f.write("%(kernel)s: loads %(loads)d, vmcnt waits %(vmcnt_waits)d, loops that load and wait "
                    "%(loops_that_load_and_wait)d, scratch %(scratch)d, vgprs %(vgprs)d\n" % counts)
    return counts


def check_prologue(asm, frag):
    c = prologue_counts(asm, frag)
    print(c)
    assert c["loops_that_load_and_wait"] == 0, c
    assert c["vmcnt_waits"] <= 3, c
    assert c["scratch"] == 0, c


PW = ["pw_stream_kernelILi8ELi1ELb1ELi7ELb0ELb0E", "pw_stream_kernelILi2ELi2ELb1ELi3ELb0ELb1E",
      "pw_stream_kernelILi4ELi2ELb1ELi4ELb0ELb0E", "pw_stream_kernelILi8ELi1ELb0ELi3ELb0ELb0E"]


@pytest.mark.parametrize("frag", PW)
def test_pw_stream_start_up_requests_everything_before_its_first_wait(pwconv_asm, frag):
    check_prologue(pwconv_asm, frag)


def test_tap_stream_start_up_requests_everything_before_its_first_wait(lateral_asm):
    check_prologue(lateral_asm, "tap_stream_kernelILi8ELi1ELb0EE")


# <CP, KSA, COUTP, PAIR, SEGS, ACT_B, MODE, ABL>: res2, res3, res4; the whole block with ReLU behind conv_b (2, 0, 0) and the
# squeeze-excitation form that stops behind conv_b (0, 1, 0)
BLOCK = ["bottleneck_block_kernelILi%sELb%dELi%dELi%dELi%dELi0EE" % (g, pair, segs, act_b, mode)
         for g, pair, segs in (("64ELi1ELi32", 0, 2), ("128ELi2ELi48", 1, 2), ("224ELi3ELi96", 1, 1))
         for act_b, mode in ((0, 1), (2, 0))]


@pytest.mark.parametrize("frag", BLOCK)
def test_bottleneck_block_start_up_requests_everything_before_its_first_wait(block_asm, frag):
    """(The res4 form that stops behind conv_b, <224, 3, 96, true, 1, 0, 1, 0>, had 64 bytes of scratch before this test
    existed: 15 registers of its stencil waves; profiles/r20/isa_counts.md.)"""
    check_prologue(block_asm, frag)


def test_gate_refresh_of_the_res4_conv_c_issues_its_loads_back_to_back(pwconv_asm):
    """The squeeze-excitation gate rows are the kernel's only single-dword global loads behind the barrier (cin = 216: 7 per lane
    for the two clips a wave tile can touch).  They must stand as runs of 7 with no wait, label or branch in between."""
    lines = kernel_lines(pwconv_asm, PW[0])
    bar = next(i for i, l in enumerate(lines) if re.match(r"^\s+s_barrier\b", l))
    runs, run = [], 0
    for l in lines[bar:]:
        if re.match(r"^\s+global_load_dword\s", l):
            run += 1
        elif run and (_VMWAIT.match(l) or _LABEL.match(l) or _BRANCH.match(l)):
            runs.append(run)
            run = 0
    if run:
        runs.append(run)
    print("gate load runs behind the barrier:", runs)
    assert runs and all(r >= 7 for r in runs), runs
