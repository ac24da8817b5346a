"""The teacher-forced per-block gate (tools/parity_blocks.py) at the batches whose kernels it is meant to judge.

The library picks kernels by tile count, i.e. by batch: at one clip SlowFast-R50's res4 / res5 GEMM layers run on the older
128 x 128 kernel and MViT-B's stage-3 pooling convs on the fused pool + LayerNorm kernel, while the plans bench.py times (8 and 4
clips per sub-batch) run them on the eight-phase kernels and on the plane-streaming kernel + layernorm16.  So the batch-1 gate
of tests/test_gpu_full_geometry.py judges other kernels than the timed ones.  Here:

1. the same gate at the bench's per-branch batch (16 / 16 / 8 / 4 clips): every block, every ROW (max|d| over the row / max|oracle
   block output| over the row; the block's figure is its worst row, named), with the sites that lie between the blocks of the
   full plan (lateral fusions, MViT's prologue / head / pre-written norm1) judged as well;
2. coverage: every op of the bench form's sub-plan 0 has, by kernel symbol AND geometry key, a counterpart among the ops the gate
   ran -- which is what makes (1) mean what its name says, and fails the day a routing change moves a bench layer to a kernel
   the gate does not reach;
3. the premise: for SlowFast-R50 and MViT-B the route at the branch batch differs from the batch-1 route;
4. defect injection at the branch batch in a layer an eight-phase kernel serves at 8 clips and not at 1;
5. the same gate OFF the bench shapes (2, 3, the whole bench batch in one plan, SlowFast 17), where the routing thresholds
   were not fitted, and one end-to-end case per workload at an odd batch split raggedly over two sub-batch plans.

Bounds: the constants of tests/test_gpu_full_geometry.py as they stand (BLOCK_BF16_TOL / BLOCK_BF16_TOL_STRESS: a kernel's
per-element error has no reason to depend on the batch, and their x 1.3 is the margin for seeing more clips).  A per-(workload,
batch) exception is allowed ONLY as 1.3 x a reference-only floor (the oracle under bf16 storage emulation against the fp32 oracle,
no kernel involved) that is itself at or above the bound: FLOOR_BOUNDS below.  Nothing here is derived from the deploy form's output.

PV_PARITY_DUMP=<file> keeps every case's figures, PV_ROUTE_DUMP=<file> every case's route (profiles/r8/).
"""
import collections
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import test_gpu_full_geometry as G  # noqa: E402  (the project's constants and the bench-form assertions, unchanged)

WORKLOADS4 = G.WORKLOADS4
EXPECT_BLOCKS = {"x3d_m": 26, "x3d_l": 55, "slowfast_r50": 32, "mvit_b_32x3": 16}
# batches the routing thresholds were NOT fitted to: 2 and 3 (small; 3 is odd: a last tile that is partly another clip's or partly
# empty), the whole bench batch in one plan, and for SlowFast one clip more (17: res4 goes from the half-height to the 256 x 256
# kernel there, pv_gemm9.hip: t256 = 136 >= gemm9_min_tiles and th = 272 > 256).  Which decision each of them shows on which
# side: profiles/r8/route_census.md.
OFF_BENCH = [("x3d_m", 2), ("x3d_m", 3), ("x3d_m", 32), ("x3d_l", 2), ("x3d_l", 3), ("x3d_l", 32),
             ("slowfast_r50", 2), ("slowfast_r50", 3), ("slowfast_r50", 16), ("slowfast_r50", 17),
             ("mvit_b_32x3", 2), ("mvit_b_32x3", 3), ("mvit_b_32x3", 8)]
# With every case in the default run this file added more than the parent commit's whole GPU suite takes (157 s), so the largest
# off-bench cases moved under the existing `slow` marker, largest first, until it no longer does (tools/gpu_round.sh runs them;
# durations in profiles/r8/gpu_suite_tail.txt): 51 / 32 / 30 / 30 / 29 s, then MViT-B at 3 and 2 clips (13 / 10 s).  MViT-B's 4 + 3
# ragged end-to-end case and everything at the branch batch stay in the default run.
OFF_BENCH_SLOW = {("x3d_l", 32), ("mvit_b_32x3", 8), ("slowfast_r50", 17), ("x3d_m", 32), ("slowfast_r50", 16),
                  ("mvit_b_32x3", 3), ("mvit_b_32x3", 2)}
# (workload, batch) -> {block: (bound, measured reference-only floor, measured deploy figure)}: 1.3 x a bf16-storage floor that is
# itself at or above the project's bound; every other block of the case stays on the project's constant.
# X3D-L at 32 clips: rows 16 and 17 (clips the 16-clip gate never sees) of blocks.3.res_blocks.0 read 7.849e-3 / 7.832e-3 where bf16
# storage ALONE -- the oracle under storage emulation, no kernel -- reads the same 7.849e-3 / 7.832e-3 (the worst element is an
# output rounding both share), above BLOCK_BF16_TOL's 6.8e-3 (profiles/r8/parity_blocks_batches.jsonl).  1.3 x 7.849e-3:
FLOOR_BOUNDS = {("x3d_l", 32): {"blocks.3.res_blocks.0": (1.02e-2, 7.849e-3, 7.849e-3)}}
# Ops of the bench plan that need no counterpart in the gate: kernel symbol -> reason.  Only kernels without arithmetic (ingest,
# egress, layout copies, joins) may be listed; nothing that multiplies, accumulates, normalises, pools or applies softmax.
EXCUSED_KERNELS = {}

_GATE = {}


def _branch_batch(workload):
    from bench import WORKLOADS
    return WORKLOADS[workload]["batch"] // WORKLOADS[workload].get("streams", 1)


def _gate(workload, batch, fill="trained_like", floor=True):
    """Records of parity_blocks.blocks_case(detail=True), computed once per (workload, batch, fill) and test session."""
    key = (workload, batch, fill)
    if key not in _GATE:
        from parity_blocks import blocks_case
        _GATE[key] = blocks_case(workload, fill, batch=batch, detail=True, floor=floor)
        _dump_routes(workload, batch, "gate", [dict(op, unit=r["name"]) for r in _GATE[key] for op in r["route"]])
    return _GATE[key]


def _census(ops):
    return dict(sorted(collections.Counter(op["kernel"] for op in ops).items()))


def _dump_routes(workload, batch, what, ops):
    print("\ncensus %s b=%d (%s): %s" % (workload, batch, what, json.dumps(_census(ops))))
    path = os.environ.get("PV_ROUTE_DUMP")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"workload": workload, "batch": batch, "what": what, "census": _census(ops),
                                "ops": [{k: op[k] for k in ("unit", "label", "kind", "kernel", "geom") if k in op} for op in ops]}) + "\n")


def _assert_gate(workload, batch, recs, tol, what):
    """Every block and every extra site, every row, against `tol`; the worst block and row are printed and kept."""
    blocks = [r for r in recs if not r["extra"]]
    assert len(blocks) >= EXPECT_BLOCKS[workload] and all(len(r["rows"]) == batch for r in recs), (len(blocks), batch)
    worst = max(recs, key=lambda r: r["worst"])
    floor = max(recs, key=lambda r: r.get("floor_worst", 0.0))
    print("\n%s b=%d [%s]: %d blocks + %d sites between them x %d rows teacher-forced; worst %.3e at %s row %d (bf16 storage alone "
          "on that row, no kernel: %.3e); largest storage floor %.3e at %s; bound %.2e" % (
              workload, batch, what, len(blocks), len(recs) - len(blocks), batch, worst["worst"], worst["name"], worst["worst_row"],
              worst["floor_rows"][worst["worst_row"]] if "floor_rows" in worst else float("nan"),
              floor.get("floor_worst", float("nan")), floor["name"], tol))
    G._dump({"workload": workload, "batch": batch, "blocks": len(blocks), "sites": len(recs), "bound": tol,
             "worst": worst["worst"], "worst_block": worst["name"], "worst_row": worst["worst_row"],
             "per_block": {r["name"]: [float("%.3e" % r["worst"]), r["worst_row"], float("%.3e" % r.get("floor_worst", -1.0))] for r in recs}},
            "teacher-forced per block and row, %s" % what)
    own = {k: v[0] for k, v in FLOOR_BOUNDS.get((workload, batch), {}).items()}       # blocks held to 1.3 x their storage floor
    for r in recs:      # an exception lives only as long as its reason: the reference-only floor is at or above the project's bound
        if r["name"] in own:
            assert r["floor_worst"] >= tol and own[r["name"]] <= 1.3 * r["floor_worst"] * 1.005, (r["name"], r["floor_worst"], tol, own)
    bad = [(r["name"], i, "%.3e" % v, "floor %.3e" % (r["floor_rows"][i] if "floor_rows" in r else -1.0))
           for r in recs for i, v in enumerate(r["rows"]) if not v <= own.get(r["name"], tol)]
    assert not bad, "rows above %.2e%s (block, row, figure, bf16-storage floor of the row): %s" % (tol, " / %s" % own if own else "", bad)


def _tol(workload, batch):
    return G.BLOCK_BF16_TOL[workload]


@pytest.mark.parametrize("workload", WORKLOADS4)
def test_every_block_teacher_forced_bf16_at_the_bench_branch_batch(workload):
    batch = _branch_batch(workload)
    assert batch == {"x3d_m": 16, "x3d_l": 16, "slowfast_r50": 8, "mvit_b_32x3": 4}[workload]
    _assert_gate(workload, batch, _gate(workload, batch), _tol(workload, batch), "bench branch batch")


def _unit_kernels(recs):
    """{unit name: [(label without its batch, kernel)]}: the unit's op list, comparable across batches."""
    import re
    strip = lambda s: re.sub(r"\|\d+x", "|", s, count=1)          # "conv_a|8x8x16x16 c1024->256 ..." -> "conv_a|8x16x16 c1024->256 ..."
    out, cur = {}, None
    for r in recs:
        if r["route"]:
            cur = out.setdefault(r["name"], [])
            cur += [(strip(op["label"]), op["kernel"]) for op in r["route"]]
    return out


def _route_changes(workload, batch):
    """[(unit, what changed)] between the batch-1 gate and the gate at `batch`."""
    one, many = _unit_kernels(_gate(workload, 1, floor=False)), _unit_kernels(_gate(workload, batch))
    assert list(one) == list(many)
    changes = []
    for name in one:
        a, b = one[name], many[name]
        if [l for l, _ in a] != [l for l, _ in b]:
            changes.append((name, "op list: %s -> %s" % (sorted(set(a) - set(b)), sorted(set(b) - set(a)))))
        else:
            changes += [(name, "%s: %s -> %s" % (la, ka, kb)) for (la, ka), (_, kb) in zip(a, b) if ka != kb]
    return changes


@pytest.mark.parametrize("workload", WORKLOADS4)
def test_the_block_gate_reaches_every_kernel_the_bench_plan_runs(workload):
    """Sub-plan 0 of the bench form (built as test_north_star_bench_batch_with_bench_streams_every_row builds it), profiled once:
    every op must be matched, by kernel symbol and geometry key, by an op of the per-block runs at the branch batch."""
    from parity_blocks import plan_route
    batch = _branch_batch(workload)
    recs = _gate(workload, batch)
    reached = {(op["kernel"], op["kind"], op["geom"]) for r in recs for op in r["route"]}
    plan = plan_route(workload)
    _dump_routes(workload, batch, "bench plan, sub-plan 0", plan)
    assert len(plan) > 20 and all(op["kernel"] for op in plan), [op["label"] for op in plan if not op["kernel"]]
    missing = [op for op in plan if (op["kernel"], op["kind"], op["geom"]) not in reached]
    excused = [op for op in missing if op["kernel"] in EXCUSED_KERNELS]
    unmatched = [op for op in missing if op["kernel"] not in EXCUSED_KERNELS]
    print("%s b=%d: %d plan ops, %d matched by the gate, %d excused %s, %d unmatched" % (
        workload, batch, len(plan), len(plan) - len(missing), len(excused), sorted({op["kernel"] for op in excused}), len(unmatched)))
    near = lambda op: sorted({g["kernel"] for r in recs for g in r["route"] if g["label"] == op["label"]})
    assert not unmatched, "bench-plan ops the block gate does not reach (label, kernel in the plan, kernels of the gate's ops with that " \
                          "label): %s" % [(op["label"], op["kernel"], near(op)) for op in unmatched]
    # the premise, so that this test cannot rot into a no-op: the batch-1 gate does NOT reach the bench plan's kernels
    changes = _route_changes(workload, batch)
    print("%s: %d route changes between the gate at 1 clip and at %d clips:\n  %s" % (
        workload, len(changes), batch, "\n  ".join("%s | %s" % c for c in changes) or "(none)"))
    if workload in ("slowfast_r50", "mvit_b_32x3"):
        assert changes, "the route at %d clips is the batch-1 route: the branch-batch gate adds nothing" % batch


# a slow-pathway res4 bottleneck (8 x 16 x 16 voxels per clip): conv_c 256 -> 1024 has 256 tiles of 256 x 256 at 8 clips (the
# eight-phase 256 x 256 kernel) and 32 at one clip (below gemm9_min_tiles; K = 256 is too short for the half-height form: the
# older 128 x 128 kernel).  The block's last conv: its defect reaches the output undiluted.
DEFECT_BLOCK, DEFECT_CONV = "blocks.3.multipathway_blocks.0.res_blocks.1", "conv_c"


def test_the_block_gate_sees_a_five_percent_defect_in_a_layer_the_eight_phase_kernel_serves_at_8_clips():
    """conv_c of one SlowFast-R50 res4 bottleneck x 1.05 in the deploy form only, on the stress instance, at the bench's 8 clips
    per branch -- where that layer runs on an eight-phase kernel, which the batch-1 gate never executes for it."""
    from parity_blocks import defect_case
    batch, tol = _branch_batch("slowfast_r50"), G.BLOCK_BF16_TOL_STRESS["slowfast_r50"]
    r = defect_case("slowfast_r50", DEFECT_BLOCK, scale=1.05, fills=("calibrated",), batch=batch, conv=DEFECT_CONV)
    c = r["calibrated"]
    layer = [op for op in c["route"] if op["label"].startswith(DEFECT_CONV + "|")]
    at_one = [op for rec in _gate("slowfast_r50", 1, floor=False) if rec["name"] == DEFECT_BLOCK for op in rec["route"]
              if op["label"].startswith(DEFECT_CONV + "|")]
    print("\nslowfast_r50 %s, %s x 1.05 at %d clips [calibrated]: clean %.3e (row %d) -> defect %.3e (row %d); gate %.2e; the layer "
          "runs on %s (at one clip: %s)" % (DEFECT_BLOCK, DEFECT_CONV, batch, c["clean"], c["clean_row"], c["defect"], c["defect_row"],
                                            tol, [op["kernel"] for op in layer], [op["kernel"] for op in at_one]))
    G._dump(dict(r, calibrated={k: v for k, v in c.items() if k != "route"}, bound=tol,
                 kernel=[op["kernel"] for op in layer], kernel_at_one_clip=[op["kernel"] for op in at_one]),
            "defect injection at the branch batch: one SlowFast conv_c filter bank x 1.05")
    assert len(layer) == 1 and len(at_one) == 1
    assert layer[0]["kernel"].startswith("gemm_quad") and not at_one[0]["kernel"].startswith("gemm_quad"), (layer, at_one)
    assert c["clean"] <= tol
    assert c["defect"] > c["clean"]
    assert c["defect"] > tol, "a 5 %% defect in %s reads %.3e, below the gate %.2e" % (DEFECT_CONV, c["defect"], tol)


def _off_bench_params():
    return [pytest.param(w, b, marks=pytest.mark.slow) if (w, b) in OFF_BENCH_SLOW else pytest.param(w, b) for w, b in OFF_BENCH]


@pytest.mark.parametrize("workload,batch", _off_bench_params())
def test_every_block_teacher_forced_bf16_off_the_bench_batch(workload, batch):
    recs = _gate(workload, batch)
    _assert_gate(workload, batch, recs, _tol(workload, batch), "off the bench batch")
    _GATE.pop((workload, batch, "trained_like"), None)          # nobody else reads it


@pytest.mark.parametrize("workload", WORKLOADS4)
def test_north_star_odd_batch_split_raggedly_over_two_streams(workload):
    """End to end off the bench shape: bench batch - 1 clips over two sub-batch plans of unequal size (16 + 15, 8 + 7, 4 + 3), the
    assertions and constants of the bench-batch case.  The oracle is evaluated for the first row, the last row of the first
    sub-batch, the first row of the second and the last row, one clip per call (tools/parity_full.py says why)."""
    from bench import WORKLOADS
    from parity_full import case
    batch, streams = WORKLOADS[workload]["batch"] - 1, 2
    first = batch - batch // streams                              # size of the first (larger) sub-batch
    r = case(workload, "trained_like", batch=batch, streams=streams, dtypes=("bf16",), oracle_rows=[0, first - 1, first, batch - 1])
    print("\n%s b=%d (%d + %d) [trained_like], rows %s: bf16 vs fp32 oracle %.2e (worst row %.2e; storage alone %.2e) | vs "
          "bf16-storage oracle %.2e | top-1 %d/%d" % (workload, batch, first, batch - first, r["oracle_rows"], r["bf16_vs_fp32_oracle"],
                                                      r["bf16_rows_worst_fp32"], r["storage_floor"], r["bf16_vs_emulated_oracle"],
                                                      r["top1_agree"], len(r["oracle_rows"])))
    G._dump(r, "north star: odd batch, ragged split over two streams, four rows")
    assert r["oracle_rows"] == [0, first - 1, first, batch - 1]
    G.assert_every_row_of_a_bench_form(r, workload)
