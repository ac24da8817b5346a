"""Which kernel serves which layer at which batch: the table behind profiles/r8/route_census.md.

Input: the route dumps of tests/test_gpu_batch_routing.py (PV_ROUTE_DUMP=<file>: one JSON line per (workload, batch) with every
op's unit, label, kernel symbol and geometry key).  Output (stdout, markdown):
  * per workload and batch the census kernel symbol -> number of ops;
  * every layer whose kernel symbol differs between two batches, with the quantities the GEMM dispatchers decide on
    (csrc/pv_gemm9.hip, pv_gemm9h.hip, pv_gemm8.hip): t256 = 256 x 256 tiles, th = half-height tiles of the same column count,
    half = tiles of the half-height kernel in the shape it would pick (tr = the transposed 256 x 128 tile), t128 = pv_gemm8's
    256-voxel x 128-channel tiles, K;
  * every unit whose op LIST differs between two batches (emitter decisions: pool_stream_min_elems).
`--compact <file>` additionally writes the dumps without the geometry keys (label + kernel per op), the form kept in profiles/.

    python tools/route_census.py routes_a.jsonl [routes_b.jsonl ...] [--compact profiles/r8/route_census.jsonl] > table.md
"""
import collections
import json
import re
import sys


def _geom(g):
    return dict(it.partition("=")[::2] for it in g.split())


def _cd(a, b):
    return -(-a // b)


def _strip(label):
    return re.sub(r"\|\d+x", "|", label, count=1)      # the batch in front of the grid


def gemm_quantities(g):
    """The tile counts pv_gemm9_try / pv_gemm9h_try / pv_gemm8_try compare with their thresholds, from a conv op's geometry key."""
    if not all(k in g for k in ("B", "To", "Ho", "Wo", "cout", "cin", "kt", "kh", "kw")):
        return None
    M = int(g["B"]) * int(g["To"]) * int(g["Ho"]) * int(g["Wo"])
    c8 = _cd(int(g["cout"]), 8) * 8
    tn = _cd(c8, 256)
    waste256, waste128 = (tn * 256 - c8) / c8, (_cd(c8, 128) * 128 - c8) / c8
    tr = waste256 > 0.15 and waste128 <= 0.15
    return {"t256": _cd(M, 256) * tn, "th": _cd(M, 128) * tn, "tr": tr, "half": _cd(M, 256 if tr else 128) * _cd(c8, 128 if tr else 256),
            "t128": _cd(M, 256) * _cd(c8, 128), "K": int(g["kt"]) * int(g["kh"]) * int(g["kw"]) * int(g["cin"])}


def main(argv):
    compact = None
    if "--compact" in argv:
        i = argv.index("--compact")
        compact = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    recs = [json.loads(line) for p in argv for line in open(p)]
    gate, plan = {}, {}
    for r in recs:
        (gate if r["what"] == "gate" else plan)[(r["workload"], r["batch"])] = r
    if compact:
        with open(compact, "w") as f:
            for r in list(gate.values()) + list(plan.values()):
                f.write(json.dumps({"workload": r["workload"], "batch": r["batch"], "what": r["what"], "census": r["census"],
                                    "ops": [[op.get("unit", ""), op["label"], op["kernel"]] for op in r["ops"]]}) + "\n")
    print("## Census: kernel symbol -> ops, per workload and batch\n")
    print("| workload | batch | what | symbols |\n|---|---|---|---|")
    for (w, b), r in sorted(list(gate.items())) + sorted(plan.items()):
        print("| %s | %d | %s | %s |" % (w, b, r["what"], ", ".join("%s %d" % (k.replace("_kernel", ""), v) for k, v in r["census"].items())))
    layers = collections.OrderedDict()
    for (w, b), r in sorted(gate.items()):
        seen = collections.Counter()
        for op in r["ops"]:
            key = (w, op["unit"], _strip(op["label"]))
            seen[key] += 1
            layers.setdefault(key + (seen[key],), {})[b] = (op["kernel"], gemm_quantities(_geom(op["geom"])))
    print("\n## Layers whose kernel symbol depends on the batch\n")
    print("Per batch: kernel (t256 / th / half[ tr] / t128, K).  Layers of one stage with the same row are listed once.\n")
    print("| workload | first unit | layer (per clip) | batch: kernel |\n|---|---|---|---|")
    done = set()
    for key, per in layers.items():
        if len({k for k, _ in per.values()}) < 2:
            continue
        cells = ["%d: %s%s" % (b, k.replace("_kernel", ""), " (%d / %d / %d%s / %d, K %d)" % (
            q["t256"], q["th"], q["half"], " tr" if q["tr"] else "", q["t128"], q["K"]) if q else "") for b, (k, q) in sorted(per.items())]
        sig = (key[0], key[2], tuple(cells))
        if sig in done:
            continue
        done.add(sig)
        print("| %s | %s | `%s` | %s |" % (key[0], key[1], key[2].replace("|", " "), "; ".join(cells)))
    print("\n## Units whose op list depends on the batch (emitter decisions)\n")
    print("| workload | unit | batch: pooling ops |\n|---|---|---|")
    for w in sorted({k[0] for k in gate}):
        bs = sorted(b for (ww, b) in gate if ww == w)
        units = collections.OrderedDict()
        for b in bs:
            for op in gate[(w, b)]["ops"]:
                units.setdefault(op["unit"], {}).setdefault(b, []).append((_strip(op["label"]).split("|")[0], op["kernel"].replace("_kernel", "")))
        for unit, per in units.items():
            if len({tuple(l for l, _ in v) for v in per.values()}) > 1:
                print("| %s | %s | %s |" % (w, unit, "; ".join("%d: %s" % (b, ", ".join("%s=%s" % lk for lk in per[b] if "pool" in lk[0])) for b in bs)))


if __name__ == "__main__":
    main(sys.argv[1:])
