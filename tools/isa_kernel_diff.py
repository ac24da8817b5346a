"""Compare the bodies of the kernels of two `hipcc -S --cuda-device-only` listings of one translation unit.

    python tools/isa_kernel_diff.py before.s after.s [name-regex]

A body is the text from a kernel's label to its `.Lfunc_end` marker, without comment lines and without the names of local labels
(`.LBB12_3`), which are numbered per translation unit and move when kernels are added.  Prints one line per kernel of
`before` whose name matches: `same`, `DIFFERENT` or `missing`, with the metadata (VGPRs, SGPRs, private segment, spills)
of both sides, then a count.  Exit status 1 if any body differs or is missing."""
import re
import sys


def bodies(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = []
        for ln in m.group(2).splitlines():
            ln = ln.split(";")[0].rstrip()
            if ln.strip():
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[m.group(1)] = "\n".join(lines)
    meta = {}
    for name, body in re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        kv = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", body)}
        meta[name] = (kv.get("vgpr_count"), kv.get("sgpr_count"), kv.get("private_segment_fixed_size"),
                      kv.get("vgpr_spill_count"), kv.get("sgpr_spill_count"))
    return out, meta


def main():
    before, mb = bodies(sys.argv[1])
    after, ma = bodies(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    bad = n = 0
    for name in sorted(before):
        if not pat.search(name):
            continue
        n += 1
        state = "missing" if name not in after else ("same" if before[name] == after[name] else "DIFFERENT")
        bad += state != "same"
        print("%-9s %s  before %s  after %s" % (state, name, mb.get(name), ma.get(name)))
    print("%d kernels compared, %d not identical" % (n, bad))
    return 1 if bad or not n else 0


if __name__ == "__main__":
    sys.exit(main())
