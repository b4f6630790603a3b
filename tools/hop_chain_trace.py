"""Per-step figures of a g1 benchmark run from a rocprofv3 kernel trace (profiles/hop_chain/README.md,
profiles/hop_fold/README.md).

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python bench.py --steps 15
    python tools/hop_chain_trace.py DIR/NAME_kernel_trace.csv [warm-up steps to drop, default 3]

A step runs from one k_gen_uniform to the last k_final before the next.  Prints the median (min - max) over the steps of
every kernel's time in launch order, of the time from the end of k_gen_uniform to the start of the compress pass, and of
the time from the end of the compress pass to the end of k_final.  The k_hop_* launches carry the number of their two-hop
pass (a pass ends with its k_hop_match, whichever kernels it is made of: four while k_hop_esc made the masks of tight
free columns, three since k_hop_table tests them itself), and every pass gets a line with its sum.  The last two lines: the
idle time in front of k_gen_uniform (end of the step before's last k_final -> start of the cost write: the host round
trip at the end of td_assign) and the launches per step (profiles/front_gap/README.md).
"""
import csv
import re
import statistics
import sys


def short(name):
    m = re.search(r"(k_\w+)(<[^>]*>)?", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:40]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    drop = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], None
    for r in rows:
        k = (short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
        if k[0].startswith("k_gen_uniform"):
            cur = []
            steps.append(cur)
        if cur is not None:
            cur.append(k)
    steps = [s for s in steps if any(k[0].startswith("k_final") for k in s)]
    # end of the step before (its last k_final) -> start of this step's cost write: the host round trip at the end of td_assign
    prev_end = {id(s): max(k[2] for k in p if k[0].startswith("k_final")) for p, s in zip(steps, steps[1:])}
    steps = steps[drop:]
    shape = [k[0] for k in steps[-1]]
    steps = [s for s in steps if [k[0] for k in s] == shape]   # (the steps that launched the same sequence)

    def stat(v):
        return "%7.1f (%.1f - %.1f)" % (statistics.median(v) / 1e3, min(v) / 1e3, max(v) / 1e3)

    print("%d steps of %d launches; us, median (min - max)" % (len(steps), len(shape)))
    npass, passes = 1, {}
    for i, name in enumerate(shape):
        label = name
        if name.startswith("k_hop_"):
            label = "%s  [two-hop pass %d]" % (name, npass)
            passes.setdefault(npass, []).append(i)
            if name.startswith("k_hop_match"):
                npass += 1
        print("  %-72s %s" % (label[:72], stat([s[i][2] - s[i][1] for s in steps])))
    for k, idx in sorted(passes.items()):
        print("two-hop pass %d: %d launches, kernel time            %s" % (k, len(idx), stat([sum(s[i][2] - s[i][1] for i in idx) for s in steps])))
    ci = next(i for i, n in enumerate(shape) if n.startswith("k_compress"))
    fi = max(i for i, n in enumerate(shape) if n.startswith("k_final"))
    print("end of k_gen_uniform -> start of compress   %s" % stat([s[ci][1] - s[0][2] for s in steps]))
    for i in range(1, ci + 1):
        print("    idle in front of %-40s %s" % (shape[i][:40], stat([s[i][1] - s[i - 1][2] for s in steps])))
    print("end of compress -> end of k_final           %s" % stat([s[fi][2] - s[ci][2] for s in steps]))
    print("start of k_gen_uniform -> end of k_final    %s" % stat([s[fi][2] - s[0][1] for s in steps]))
    print("sum of kernel times                         %s" % stat([sum(k[2] - k[1] for k in s) for s in steps]))
    gaps = [s[0][1] - prev_end[id(s)] for s in steps if id(s) in prev_end]
    if gaps:
        print("end of k_final of the step before -> start of k_gen_uniform %s" % stat(gaps))
    print("launches per step                           %d" % len(shape))


if __name__ == "__main__":
    main()
