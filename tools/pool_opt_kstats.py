"""Readable summary of a rocprofv3 --kernel-trace --stats run of tools/pool_opt_time.py.

    python tools/pool_opt_kstats.py <rocprofv3 output dir> [out.txt [title line]]

Part 1: the run's kernel_stats.csv (every kernel, named).  Part 2: from kernel_trace.csv, per kernel and grid size (in
workgroups) the number of dispatches and the median / min / max duration, so that the 1000-model calls (grid 1000) and
the single-model calls (grid 1) of the same kernel stay apart.  Register and LDS use are not taken from the trace: see
DESIGN.md 3.5 (-Rpass-analysis=kernel-resource-usage of the build).
"""
import collections
import csv
import glob
import os
import statistics
import sys


def clean(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]


def main():
    d = sys.argv[1]
    stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[-1]
    trace = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1]
    out = ["# " + sys.argv[3]] if len(sys.argv) > 3 else []
    out.append("# kernel stats (all dispatches of the run): name | calls | total_us | avg_us | percent")
    for r in csv.DictReader(open(stats)):
        out.append("%s | %s | %.1f | %.1f | %.3f" % (clean(r["Name"]), r["Calls"], int(r["TotalDurationNs"]) / 1e3,
                                                    float(r["AverageNs"]) / 1e3, float(r["Percentage"])))
    g = collections.defaultdict(list)
    for r in csv.DictReader(open(trace)):
        key = (clean(r["Kernel_Name"]), int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1))
        g[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out.append("")
    out.append("# per kernel and grid (workgroups), from the trace: name | grid | dispatches | median_us | min_us | max_us")
    for (name, grid), ts in sorted(g.items(), key=lambda kv: -sum(kv[1])):
        out.append("%s | %d | %d | %.1f | %.1f | %.1f" % (name, grid, len(ts), statistics.median(ts), min(ts), max(ts)))
    text = "\n".join(out) + "\n"
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
