"""The compiler's resource report for every kernel of the given csrc sources, one line per kernel, sorted by name.

    python tools/resource_usage.py [--csrc DIR] td_batch td_match ... > listing.txt

Compiles the device side only, with the build's flags plus -Rpass-analysis=kernel-resource-usage (no GPU needed).  Two
listings of the same sources are equal exactly when the kernel names and every kernel's register, LDS, scratch and
occupancy figures are.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]")


def listing(csrc, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           "-DTD_BUILDING=1", "-DTD_SX_G=8", "-DTD_SX_NG=2", "-DTD_SX_TX=128", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(csrc, name + ".hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.+?): (.+?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    names = sorted(kernels)
    dem = subprocess.run([shutil.which("c++filt") or shutil.which("llvm-cxxfilt")] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    rows = sorted(zip(dem, names))
    return ["%s.hip  %s\n    %s" % (name, d, "  ".join("%s %s" % (k, kernels[n].get(k, "-")) for k in KEYS)) for d, n in rows]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "taxidispatcher_amd", "csrc"))
    ap.add_argument("sources", nargs="+")
    a = ap.parse_args()
    for s in a.sources:
        print("\n".join(listing(os.path.abspath(a.csrc), s)))
