#!/usr/bin/env python3
"""Register and scratch use of every k_rollout_staged instantiation, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks of a whole build:

    make clean && make -j8 --output-sync=target lib HIPCC="/opt/rocm/bin/hipcc -Rpass-analysis=kernel-resource-usage" 2> remarks.txt
    python tools/staged_resources.py remarks.txt > profiles/staged_prefetch_resources_after.txt

Prints one line per instantiation (demangled with c++filt where there is one) and, last, how
many of them use scratch.  Exit status 1 if any does.
"""
import re
import shutil
import subprocess
import sys

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
        "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return names
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void dpac::|\(dpac::.*$", "", s) for s in out.splitlines()]


def main():
    rows, cur = {}, None
    for path in sys.argv[1:]:
        for line in open(path, errors="replace"):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = rows.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:(?: \S+:\d+:\d+:)?\s+([A-Za-z][^:]*): (\w+) \[-Rpass-analysis", line)
            if m and cur is not None and m.group(1) in KEYS:
                cur[m.group(1)] = m.group(2)
    staged = sorted(n for n in rows if "k_rollout_staged" in n)
    names = demangle(staged)
    print("# " + " | ".join(("instantiation",) + KEYS))
    bad = 0
    for n, pretty in sorted(zip(staged, names), key=lambda p: p[1]):
        r = rows[n]
        bad += r.get("ScratchSize [bytes/lane]", "0") != "0"
        print(" | ".join([pretty] + [r.get(k, "?") for k in KEYS]))
    print(f"# {len(staged)} instantiations, {bad} with scratch")
    return 1 if bad or not staged else 0


if __name__ == "__main__":
    sys.exit(main())
