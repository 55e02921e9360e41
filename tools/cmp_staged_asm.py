#!/usr/bin/env python3
"""Compare the generated code of every k_rollout_staged instantiation in two device assembly
files of the same translation unit (two commits, or two values of a build knob):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Ideeppde_actorcritic_amd/csrc \\
        -DDPAC_DIMS=20 -DDPAC_DIMS_EVEN=20 -DDPAC_TU_DOUBLE=0 --cuda-device-only -S \\
        deeppde_actorcritic_amd/csrc/dpac_eqn_lqr.hip -o new.s        (and the same of the other tree)
    python tools/cmp_staged_asm.py old.s new.s

Comments are dropped; everything else, register names included, must match for IDENTICAL.
--expect-identical PATTERN (repeatable) makes the exit status 1 unless every instantiation whose
demangled template arguments end in PATTERN is identical, e.g. ", 12>" for the generator variant.
"""
import argparse
import re
import shutil
import subprocess
import sys


def funcs(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(_ZN4dpac16k_rollout_staged\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = line.split(";")[0].rstrip()
        if line.strip():
            cur.append(line)
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return list(names)
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void dpac::|\(dpac::.*$", "", s) for s in out.splitlines()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--expect-identical", action="append", default=[])
    a = ap.parse_args()
    fa, fb = funcs(a.old), funcs(a.new)
    names = sorted(set(fa) | set(fb))
    bad = 0
    for n, pretty in zip(names, demangle(names)):
        la, lb = fa.get(n), fb.get(n)
        same = la is not None and la == lb
        print(f"{pretty}: {len(la or [])} -> {len(lb or [])} lines, {'IDENTICAL' if same else 'differs'}")
        bad += (not same) and any(pretty.endswith(p) for p in a.expect_identical)
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main())
