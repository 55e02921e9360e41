#!/usr/bin/env python3
"""Resource usage of the three NN forward kernels (k_rollout_nn, k_rollout_nn4, k_rollout_nn_x3)
from two build logs made with `make lib HIPCC="hipcc -Rpass-analysis=kernel-resource-usage"`:
the baseline's and this tree's, side by side per existing instantiation, then the lean ones
(NnMode 1 / 2) beside their full counterpart (COST = true, no saves).  A cross-compile: no GPU.

  python tools/nn_mode_resources.py BASE.log TREE.log > profiles/policy_cost_resources.txt
"""
import re
import subprocess
import sys

KEYS = (("vgpr", r"    VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))
KERNEL = re.compile(r"dpac::(k_rollout_nn4|k_rollout_nn_x3|k_rollout_nn)<")


def parse(path):
    """{demangled instantiation: {vgpr, agpr, scratch, lds, occ}} of the three kernels."""
    rows, cur, names = {}, None, []
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {}
            names.append((m.group(1), cur))
            continue
        if cur is not None:
            for key, pat in KEYS:
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    dem = subprocess.run(["c++filt"], input="\n".join(n for n, _ in names), capture_output=True,
                         text=True).stdout.splitlines()
    for full, (_, vals) in zip(dem, names):
        if KERNEL.search(full):
            name = re.sub(r"\(.*", "", full.replace("dpac::", ""))
            name = re.sub(r"^void ", "", name)
            rows[name] = vals
    return rows


def mode_of(name):
    """(the instantiation with its NnMode argument removed, the mode)."""
    m = re.search(r", \(?(?:NnMode\))?(\d)>$", name)
    return (name[:m.start()] + ">", int(m.group(1))) if m else (name, 0)


def fmt(v):
    return "%4d vgpr %3d agpr %5d scratch %6d lds  occ %d" % (v["vgpr"], v["agpr"], v["scratch"], v["lds"], v["occ"])


def main(base_log, tree_log):
    base, tree = parse(base_log), parse(tree_log)
    full, lean = {}, {}
    for name, v in tree.items():
        stem, mode = mode_of(name)
        (full if mode == 0 else lean)[(stem, mode)] = v
    print("# existing instantiations: baseline | this tree")
    diff = 0
    for name in sorted(base):
        stem = None
        for cand in (name, name[:-1] + ", false>"):  # k_rollout_nn's MASK default is spelled out now
            if (cand, 0) in full:
                stem = cand
        t = full.get((stem, 0))
        same = t is not None and all(t[k] == base[name][k] for k in ("vgpr", "agpr", "scratch", "lds", "occ"))
        diff += not same
        print(f"{fmt(base[name])} | {fmt(t) if t else 'missing':<58} {'same' if same else 'DIFFERS'}  {name}")
    print(f"# {len(base)} existing instantiations, {diff} differ")
    print("# lean instantiations (mode 1: dw read, mode 2: dw drawn in-kernel) | full counterpart")
    worse = 0
    for (stem, mode), v in sorted(lean.items()):
        ref = full.get((stem, 0))
        more = ref is not None and v["scratch"] > ref["scratch"]
        worse += more
        print(f"mode {mode} {fmt(v)} | {fmt(ref) if ref else 'missing':<58} "
              f"{'MORE SCRATCH' if more else 'ok'}  {stem}")
    print(f"# {len(lean)} lean instantiations, {worse} with more scratch than their full counterpart")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
