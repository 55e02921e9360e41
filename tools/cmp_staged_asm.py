#!/usr/bin/env python3
"""Compare the generated code of every k_rollout_staged instantiation (--all: of every function)
in two device assembly files of the same translation unit (two commits, or two values of a build
knob):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -Ideeppde_actorcritic_amd/csrc \\
        -DDPAC_DIMS=20 -DDPAC_DIMS_EVEN=20 -DDPAC_TU_DOUBLE=0 --cuda-device-only -S \\
        deeppde_actorcritic_amd/csrc/dpac_eqn_lqr.hip -o new.s        (and the same of the other tree)
    python tools/cmp_staged_asm.py old.s new.s

Comments are dropped, block labels lose the function's position in the file (.LBB12_3 ->
.LBB_3) and the function's own name reads <self>; everything else, register names and the
kernel descriptor included, must match for IDENTICAL.
--expect-identical PATTERN (repeatable) makes the exit status 1 unless every instantiation whose
demangled template arguments end in PATTERN is identical, e.g. ", 12>" for the generator variant;
the pattern "" asks it of every function, and so of both files to hold the same set of them.
--drop-old-arg K pairs functions by demangled name after the K-th template argument (from 0) of
each k_rollout_staged instantiation of the OLD file is removed: for a change that drops a template
parameter.  The pairing must be one to one.
--summary prints one line, "<functions> functions, <identical> identical", instead of one per function.
"""
import argparse
import re
import shutil
import subprocess
import sys

STAGED = r"_ZN4dpac16k_rollout_staged\w+"


def funcs(path, name_re):
    out, cur, own = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"^(%s):" % name_re, line)
        if m:
            own = m.group(1)
            cur = out.setdefault(own, [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip()).replace(own, "<self>")
        if line.strip():
            cur.append(line)
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return list(names)
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return [re.sub(r"^void dpac::|\(dpac::.*$", "", s) for s in out.splitlines()]


def drop_arg(pretty, k):
    """pretty without its k-th top-level template argument, if it is a k_rollout_staged<...>."""
    head = "k_rollout_staged<"
    if not pretty.startswith(head) or not pretty.endswith(">"):
        return pretty
    args, depth, start = [], 0, len(head)
    for i in range(start, len(pretty) - 1):
        ch = pretty[i]
        depth += (ch in "<(") - (ch in ">)")
        if ch == "," and depth == 0:
            args.append(pretty[start:i].strip())
            start = i + 1
    args.append(pretty[start:-1].strip())
    del args[k]
    return head + ", ".join(args) + ">"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--all", action="store_true", help="every function of the unit, not only k_rollout_staged")
    ap.add_argument("--expect-identical", action="append", default=[])
    ap.add_argument("--drop-old-arg", type=int, default=None, metavar="K")
    ap.add_argument("--summary", action="store_true")
    a = ap.parse_args()
    name_re = r"_Z\w+" if a.all else STAGED
    fa, fb = funcs(a.old, name_re), funcs(a.new, name_re)
    # keyed by demangled name (the old file's with one argument dropped, if asked)
    ka = list(zip(demangle(list(fa)), fa.values()))
    kb = dict(zip(demangle(list(fb)), fb.values()))
    if a.drop_old_arg is not None:
        ka = [(drop_arg(pretty, a.drop_old_arg), body) for pretty, body in ka]
    if len(dict(ka)) != len(fa) or len(kb) != len(fb):
        sys.exit("pairing by demangled name is not one to one")
    ka = dict(ka)
    names = sorted(set(ka) | set(kb))
    bad = ident = 0
    for pretty in names:
        la, lb = ka.get(pretty), kb.get(pretty)
        same = la is not None and la == lb
        ident += same
        if not a.summary:
            print(f"{pretty}: {len(la or [])} -> {len(lb or [])} lines, {'IDENTICAL' if same else 'differs'}")
        bad += (not same) and any(pretty.endswith(p) for p in a.expect_identical)
    if a.summary:
        print(f"{len(names)} functions, {ident} identical")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main())
