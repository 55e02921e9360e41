#!/usr/bin/env python3
"""Time breakdown of the staged rollout kernel from a -DDPAC_ST_TRACE=1 build (GPU only): lane 0
of every wavefront of the first and the last workgroup of k_rollout_staged records the shader
clock at fixed points (ST_MARK in dpac_rollout_staged.h).  Runs bench.py's headline launch (LQR d = 20,
B = 4096, N = 200, rotating HBM-cold buffer sets) and prints the table of the last launch.

    bash tools/build_variants.sh "sttrace:-DDPAC_ST_TRACE=1 -DDPAC_TU_TRACE=1"
    DPAC_LIB=tools/variants/libdpac_sttrace.so python tools/probe_staged_trace.py
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROW, WAVES, CHUNKS, CH = 128, 16, 32, 16  # kStTraceRow, kStTraceWaves, kStTraceChunks, kStCH


def rel(a, b):
    """a - b of two 32-bit clock stamps."""
    d = (int(a) - int(b)) & 0xFFFFFFFF
    return d - (1 << 32) if d >= 1 << 31 else d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--scheme", choices=["adaptive", "naive"], default="adaptive")
    a = ap.parse_args()
    import bench
    from deeppde_actorcritic_amd import _lib
    from deeppde_actorcritic_amd.equation import LQR
    lib = _lib.load()
    lib.dpac_debug_staged_trace.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    torch.cuda.set_device(0)
    dtype = torch.float32 if a.dtype == "f32" else torch.float64
    scheme = _lib.SCHEME_ADAPTIVE if a.scheme == "adaptive" else _lib.SCHEME_NAIVE
    B, N, d = bench.B_PER_GPU, bench.HORIZON, bench.DIM
    rs = bench.RolloutSets(lib, LQR(bench.lqr_config()).params(), scheme, dtype, B, N, d, 0, bench.N_SETS)
    launch = rs.launcher(bench.N_SETS)
    for i in range(a.launches):
        launch(i)
    torch.cuda.synchronize()
    buf = np.zeros(2 * WAVES * ROW, dtype=np.uint32)
    assert lib.dpac_debug_staged_trace(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(buf.nbytes)) == 0
    tr = buf.reshape(2, WAVES, ROW)
    nch = (N + CH - 1) // CH
    full = N // CH
    assert nch <= CHUNKS
    print(f"# k_rollout_staged clock trace: {a.dtype} {a.scheme} LQR d={d} B={B} N={N}, launch {a.launches} of "
          f"{a.launches} over {bench.N_SETS} cold buffer sets; cycles of the shader clock since the wave's entry")
    per_step, period, handoff, tail = [], [], [], []
    for g, gname in enumerate(("first workgroup", "last workgroup")):
        t0 = tr[g, 0, 0]
        rt = rel(tr[g, 0, 6], tr[g, 0, 5])  # 100 MHz ticks, compute wave 0
        cyc = rel(tr[g, 0, 7], tr[g, 0, 0])
        mhz = cyc / rt * 100.0 if rt > 0 else float("nan")
        print(f"\n## {gname}: wave 0 lives {cyc} cycles = {rt / 100.0:.2f} us (real-time clock) -> {mhz:.0f} MHz; "
              f"real-time entry stamp {int(tr[g, 0, 5])}")
        print("wave      entry  barrier  x0+r0  ready0  stores_issued  stores_acked   (vs wave 0's entry)")
        for w in range(5):
            r = tr[g, w]
            cells = [rel(r[p], t0) for p in (0, 1)]
            if w < 4:
                cells += [rel(r[2], t0), rel(r[3], t0), rel(r[4], t0), rel(r[7], t0)]
                print("compute%d %6d %8d %6d %7d %14d %13d" % ((w,) + tuple(cells)))
            else:
                print("loader   %6d %8d   last publish %d" % (cells[0], cells[1], rel(r[4], t0)))
        print("chunk  " + "  ".join(f"w{w}:start   end  poll" for w in range(4)) + "  loader:issue0 issued publish")
        for c in range(nch):
            line = "%5d  " % c
            for w in range(4):
                r = tr[g, w]
                s, e, p = rel(r[16 + c], t0), rel(r[48 + c], t0), int(r[80 + c])
                line += "%8d %6d %5d  " % (s, e, p)
                if c < full and c >= 1:
                    per_step.append((e - s) / CH)
                if 2 <= c < full:  # chunk 1 may still wait for the loader
                    period.append((s - rel(r[16 + c - 1], t0)) / CH)
                    handoff.append(s - rel(r[48 + c - 1], t0))
                if c == full and N % CH:
                    tail.append(e - s)
            r = tr[g, 4]
            line += "%13d %6d %7s" % (rel(r[16 + c], t0), rel(r[48 + c], t0), rel(r[80 + c], t0) if r[80 + c] else "-")
            print(line)
    ps = np.array(per_step)
    print(f"\nsteady state (full chunks 1..{full - 1}, both workgroups, 4 compute waves): "
          f"median {np.median(ps):.1f} cycles/step, min {ps.min():.1f}, max {ps.max():.1f} "
          f"(includes the two stamps per chunk, about 40 cycles each: -5 cycles/step)")
    if period:
        pe, ho = np.array(period), np.array(handoff)
        print(f"chunk period (start of chunk c - 1 to start of chunk c, c = 2..{full - 1}, hand-off and stamps "
              f"included): median {np.median(pe):.1f} cycles/step, min {pe.min():.1f}, max {pe.max():.1f}")
        print(f"hand-off (end stamp of chunk c - 1, after its `done` publish, to start stamp of chunk c, "
              f"after the `ready` poll): median {np.median(ho):.0f} cycles, min {ho.min()}, max {ho.max()}")
    if tail:
        ta = np.array(tail)
        print(f"last {N % CH} steps (the remainder after {full} full chunks): median {np.median(ta):.0f} cycles, "
              f"min {ta.min()}, max {ta.max()} = {np.median(ta) / (N % CH):.1f} cycles/step")
    w0 = tr[:, :4]
    poll = w0[:, :, 80:80 + nch].astype(np.int64)
    print(f"ready polls: chunk 0 median {np.median(poll[:, :, 0]):.0f} cycles, later chunks median "
          f"{np.median(poll[:, :, 1:]):.0f}, max {poll[:, :, 1:].max()} (a poll that finds the chunk ready costs "
          f"one LDS read and the stamps)")
    skew = rel(tr[1, 0, 5], tr[0, 0, 5])
    print(f"launch ramp: the last workgroup enters {skew / 100.0:.2f} us after the first (real-time clock)")


if __name__ == "__main__":
    main()
