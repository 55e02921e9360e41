#!/usr/bin/env python3
"""Time policy evaluation against the full NN rollout on lqr_d20 (N = 100, float32) and print
one JSON object.

Per batch (4096 and 65 536 by default) and variant, HIP-event time per launch over 20 launches
after 5 warm-ups:
  a  ops.sample + ops.rollout_nn(want_u=False, cost_order=COST_ACTOR)
  b  that rollout_nn alone, dw resident
  c  ops.policy_cost with the same dw
  d  ops.policy_cost(dw=None): the increments drawn in-kernel
and torch.cuda.max_memory_allocated of the measured launches.  Every measurement is a fresh
child process under its own `timeout`; the tool stops at the first non-zero status.

  python tools/bench_policy_cost.py [--batches 4096,65536] [--variants a,b,c,d] [--runs 5]
A tree without dpac_policy_cost (a baseline checkout) runs --variants a,b.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, D, HIDDEN = 100, 1.0, 20, (200, 200, 200)
WARMUP, LAUNCHES = 5, 20
CHILD_TIMEOUT = 180  # seconds per child: start-up, 25 launches of at most tens of ms


def child(batch: int, variant: str) -> None:
    sys.path.insert(0, ROOT)
    import torch

    from deeppde_actorcritic_amd import _lib, ops
    from deeppde_actorcritic_amd import equation as peq
    from deeppde_actorcritic_amd import solver as psol
    from deeppde_actorcritic_amd.config import munchify, set_floatx

    cfg = munchify({
        "eqn_config": {"eqn_name": "LQR", "total_time_critic": T, "total_time_actor": T, "dim": D,
                       "control_dim": D, "num_time_interval_critic": N, "num_time_interval_actor": N,
                       "discount": 1.0, "p": 1.0, "q": 1.0, "beta": 1.0, "R": 1.0},
        "net_config": {"num_hiddens_critic": list(HIDDEN), "num_hiddens_actor": list(HIDDEN), "dtype": "float32"},
        "train_config": {"sample_type": "normal", "scheme": "adaptive", "TD_type": "TD1", "train": "actor-critic"}})
    set_floatx("float32")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eqp = peq.LQR(cfg.eqn_config).params()
    net = psol.DeepNN(cfg, "actor", torch.Generator().manual_seed(3), torch.float32, dev)
    view = net.mlp_view()
    sch, kind = _lib.SCHEME_ADAPTIVE, _lib.SAMPLE_NORMAL
    x0, dw, _ = ops.sample(eqp, kind, batch, N, seed=1, dtype=torch.float32, device=dev,
                           want_dw=variant in "bc")

    def full(w):
        return ops.rollout_nn(eqp, sch, x0, w, T, N, view, want_u=False, cost_order=_lib.COST_ACTOR)

    run = {"a": lambda: full(ops.sample(eqp, kind, batch, N, seed=1, dtype=torch.float32, device=dev)[1]),
           "b": lambda: full(dw),
           "c": lambda: ops.policy_cost(eqp, sch, x0, dw, T, N, view),
           "d": lambda: ops.policy_cost(eqp, sch, x0, None, T, N, view, seed=1)}[variant]
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(LAUNCHES + 1)]
    ev[0].record()
    for i in range(LAUNCHES):
        run()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(LAUNCHES)]
    print(json.dumps({"batch": batch, "variant": variant, "ms_mean": sum(ms) / len(ms), "ms_min": min(ms),
                      "ms_max": max(ms), "peak_bytes": torch.cuda.max_memory_allocated(),
                      "fell_back": bool(ops.x3_fell_back(dev))}))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--runs", type=int, default=5, help="fresh-process runs per batch and variant")
    ap.add_argument("--child", nargs=2, metavar=("BATCH", "VARIANT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(int(args.child[0]), args.child[1])
        return 0
    out = {"workload": {"equation": "LQR", "dim": D, "hidden": list(HIDDEN), "N": N, "T": T, "dtype": "float32",
                        "scheme": "adaptive", "warmup": WARMUP, "launches": LAUNCHES, "runs": args.runs},
           "results": {}}
    status = 0
    for b in (int(v) for v in args.batches.split(",")):
        for v in args.variants.split(","):
            runs = []
            for _ in range(args.runs):
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable,
                                    os.path.abspath(__file__), "--child", str(b), v],
                                   capture_output=True, text=True)
                if p.returncode != 0:  # nothing more on the GPU after a failed step
                    status = p.returncode
                    out["failed"] = {"batch": b, "variant": v, "status": status, "stderr": p.stderr[-2000:]}
                    break
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            if status:
                break
            means = [r["ms_mean"] for r in runs]
            out["results"].setdefault(str(b), {})[v] = {
                "ms_mean_per_run": means, "ms_mean": sum(means) / len(means), "ms_min_run": min(means),
                "ms_max_run": max(means), "peak_bytes": max(r["peak_bytes"] for r in runs),
                "fell_back": any(r["fell_back"] for r in runs)}
        if status:
            break
    print(json.dumps(out))
    return status


if __name__ == "__main__":
    sys.exit(main())
