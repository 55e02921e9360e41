"""GPU: Adam with its step count and alpha schedule in device memory (dpac_adam_step,
DPAC_ADAM=device), captured inside the solver's HIP graphs, against the host-scalar path
(dpac_adam_apply, DPAC_ADAM=host): everything compared bitwise.

* the kernel against ops.adam_apply with tf_adam_scalars' alpha: across lr boundaries, over more
  tensors than one launch takes, as two halves of one step, past the table's end, under replay;
* the solver with ADAM "device" against "host" after every iteration, small shape and
  production shape, and no optimizer launch from the host once the graphs exist;
* save and restore: 3 + 3 iterations equal 6.
"""
import weakref

import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import equation as peq
from deeppde_actorcritic_amd import ops
from deeppde_actorcritic_amd import solver as psol
from tests.helpers import full_config

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
BOUNDS, VALUES = [2, 4], [1e-3, 5e-4, 1e-4]
SCHEDULE = psol.PiecewiseConstantDecay(BOUNDS, VALUES)
# 1 element, one short of / exactly / one past a workgroup's 256 threads, several workgroups
FIVE = [1, 255, 256, 257, 4000]
FORTY = FIVE + [3 + 37 * i for i in range(35)]  # 40 tensors: two launches (32 per launch)


def _eq(a, b):
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


def _table(dtype):
    return torch.from_numpy(psol.adam_alpha_table(SCHEDULE, B1, B2, dtype).copy()).cuda()


class _Vars:
    """Seeded variables and moments on the GPU (the moments start non-zero: every term of the
    update is live from the first step)."""

    def __init__(self, sizes, dtype, seed=0):
        g = torch.Generator().manual_seed(seed)
        mk = lambda n, s: (torch.randn(n, generator=g, dtype=torch.float64) * s).to(dtype).cuda()
        self.v = [mk(n, 1.0) for n in sizes]
        self.m = [mk(n, 0.1) for n in sizes]
        self.s = [mk(n, 0.1).square() for n in sizes]

    def all(self):
        return self.v + self.m + self.s


def _grads(sizes, dtype, step):
    g = torch.Generator().manual_seed(1000 + step)
    return [torch.randn(n, generator=g, dtype=torch.float64).to(dtype).cuda() for n in sizes]


def _host_step(x, gs, t, dtype):
    alpha = psol.tf_adam_scalars(SCHEDULE(t - 1), t, B1, B2, dtype)[0]
    ops.adam_apply(x.v, gs, x.m, x.s, alpha, B1, B2, EPS)


@pytest.mark.parametrize("sizes", [FIVE, FORTY], ids=["five", "forty"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kernel_matches_host_scalars(dtype, sizes):
    """8 steps over both lr boundaries: var, m, v bitwise those of adam_apply with the host's
    alpha, the device counter equal to the step number; the same list applied as two disjoint
    halves (advance=0, then 1); a call without tensors moves only the counter."""
    ref, one, two = (_Vars(sizes, dtype) for _ in range(3))
    table = _table(dtype)
    st1, st2 = ops.adam_state("cuda"), ops.adam_state("cuda")
    h = len(sizes) // 2
    for t in range(1, 9):
        gs = _grads(sizes, dtype, t)
        _host_step(ref, gs, t, dtype)
        ops.adam_step(one.v, gs, one.m, one.s, st1, table, B1, B2, EPS, True)
        ops.adam_step(two.v[:h], gs[:h], two.m[:h], two.s[:h], st2, table, B1, B2, EPS, False)
        assert st2.tolist() == [t - 1, 0]
        ops.adam_step(two.v[h:], gs[h:], two.m[h:], two.s[h:], st2, table, B1, B2, EPS, True)
        assert st1.tolist() == [t, 0] and st2.tolist() == [t, 0]
        for a, b, c in zip(ref.all(), one.all(), two.all()):
            _eq(b, a)
            _eq(c, a)
    before = [x.clone() for x in one.all()]
    ops.adam_step([], [], [], [], st1, table, B1, B2, EPS, True)
    ops.adam_step([], [], [], [], st1, table, B1, B2, EPS, False)
    assert st1.tolist() == [9, 0]
    for a, b in zip(before, one.all()):
        _eq(b, a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_step_past_the_tables_end(dtype):
    """iterations = 10^6, far past the table: the clamped index gives the host's alpha of
    t = 10^6 + 1."""
    ref, dev = _Vars(FIVE, dtype), _Vars(FIVE, dtype)
    table = _table(dtype)
    assert table.numel() < 10 ** 5
    st = ops.adam_state("cuda")
    st[0] = 10 ** 6
    gs = _grads(FIVE, dtype, 0)
    _host_step(ref, gs, 10 ** 6 + 1, dtype)
    ops.adam_step(dev.v, gs, dev.m, dev.s, st, table, B1, B2, EPS, True)
    assert st.tolist() == [10 ** 6 + 1, 0]
    for a, b in zip(ref.all(), dev.all()):
        _eq(b, a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_captured_step_follows_the_schedule_under_replay(dtype):
    """One adam_step captured in a HIP graph and replayed 6 times across both boundaries, the
    gradient buffer refilled between replays: bitwise the host path (a by-value alpha would
    stay that of the capture)."""
    ref, dev = _Vars(FORTY, dtype), _Vars(FORTY, dtype)
    table = _table(dtype)
    st = ops.adam_state("cuda")
    gbuf = _grads(FORTY, dtype, 0)
    warm = _Vars([5], dtype)  # the kernels' first launch outside the capture, on other tensors
    ops.adam_step(warm.v, _grads([5], dtype, 0), warm.m, warm.s, ops.adam_state("cuda"), table, B1, B2, EPS, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.adam_step(dev.v, gbuf, dev.m, dev.s, st, table, B1, B2, EPS, True)
    assert st.tolist() == [0, 0]  # capturing applies nothing
    for t in range(1, 7):
        gs = _grads(FORTY, dtype, t)
        for dst, src in zip(gbuf, gs):
            dst.copy_(src)
        graph.replay()
        _host_step(ref, gs, t, dtype)
        assert st.tolist() == [t, 0]
        for a, b in zip(ref.all(), dev.all()):
            _eq(b, a)


# ---- the solver -----------------------------------------------------------------------------
def _small_cfg(dtype, td="TD1", train="actor-critic"):
    cfg = full_config("LQR", 4, N=6, hidden=(16, 16), batch=96, td=td, train=train, dtype=dtype)
    for k in ("critic", "actor"):
        cfg.net_config["lr_boundaries_" + k] = list(BOUNDS)
    return cfg


def _iterate(sp, cfg):
    B, N = cfg.net_config.batch_size, cfg.eqn_config.num_time_interval_critic
    mode = cfg.train_config.train
    if mode == "actor-critic":  # the loop body of solver.train and bench.py
        dc, da = sp.sample_iteration(B, N, N)
        sp.train_iteration(dc, da, B)
        sp.prefetch_samples(B, N, N)
    elif mode == "critic":
        sp.train_step_critic(sp.sample(B, N), B)
    else:
        sp.train_step_actor(sp.sample(B, N), B)


def _params(sp):
    torch.cuda.synchronize()
    return [v.detach().cpu().clone() for v in sp.critic_variables() + sp.actor_variables()]


def _run(monkeypatch, adam, cfg, graphs, iters, seed=5, each=None):
    """The parameters after every iteration with psol.ADAM = adam; each(solver, i) runs first
    in iteration i (1-based)."""
    monkeypatch.setattr(psol, "ADAM", adam)
    sp = psol.ActorCriticSolver(cfg, peq.LQR(cfg.eqn_config), seed=seed, sampler="device", graphs=graphs)
    out = []
    for i in range(1, iters + 1):
        if each is not None:
            each(sp, i)
        _iterate(sp, cfg)
        out.append(_params(sp))
    if adam == "host":  # the patch reached the optimizers: no step ever ran on the device path
        assert sp.optimizer_critic.device_iterations() is None and sp.optimizer_actor.device_iterations() is None
    return sp, out


# DPAC_GBACK is read only where the critic step is split (actor-critic, TD1, graphs): "early"
# runs there; every other case runs the same code under either value.
CASES = [(dt, g, td, tr, "late") for dt in ("float32", "float64") for g in (True, False)
         for td in ("TD1", "TD2") for tr in ("actor-critic", "critic", "actor")]
CASES += [(dt, True, "TD1", "actor-critic", "early") for dt in ("float32", "float64")]


@pytest.mark.parametrize("dtype,graphs,td,train,gback", CASES,
                         ids=["-".join([c[0], "graphs" if c[1] else "eager", *c[2:]]) for c in CASES])
def test_solver_device_matches_host_every_iteration(monkeypatch, dtype, graphs, td, train, gback):
    """6 iterations over both lr boundaries: ADAM "device" (the steps inside the graphs, or
    host-launched dpac_adam_step without graphs) against "host", bitwise after every iteration;
    the device counters equal the host's counts."""
    monkeypatch.setattr(psol, "GBACK", gback)
    cfg = _small_cfg(dtype, td, train)
    _, want = _run(monkeypatch, "host", cfg, graphs, 6)
    sp, got = _run(monkeypatch, "device", cfg, graphs, 6)
    for i, (w, g) in enumerate(zip(want, got)):
        for a, b in zip(w, g):
            assert torch.equal(a, b), f"iteration {i + 1}"
    assert any(not torch.equal(a, b) for a, b in zip(want[0], want[5]))
    if train == "actor-critic" and td == "TD1" and graphs:
        assert sp._critic_split_ok()
    used = {"actor-critic": ("critic", "actor"), "critic": ("critic",), "actor": ("actor",)}[train]
    for k in used:
        opt = getattr(sp, "optimizer_" + k)
        assert opt.iterations == 6 and opt.device_iterations() == 6, k


@pytest.mark.parametrize("td", ["TD1", "TD2"])
def test_no_optimizer_launch_from_the_host_once_the_graphs_exist(monkeypatch, td):
    """With graphs in one process, both graph sets exist after two iterations: iterations 3 to 6
    call neither ops.adam_step nor ops.adam_apply (the steps are replayed), and building the
    graphs applied no step of its own (the counts are 6)."""
    calls = []
    real_step, real_apply = ops.adam_step, ops.adam_apply
    monkeypatch.setattr(ops, "adam_step", lambda *a, **k: (calls.append("step"), real_step(*a, **k))[1])
    monkeypatch.setattr(ops, "adam_apply", lambda *a, **k: (calls.append("apply"), real_apply(*a, **k))[1])
    seen = {}
    sp, _ = _run(monkeypatch, "device", _small_cfg("float32", td), True, 6,
                 each=lambda s, i: seen.setdefault(i, len(calls)))
    assert "apply" not in calls
    assert len(calls) == seen[3], (calls, seen)  # nothing since iteration 3 began
    assert seen[3] > 0  # the captures go through ops.adam_step
    for opt in (sp.optimizer_critic, sp.optimizer_actor):
        assert opt.iterations == 6 and opt.device_iterations() == 6


@pytest.mark.parametrize("sets", [1, 2])
def test_production_shape_device_matches_host(monkeypatch, sets):
    """The float32 production path (lqr_d20, B = 2048, N = 100, HIP graphs, split steps, device
    sampler; tests/test_gpu_training.py's shape), 4 iterations with the lr boundaries at 2 and 3:
    bitwise, with one and with two graph sets."""
    from deeppde_actorcritic_amd.config import baseline_config
    monkeypatch.setattr(psol, "GRAPH_SETS", sets)
    out = {}
    for adam in ("host", "device"):
        monkeypatch.setattr(psol, "ADAM", adam)
        ops.x3_status_reset("cuda")
        cfg = baseline_config(4, 10 ** 9, "float32", 2048, 256, "lqr_d20")
        for k in ("critic", "actor"):
            cfg.net_config["lr_boundaries_" + k] = [2, 3]
        sp = psol.ActorCriticSolver(cfg, peq.LQR(cfg.eqn_config), seed=5, sampler="device")
        for _ in range(4):
            dc, da = sp.sample_iteration(2048, 100, 100)
            sp.train_iteration(dc, da, 2048)
            sp.prefetch_samples(2048, 100, 100)
        assert sp._critic_split_ok()
        assert sum(s is not None for v in sp._gsets.values() for s in v) == sets
        if adam == "host":
            assert sp.optimizer_critic.device_iterations() is None and sp.optimizer_actor.device_iterations() is None
        out[adam] = _params(sp)
        # in no reference cycle: a solver left to the garbage collector could be freed, its HIP
        # graphs destroyed, inside a later solver's capture, which aborts the process
        gone = weakref.ref(sp)
        del sp
        assert gone() is None
    for a, b in zip(out["host"], out["device"]):
        assert torch.equal(a, b)


GUARDS = [(False, False), (True, False), (True, True)]  # (GUARD_DEFER, GUARD_DEFER_JOIN)


def test_actor_split_without_the_critic_split_all_guard_modes_and_both_adams(monkeypatch):
    """train = "actor-critic" under TD2 with graphs: the actor step is split around the unsplit
    critic step (one _SplitActorGraphs in sp._graphs, no graph set), so train_iteration replays the
    actor chain's redo graph and then counts or applies the actor's step on its own.  4 iterations
    at _small_cfg's shape under DPAC_GUARD_DEFER = 0, 1 and join, each with ADAM host and device:
    all six bitwise equal, ops.x3_fell_back the same (clear).  At this shape the actor chain does
    collect deferred fallbacks (two, before and after the chain moved to _BackwardChain: in float32
    the split-fp16 range guard is on at every batch size), so the batch stays 96."""
    cfg = _small_cfg("float32", "TD2")
    runs = {}
    for defer, join in GUARDS:
        monkeypatch.setattr(psol, "GUARD_DEFER", defer)
        monkeypatch.setattr(psol, "GUARD_DEFER_JOIN", join)
        for adam in ("host", "device"):
            ops.x3_status_reset("cuda")
            sp, out = _run(monkeypatch, adam, cfg, True, 4)
            assert sp._actor_split_ok() and not sp._critic_split_ok() and not sp._gsets
            chain, = [g.chain for k, g in sp._graphs.items() if k[0] == "actor_split"]
            assert bool(chain.redo_fns) == defer
            assert chain.stepped == (adam == "device")
            assert (chain.g_redo is not None) == join
            assert sp.optimizer_actor.iterations == sp.optimizer_critic.iterations == 4
            runs[defer, join, adam] = (out, ops.x3_fell_back("cuda"))
            gone = weakref.ref(sp)  # in no reference cycle (test_production_shape_device_matches_host)
            del sp, chain
            assert gone() is None
    want, fell = runs[False, False, "host"]
    assert fell is False and any(not torch.equal(a, b) for a, b in zip(want[0], want[3]))
    for key, (got, f) in runs.items():
        assert f == fell, key
        for i, (w, g) in enumerate(zip(want, got)):
            for a, b in zip(w, g):
                assert torch.equal(a, b), (key, i + 1)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_resume_continues_bit_for_bit(monkeypatch, dtype):
    """3 iterations, state_dict(), a new solver from the same config and seed, load_state_dict(),
    3 more: parameters and both optimizers' moments bitwise those of 6 uninterrupted iterations
    (the pair prefetch_samples drew ahead is drawn again under the same keys)."""
    cfg = _small_cfg(dtype)
    whole, _ = _run(monkeypatch, "device", cfg, True, 6)
    first, _ = _run(monkeypatch, "device", cfg, True, 3)
    sd = first.state_dict()
    assert first._next_samples is not None and sd["sampler_calls"] == first._calls - 2
    assert sd["optimizer_critic"]["iterations"] == sd["optimizer_actor"]["iterations"] == 3
    fresh = psol.ActorCriticSolver(cfg, peq.LQR(cfg.eqn_config), seed=5, sampler="device", graphs=True)
    fresh.load_state_dict(sd)
    for _ in range(3):
        _iterate(fresh, cfg)
    a, b = whole.state_dict(), fresh.state_dict()
    for net in ("critic", "critic_grad", "actor"):
        for key in ("bn_gamma", "bn_beta", "W"):
            for x, y in zip(a["params"][net][key], b["params"][net][key]):
                assert torch.equal(x, y), (net, key)
        assert torch.equal(a["params"][net]["b"], b["params"][net]["b"])
    for k in ("optimizer_critic", "optimizer_actor"):
        assert a[k]["iterations"] == b[k]["iterations"] == 6
        assert getattr(fresh, k).device_iterations() == 6
        for key in ("m", "v"):
            assert len(a[k][key]) == len(b[k][key]) > 0
            for x, y in zip(a[k][key], b[k][key]):
                assert x is not None and torch.equal(x, y), (k, key)
    # loading into a solver whose graphs exist writes in place: the same state, the same future
    whole.load_state_dict(sd)
    for _ in range(3):
        _iterate(whole, cfg)
    for x, y in zip(_params(whole), _params(fresh)):
        assert torch.equal(x, y)
