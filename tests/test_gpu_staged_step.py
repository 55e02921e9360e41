"""The staged rollout (k_rollout_staged, which has its own step body) against k_rollout
(DPAC_ROLLOUT_STAGED=0, Transition's arithmetic): bitwise equality of every output on starts
placed by hand so that each branch of the step runs — sampled starts may never leave the ball
in T = 0.2.

Coverage: the dw-from-memory cases launch k_rollout_staged in both dtypes, the in-kernel Philox
cases in float (all four equations here have the 2 components per lane its generator variant
needs).  The 48 float64 Philox cases are part of the required matrix but launch k_rollout both
times (the generator variant is float-only, launch_rollout's kGenOk): they pin that dispatch, they do
not exercise the staged step, and are not to be counted as coverage of it.

Start radii (start_points): the rows cycle through 17 classes from the centre to just inside R,
expressed through the horizon's own boundary-layer width c = sigma_up sqrt(3 d dt0) and its
clamp width (R - r)^2 / den < 1e-4 dt0  <=>  R - r < c / 100, so every horizon N gets inner
starts, boundary-layer starts with dt_min < dt < dt0, and clamped starts.  With the adaptive
scheme the test first asserts, on the k_rollout result of the 70-row batch, that a trajectory of
each kind is present: never rejected; rejected mid-horizon (first rejected step k with
1 <= k <= N - 2; for N < 3 any rejected step) and frozen from there on; a boundary-layer step with
dt_min < dt < dt0; a step with dt == dt_min.  tools/check_staged_starts.py checks the same on the
CPU with oracle/equations.py for the dw-from-memory cases.
"""
import os

import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import _lib, ops
from deeppde_actorcritic_amd import equation as peq
from oracle import equations as oeq
from tests.helpers import eqn_config, rel_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_TOTAL = 0.2
BATCHES = (70, 17, 1)  # several workgroups, a partial workgroup, one lane group (leading rows of the 70)
HORIZONS = (1, 15, 16, 17, 65, 130)  # the tail loop alone, a chunk -/+ 1, the 64-step ring wrapping once and twice
EQUATIONS = (("LQR", 20), ("LQR", 5), ("LQR_var", 10), ("EKN", 20))
SCHEMES = {"naive": _lib.SCHEME_NAIVE, "adaptive": _lib.SCHEME_ADAPTIVE}
SIGMA_UP = np.sqrt(2.0)  # every equation family's sigma_Up (equation.py)
# R - r of the 17 start classes: fractions of R (inner), of the layer width c, and of the clamp width c / 100
CLASSES = ([("R", f) for f in (0.95, 0.7, 0.45)] + [("c", f) for f in (0.9, 0.6, 0.35, 0.15, 0.05, 0.02)]
           + [("clamp", f) for f in (0.9, 0.6, 0.4, 0.25, 0.15, 0.08, 0.03, 0.01)])


def start_points(d, N, B, R=1.0):
    """x0 [B, d] (float64): row i at radius R - gap(class i % 17) along a fixed random direction."""
    c = SIGMA_UP * np.sqrt(3 * d * (T_TOTAL / N))
    rng = np.random.default_rng(1000 * d + N)
    x0 = np.empty((B, d))
    for i in range(B):
        kind, f = CLASSES[i % len(CLASSES)]
        gap = {"R": f * R, "c": min(f * c, 0.9 * R), "clamp": min(f * c / 100, 0.9 * R)}[kind]
        v = rng.standard_normal(d)
        x0[i] = v / np.linalg.norm(v) * (R - gap)
    return x0


def host_dw(d, N, B):
    """dw [B, d, N] (float64, the oracle's layout), a fixed stream per (d, N)."""
    return np.random.default_rng(77 * d + N).standard_normal((B, d, N))


def kinds(x, dt, coef, N, dtype):
    """Which of the four kinds of trajectory a result holds (x [N+1, B, d], dt / coef [B, N])."""
    np_t = np.float32 if dtype == torch.float32 else np.float64
    dt0, dt_min = np_t(T_TOTAL / N), np_t(T_TOTAL / N * 1e-4)
    x, dt, coef = x.cpu().numpy(), dt.cpu().numpy(), coef.cpu().numpy()
    never = bool(np.any(np.all(coef == 1, axis=1)))
    mid = False
    for b in range(coef.shape[0]):
        zeros = np.flatnonzero(coef[b] == 0)
        if zeros.size == 0:
            continue
        k = int(zeros[0])
        if N >= 3 and not 1 <= k <= N - 2:
            continue
        frozen = (np.all(coef[b, k:] == 0) and np.all(x[k + 1:, b] == x[k, b]) and np.all(dt[b, k + 1:] == dt0))
        mid = mid or bool(frozen)
    layer = bool(np.any((coef == 1) & (dt < dt0) & (dt > dt_min)))
    clamp = bool(np.any(dt == dt_min))
    return {"never rejected": never, "rejected mid-horizon and frozen": mid,
            "boundary-layer step with dt < dt0": layer, "dt clamped to dt_min": clamp}


def run_both(fn):
    """fn() under DPAC_ROLLOUT_STAGED=0 (k_rollout) and =1 (k_rollout_staged)."""
    out = {}
    old = os.environ.get("DPAC_ROLLOUT_STAGED")
    try:
        for k in ("0", "1"):
            os.environ["DPAC_ROLLOUT_STAGED"] = k
            out[k] = fn()
    finally:
        if old is None:
            os.environ.pop("DPAC_ROLLOUT_STAGED", None)
        else:
            os.environ["DPAC_ROLLOUT_STAGED"] = old
    return out["0"], out["1"]


@pytest.mark.parametrize("sampler", ["memory", "philox"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("scheme", ["adaptive", "naive"])
@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("name,d", EQUATIONS)
def test_staged_step_bitwise_on_placed_starts(name, d, N, scheme, dtype, sampler):
    cfg = eqn_config(name, d, T=T_TOTAL, N=N)
    eqp = getattr(peq, cfg.eqn_name)(cfg).params()
    sch = SCHEMES[scheme]
    Bmax = BATCHES[0]
    x0_all = torch.as_tensor(start_points(d, N, Bmax), dtype=dtype, device=DEV)
    dw_all = None
    if sampler == "memory":
        dw_all = torch.as_tensor(host_dw(d, N, Bmax), dtype=dtype, device=DEV).permute(2, 0, 1).contiguous()
    for B in BATCHES:
        x0 = x0_all[:B].contiguous()
        dw = None if dw_all is None else dw_all[:, :B].contiguous()

        def launch():
            return [ops.rollout_analytic(eqp, sch, x0, dw, T_TOTAL, N, seed=21, traj_offset=3, want_u=wu, cost_order=co)
                    for wu, co in ((False, None), (True, _lib.COST_ACTOR))]
        ref, staged = run_both(launch)
        if scheme == "adaptive" and B == Bmax:
            got = kinds(ref[0][0], ref[0][1], ref[0][2], N, dtype)
            print(f"{name} d={d} N={N} {scheme} {sampler}: {got}")
            assert all(got.values()), got
        for ra, rb in zip(ref, staged):  # x, dt, coef, u, y, disc
            assert len(ra) == len(rb)
            for ta, tb in zip(ra, rb):
                assert (ta is None) == (tb is None)
                if ta is not None:
                    assert torch.equal(ta, tb)


def test_staged_step_bench_dtype_vs_oracle():
    """The bench's dtype and scheme (float32, adaptive, LQR d = 20), B = 64, N = 200, against the
    float64 oracle with test_rollout_fp32_within_tolerance's bounds: at most 0.1 % of the
    trajectories flip an exit decision; 2e-5 (1 + |ref|) on the others' states and dt."""
    B, N = 64, 200
    cfg = eqn_config("LQR", 20, T=T_TOTAL, N=N)
    eo, ep = oeq.make(cfg), peq.LQR(cfg)
    np.random.seed(5)
    x0, dw, _ = eo.sample_normal(B, N)
    xr, dtr, cr = eo.propagate_adaptive(B, x0, dw, None, False, T_TOTAL, N, True)
    x, dt, coef, *_ = ops.rollout_analytic(
        ep.params(), _lib.SCHEME_ADAPTIVE, torch.as_tensor(x0, dtype=torch.float32, device=DEV),
        torch.as_tensor(dw, dtype=torch.float32, device=DEV).permute(2, 0, 1).contiguous(), T_TOTAL, N)
    same = np.all(coef.cpu().numpy() == cr.numpy(), axis=1)
    assert np.mean(~same) <= 1e-3, f"{np.mean(~same):.2e} of trajectories flipped an exit decision"
    assert rel_close(x.permute(1, 2, 0).cpu().double().numpy()[same], xr.numpy()[same], 2e-5)
    assert rel_close(dt.cpu().double().numpy()[same], dtr.numpy()[same], 2e-5)
