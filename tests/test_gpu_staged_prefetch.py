"""The staged rollout's chunk reads (k_rollout_staged: a hand-off chunk's dw read into registers
at the chunk's top, the last N % 16 steps as unrolled pieces of 8, 4, 2 and 1) against k_rollout
(DPAC_ROLLOUT_STAGED=0): every output bit for bit.

Horizons: below one chunk (1, 7, 8, 9, 15: the remainder pieces alone, each piece and several
combinations), one chunk exactly and +/- 1, 24 .. 33 (two chunks, with and without a
remainder), 47 .. 49 (the float64 ring of 48 steps wraps), 63 .. 65 (the float ring of 64 steps
wraps), 97, 130 and 200 (several wraps; the remainders 1, 2 and 8).  Batches: several
workgroups, a partial workgroup, one lane group.  Equations: LQR d = 20 (one vector read per
step), LQR d = 5 (scalar reads), EKN d = 20 (the step reads r).  The in-kernel Philox variant
(generator wavefronts in the loader's place) runs in float only.  Each case launches three
times: with x, dt and coef alone and with the u output as well (both take the chunk reads when
dw comes from memory), and with the u and cost outputs (these instantiations, and the Philox
variant's, keep the one-step read-ahead and the rolled remainder loop).

The starts are those of tests/test_gpu_staged_step.py, placed so that trajectories are rejected
mid-horizon and take boundary-layer steps; with the adaptive scheme the test first asserts on the
k_rollout result of the 70-row batch that both kinds are present.
"""
import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import _lib, ops
from deeppde_actorcritic_amd import equation as peq
from tests.helpers import eqn_config
from tests.test_gpu_staged_step import BATCHES, SCHEMES, T_TOTAL, host_dw, kinds, run_both, start_points

pytestmark = pytest.mark.gpu
DEV = "cuda"
HORIZONS = (1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97, 130, 200)
EQUATIONS = (("LQR", 20), ("LQR", 5), ("EKN", 20))
VARIANTS = {"memory-f32": ("memory", torch.float32), "memory-f64": ("memory", torch.float64),
            "philox-f32": ("philox", torch.float32)}
NEEDED = ("rejected mid-horizon and frozen", "boundary-layer step with dt < dt0")
assert BATCHES == (70, 17, 1)


def assert_same(ref, staged):
    """Two lists of rollout results (x, dt, coef, u, y, disc), equal bit for bit."""
    assert len(ref) == len(staged)
    for ra, rb in zip(ref, staged):
        assert len(ra) == len(rb)
        for ta, tb in zip(ra, rb):
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert torch.equal(ta, tb)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("scheme", ["adaptive", "naive"])
@pytest.mark.parametrize("N", HORIZONS)
@pytest.mark.parametrize("name,d", EQUATIONS)
def test_staged_prefetch_bitwise(name, d, N, scheme, variant):
    sampler, dtype = VARIANTS[variant]
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
                    for wu, co in ((False, None), (True, None), (True, _lib.COST_ACTOR))]
        ref, staged = run_both(launch)
        if scheme == "adaptive" and B == Bmax:
            got = kinds(ref[0][0], ref[0][1], ref[0][2], N, dtype)
            print(f"{name} d={d} N={N} {scheme} {variant}: {got}")
            assert all(got[k] for k in NEEDED), got
        assert_same(ref, staged)


def test_staged_prefetch_bitwise_bench_shape():
    """The bench's launch: LQR d = 20, float, adaptive, B = 4096 (one compute wavefront per SIMD),
    N = 200, dw from memory, no cost or u outputs."""
    d, N, B = 20, 200, 4096
    cfg = eqn_config("LQR", d, T=T_TOTAL, N=N)
    eqp = peq.LQR(cfg).params()
    x0 = torch.as_tensor(start_points(d, N, B), dtype=torch.float32, device=DEV)
    dw = torch.as_tensor(np.random.default_rng(4096).standard_normal((N, B, d)), dtype=torch.float32, device=DEV)
    ref, staged = run_both(lambda: [ops.rollout_analytic(eqp, _lib.SCHEME_ADAPTIVE, x0, dw, T_TOTAL, N)])
    got = kinds(ref[0][0], ref[0][1], ref[0][2], N, torch.float32)
    assert all(got[k] for k in NEEDED), got
    assert_same(ref, staged)
