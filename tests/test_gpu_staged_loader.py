"""The staged rollout's loader (k_rollout_staged, dw from memory) against k_rollout
(DPAC_ROLLOUT_STAGED=0): every output bit for bit.

The loader wavefront copies a full workgroup's whole chunks (16 steps) with unpredicated DMA
pieces at incrementally formed addresses, the last piece of a step with only the lanes its rows
fill; a partial workgroup, and the last chunk of a horizon that is no multiple of 16, take the
predicated path.  The shapes are the smallest that select each path and their mixtures:

  * batches: a multiple of the workgroup's trajectories (every workgroup full), one workgroup
    short of a row (only the predicated path), and full workgroups followed by a partial one in
    the same launch.  LQR d = 20 has 16 trajectories per workgroup, d = 10 has 32, d = 5 has 64;
  * horizons: below one chunk, a chunk -/+ 1, two chunks -/+ 1, the float ring of 64 steps
    wrapping (63 .. 65) and wrapping twice with a clamped last chunk (129); in float64 (three
    pieces per step at d = 20, a ring of 48 steps) also 47 .. 49 and 97;
  * float32 and float64, the adaptive scheme throughout and the naive scheme at one shape;
  * another slot shape: d = 7 (1792-byte slots, a last piece of 48 lanes), if its dimension
    plugin is beside the library;
  * the bench's launch (B = 4096, N = 200, float32), once.

Starts and increments are those of tests/test_gpu_staged_step.py.
"""
import os

import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import _lib, ops
from deeppde_actorcritic_amd import equation as peq
from tests.helpers import eqn_config
from tests.test_gpu_staged_step import SCHEMES, T_TOTAL, host_dw, run_both, start_points

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCHES = {20: (16, 32, 15, 33, 49), 5: (64, 65), 10: (32, 40), 7: (64, 70)}
HORIZONS = (1, 15, 16, 17, 31, 33, 63, 64, 65, 129)
HORIZONS_F64 = (47, 48, 49, 97)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
CASES = ([(d, "f32", N) for d in (20, 5, 10) for N in HORIZONS]
         + [(d, "f64", N) for d in (20, 5, 10) for N in HORIZONS + HORIZONS_F64])


def check_bitwise(d, dtype, N, scheme, batches):
    """LQR at dimension d: every batch of `batches` (leading rows of the largest), with and
    without the u output, staged against k_rollout."""
    cfg = eqn_config("LQR", d, T=T_TOTAL, N=N)
    eqp = peq.LQR(cfg).params()
    Bmax = max(batches)
    x0_all = torch.as_tensor(start_points(d, N, Bmax), dtype=dtype, device=DEV)
    dw_all = torch.as_tensor(host_dw(d, N, Bmax), dtype=dtype, device=DEV).permute(2, 0, 1).contiguous()
    for B in batches:
        x0 = x0_all[:B].contiguous()
        dw = dw_all[:, :B].contiguous()

        def launch():
            return [ops.rollout_analytic(eqp, SCHEMES[scheme], x0, dw, T_TOTAL, N, want_u=wu) for wu in (False, True)]
        ref, staged = run_both(launch)
        assert_same(ref, staged, f"d={d} N={N} B={B} {scheme}")


def assert_same(ref, staged, what):
    assert len(ref) == len(staged)
    for ra, rb in zip(ref, staged):  # x, dt, coef, u, y, disc
        assert len(ra) == len(rb)
        for i, (ta, tb) in enumerate(zip(ra, rb)):
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert torch.equal(ta, tb), f"{what}: output {i} differs"


@pytest.mark.parametrize("d,dt,N", CASES)
def test_staged_loader_bitwise(d, dt, N):
    check_bitwise(d, DTYPES[dt], N, "adaptive", BATCHES[d])


def test_staged_loader_bitwise_naive():
    check_bitwise(20, torch.float32, 65, "naive", BATCHES[20])


def test_staged_loader_bitwise_d7():
    """1792-byte slots: the last piece of a step has 48 lanes."""
    _lib.load()
    if not any(os.path.basename(p) == "libdpac_d7.so" for p in _lib.dim_plugins()):
        pytest.skip("the d = 7 dimension plugin is not built")
    check_bitwise(7, torch.float32, 65, "adaptive", BATCHES[7])


def test_staged_loader_bitwise_bench_shape():
    """The bench's launch: LQR d = 20, float, adaptive, B = 4096, N = 200, every workgroup full."""
    d, N, B = 20, 200, 4096
    cfg = eqn_config("LQR", d, T=T_TOTAL, N=N)
    eqp = peq.LQR(cfg).params()
    x0 = torch.as_tensor(start_points(d, N, B), dtype=torch.float32, device=DEV)
    dw = torch.as_tensor(np.random.default_rng(4096).standard_normal((N, B, d)), dtype=torch.float32, device=DEV)
    ref, staged = run_both(lambda: [ops.rollout_analytic(eqp, _lib.SCHEME_ADAPTIVE, x0, dw, T_TOTAL, N)])
    assert_same(ref, staged, "bench shape")
