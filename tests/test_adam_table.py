"""CPU: the alpha table dpac_adam_step reads (solver.adam_alpha_table) against the host scalars
it replaces (solver.tf_adam_scalars), compared as bits, and the entry point's host validation.

The table's entry t-1 is the alpha of step t; it ends at the first step past the schedule's
last boundary from which alpha is T(values[-1]) for good, so the kernel's clamped index gives
every later step's alpha exactly.
"""
import ctypes

import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import _lib
from deeppde_actorcritic_amd import solver as psol

SCHEDULE = psol.PiecewiseConstantDecay([2, 4], [1e-3, 5e-4, 1e-4])


def _bits(x, dtype):
    f, u = (np.float32, np.uint32) if dtype == torch.float32 else (np.float64, np.uint64)
    return np.asarray(x, dtype=f).view(u)


def _check_table(schedule, b1, b2, dtype):
    tab = psol.adam_alpha_table(schedule, b1, b2, dtype)
    assert tab is not None and tab.ndim == 1
    assert tab.dtype == (np.float32 if dtype == torch.float32 else np.float64)
    n = len(tab)
    assert n >= max(schedule.boundaries) + 2  # past the last boundary: schedule(t-1) is the last value
    want = [psol.tf_adam_scalars(schedule(t - 1), t, b1, b2, dtype)[0] for t in range(1, n + 1)]
    assert np.array_equal(_bits(tab, dtype), _bits(want, dtype))
    assert _bits(tab[-1], dtype) == _bits(schedule.values[-1], dtype)
    for past in (10, 10 ** 6):  # the clamped index loses nothing
        a = psol.tf_adam_scalars(schedule(n + past - 1), n + past, b1, b2, dtype)[0]
        assert _bits(a, dtype) == _bits(tab[-1], dtype), (past, a, tab[-1])
    return tab


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_table_matches_the_host_scalars(dtype):
    tab = _check_table(SCHEDULE, 0.9, 0.999, dtype)
    # beta_2^t drops below half an ulp of 1 after ~1.7e4 (float32) / ~3.7e4 (float64) steps
    assert 10 ** 4 < len(tab) < 5 * 10 ** 4
    assert psol.adam_alpha_table(SCHEDULE, 0.9, 0.999, dtype) is tab  # cached per schedule and dtype


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_table_saturates_early_with_small_betas(dtype):
    tab = _check_table(SCHEDULE, 0.5, 0.5, dtype)
    assert len(tab) < 100


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_table_is_capped(dtype):
    """beta_2 within 1e-7 of 1: alpha keeps moving for more than 2^22 steps, so there is no
    table and the optimizer keeps the host path."""
    assert psol.adam_alpha_table(SCHEDULE, 0.9, 0.9999999, dtype) is None
    opt = psol.TFAdam(SCHEDULE, beta_2=0.9999999)
    assert opt.device_ready(torch.zeros(1, dtype=dtype)) is False


def test_adam_step_validation_without_gpu():
    """dpac_adam_step rejects a NULL state, a NULL table, an empty table and a bad dtype on the
    host, before any HIP call."""
    d = ctypes.c_void_p(0x1000)
    arr = (ctypes.c_void_p * 1)(0x1000)
    numel = (ctypes.c_int64 * 1)(4)
    ok = dict(dtype=_lib.F32, state=d, table=d, table_len=8)
    cases = [(dict(ok, state=None), "state"), (dict(ok, table=None), "alpha_table"),
             (dict(ok, table_len=0), "table_len"), (dict(ok, dtype=7), "dtype")]
    for n in (0, 1):
        for kw, word in cases:
            with pytest.raises(_lib.DpacError) as ei:
                _lib.call("dpac_adam_step", kw["dtype"], n, numel, arr, arr, arr, arr, kw["state"],
                          kw["table"], kw["table_len"], 0.9, 0.999, 1e-8, 1, None)
            assert ei.value.code == _lib.DPAC_EINVAL, (kw, ei.value)
            assert word in str(ei.value), (word, str(ei.value))
    # dpac_adam_apply's checks
    bad = (ctypes.c_int64 * 1)(0)
    for args in ((-1, numel, arr), (1, None, arr), (1, bad, arr), (1, numel, None)):
        with pytest.raises(_lib.DpacError) as ei:
            _lib.call("dpac_adam_step", _lib.F32, args[0], args[1], args[2], arr, arr, arr, d, d, 8,
                      0.9, 0.999, 1e-8, 0, None)
        assert ei.value.code == _lib.DPAC_EINVAL
    assert _lib.ABI_VERSION == 10 == _lib.load().dpac_abi_version()
