"""CPU: dpac_policy_cost (include/dpac.h) validates its arguments on the host, before any device
work, and is an additive entry point of ABI version 10."""
import ctypes

import pytest

from deeppde_actorcritic_amd import _lib


def _params(dim=20):
    p = _lib.EqnParams()
    p.eqn, p.dim, p.control_dim = _lib.EQN_LQR, dim, dim
    p.gamma, p.R, p.sigma_up, p.p, p.q, p.beta, p.k = 1.0, 1.0, 2 ** 0.5, 1.0, 1.0, 1.0, 0.618
    return p


def _net(d, n_hidden=1, hidden=32):
    """A dpac_mlp with dummy (never dereferenced) pointers: host validation only."""
    n = _lib.Mlp()
    n.n_hidden = n_hidden
    n.width[0] = d
    for i in range(1, max(n_hidden, 1) + 1):
        n.width[i] = hidden
    n.width[max(n_hidden, 1) + 1] = d
    for i in range(_lib.MLP_MAX_HIDDEN + 2):
        n.bn_scale[i] = n.bn_shift[i] = 0x1000
    for i in range(_lib.MLP_MAX_HIDDEN + 1):
        n.weight[i] = 0x1000
    n.bias = 0x1000
    return n


DUMMY = ctypes.c_void_p(0x1000)


def _args(**kw):
    """The arguments of a valid call (dummy pointers), with the named ones replaced."""
    a = dict(eq=_params(), scheme=_lib.SCHEME_ADAPTIVE, dtype=_lib.F32, num_sample=16, num_steps=10,
             total_time=0.2, actor=_net(20), x0=DUMMY, dw=DUMMY, seed=1, traj_offset=0,
             sample_type=_lib.SAMPLE_NORMAL, cost_order=_lib.COST_ACTOR, y=DUMMY, disc=DUMMY,
             x_end=DUMMY, tau=None, steps=None, stream=None)
    a.update(kw)
    a["eq"], a["actor"] = ctypes.byref(a["eq"]), ctypes.byref(a["actor"])
    return tuple(a.values())


CASES = [
    ("null y", dict(y=None), "'y'"),
    ("null disc", dict(disc=None), "'disc'"),
    ("null x_end", dict(x_end=None), "'x_end'"),
    ("bad scheme", dict(scheme=7), "scheme"),
    ("bad cost_order", dict(cost_order=5), "cost_order"),
    ("in-kernel noise, bad sample_type", dict(dw=None, sample_type=9), "sample_type"),
    ("in-kernel noise, negative traj_offset", dict(dw=None, traj_offset=-1), "traj_offset"),
    ("no hidden layer", dict(actor=_net(20, n_hidden=0)), "n_hidden"),
    # [B][d] float32 at exactly 4 GiB (B = 2^28, d = 4), and over it in float64
    ("[B][d] at 4 GiB", dict(eq=_params(4), actor=_net(4), num_sample=1 << 28, dw=None), "4 GiB"),
    ("[B][d] over 4 GiB", dict(eq=_params(4), actor=_net(4), num_sample=1 << 28, dw=None,
                               dtype=_lib.F64), "4 GiB"),
]


@pytest.mark.parametrize("what,kw,word", CASES, ids=[c[0] for c in CASES])
def test_policy_cost_rejects(what, kw, word):
    with pytest.raises(_lib.DpacError) as ei:
        _lib.call("dpac_policy_cost", *_args(**kw))
    assert ei.value.code == _lib.DPAC_EINVAL, (what, ei.value)
    assert word.lower() in str(ei.value).lower(), (what, str(ei.value))


def test_policy_cost_is_additive_to_abi_10():
    lib = _lib.load()
    assert lib.dpac_abi_version() == 10 == _lib.ABI_VERSION
    assert hasattr(lib, "dpac_policy_cost")
    assert "dpac_policy_cost" in _lib.exported_symbols()
