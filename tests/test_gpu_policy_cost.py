"""GPU: policy evaluation (dpac_policy_cost, ops.policy_cost, ActorCriticSolver.evaluate_policy):
the lean modes of the three fused NN rollout kernels, which keep no trajectory array and can
draw their increments in-kernel.

  1. lean == full, bitwise, on every kernel path (float64 generic, float32 4-row, generic 16-row,
     FAST, split-fp16), with dw read and with dw drawn in-kernel from dpac_sample's stream;
  2. sharding by traj_offset is bitwise;
  3. the split-fp16 range guard: the status word is set and the guarded f32 launch rewrites every
     lean output; in range the split-fp16 and f32 lean results agree as the full kernels' do;
  4. a batch beyond what the [N+1][B][d] descriptor of the full path can address;
  5. evaluate_policy against the same quantities formed from sample + rollout_nn + NN_value.
"""
import numpy as np
import pytest
import torch

from deeppde_actorcritic_amd import _lib, ops
from deeppde_actorcritic_amd import equation as peq
from deeppde_actorcritic_amd import solver as psol
from deeppde_actorcritic_amd.config import set_floatx
from tests.helpers import full_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCHEMES = {"naive": _lib.SCHEME_NAIVE, "adaptive": _lib.SCHEME_ADAPTIVE}
F32, F64 = torch.float32, torch.float64
# kernel path -> (dtype, per-launch environment switches)
PATHS = {"f64": (F64, {}),
         "nn4": (F32, {}),                                             # the default at B <= 1024
         "gen16": (F32, {"DPAC_NN_TILE": "16"}),                       # with a network off the fast shape
         "fast": (F32, {"DPAC_NN_TILE": "16", "DPAC_NN_X3": "0"}),
         "x3": (F32, {"DPAC_NN_TILE": "16"})}
WIDE = (200, 200, 200)


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for k in ("DPAC_NN_TILE", "DPAC_NN_FAST", "DPAC_NN_X3", "DPAC_NX_ROWS", "DPAC_WEIGHT_KM", "DPAC_MLP_MATH"):
        monkeypatch.delenv(k, raising=False)
    ops.x3_status_reset(DEV)
    yield
    ops.x3_status_reset(DEV)
    set_floatx("float64")


def _setup(name, d, hidden, dtype, scheme="adaptive", N=21, T=1.0):
    cfg = full_config(name, d, T=T, N=N, hidden=hidden, scheme=scheme,
                      dtype="float64" if dtype == F64 else "float32")
    set_floatx(cfg.net_config.dtype)
    eqp = getattr(peq, name)(cfg.eqn_config).params()
    net = psol.DeepNN(cfg, "actor", torch.Generator().manual_seed(3), dtype, DEV)
    return eqp, net


def _use(monkeypatch, path):
    dtype, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dtype


def _lean(eqp, sch, x0, dw, T, N, view, **kw):
    return ops.policy_cost(eqp, sch, x0, dw, T, N, view, want_tau=True, want_steps=True, **kw)


# (equation, d, hidden, kernel paths, sample types)
_FOUR = ("f64", "nn4", "fast", "x3")
EQUAL_CASES = [("LQR", 20, WIDE, _FOUR, ("normal", "bounded")),
               ("LQR_var", 10, WIDE, _FOUR, ("normal",)),   # sigma depends on x and u
               ("EKN", 20, WIDE, _FOUR, ("normal",)),       # the Eikonal head: 21 outputs
               ("VDP", 20, WIDE, _FOUR, ("normal",)),       # one-lane groups: the non-paired stream
               ("LQR", 20, (40, 40), ("gen16",), ("normal",)),
               ("LQR", 5, (16, 16), ("f64", "gen16"), ("normal",)),
               ("VDP", 4, (50, 50), ("f64", "gen16"), ("normal",)),
               ("LQR", 7, (16, 16), ("f64", "nn4"), ("normal",))]  # the d = 7 dimension plugin
EQUAL_PARAMS = [(n, d, h, p, k, s) for n, d, h, ps, ks in EQUAL_CASES for p in ps for k in ks
                for s in ("adaptive", "naive")]


@pytest.mark.parametrize("name,d,hidden,path,kind,scheme", EQUAL_PARAMS)
def test_lean_equals_full_bitwise(name, d, hidden, path, kind, scheme, monkeypatch):
    """B = 37: a partial 4-row group and a partial 16-row tile; N = 21: an odd horizon, so the
    paired Philox layout ends on an unpaired step."""
    B, N, T = 37, 21, 1.0
    dtype = _use(monkeypatch, path)
    eqp, net = _setup(name, d, hidden, dtype, scheme, N, T)
    sch, st = SCHEMES[scheme], peq.SAMPLE_TYPES[kind]
    x0, dw, _ = ops.sample(eqp, st, B, N, seed=9, traj_offset=123, dtype=dtype, device=DEV)
    view = net.mlp_view()
    x, dt, coef, _, y, disc, _ = ops.rollout_nn(eqp, sch, x0, dw, T, N, view, want_u=False,
                                                cost_order=_lib.COST_ACTOR)
    with_dw = _lean(eqp, sch, x0, dw, T, N, view)
    drawn = _lean(eqp, sch, x0, None, T, N, view, seed=9, traj_offset=123, sample_type=st)
    torch.cuda.synchronize()
    if path == "x3":
        assert view.status is not None and not ops.x3_fell_back(DEV)
    steps_ref = coef.sum(1).to(torch.int32)
    tau_ref = (coef.double() * dt.double()).sum(1)
    eps = 2.0 ** -52 if dtype == F64 else 2.0 ** -23
    early = int((steps_ref < N).sum())
    print(f"\n[lean {name} d={d} {path} {kind} {scheme}] {early} of {B} paths stop early")
    for tag, (ly, ldisc, lx, ltau, lsteps) in (("dw", with_dw), ("philox", drawn)):
        assert torch.equal(ly, y), tag
        assert torch.equal(ldisc, disc), tag
        assert torch.equal(lx, x[N]), tag
        assert torch.equal(lsteps, steps_ref), tag
        # N sequential additions at one unit roundoff each, with a factor of two
        assert bool(((ltau.double() - tau_ref).abs() <= N * eps * tau_ref).all()), tag
    if scheme == "adaptive":  # non-vacuity: some paths stop early, not all
        assert 1 <= early <= B - 1


@pytest.mark.parametrize("path", ["f64", "nn4", "x3"])
def test_sharding_by_traj_offset_is_bitwise(path, monkeypatch):
    B, cut, N, T, off = 101, 19, 21, 1.0, 1000
    dtype = _use(monkeypatch, path)
    eqp, net = _setup("LQR", 20, WIDE, dtype, "adaptive", N, T)
    x0, _, _ = ops.sample(eqp, _lib.SAMPLE_NORMAL, B, N, seed=4, dtype=dtype, device=DEV, want_dw=False)
    view = net.mlp_view()
    sch = _lib.SCHEME_ADAPTIVE
    whole = _lean(eqp, sch, x0, None, T, N, view, seed=5, traj_offset=off)
    head = _lean(eqp, sch, x0[:cut].contiguous(), None, T, N, view, seed=5, traj_offset=off)
    tail = _lean(eqp, sch, x0[cut:].contiguous(), None, T, N, view, seed=5, traj_offset=off + cut)
    for a, h, t in zip(whole, head, tail):
        assert torch.equal(a, torch.cat([h, t]))
    assert 1 <= int((whole[4] < N).sum()) <= B - 1


def test_range_guard_rewrites_every_lean_output(monkeypatch):
    """One hidden BN shift of 4e4 (>= 2^15, the split-fp16 range): the x3 lean kernel sets the
    status word and the guarded exact-f32 lean launch rewrites y, disc, x_end, tau and steps."""
    B, N, T = 37, 21, 1.0
    _use(monkeypatch, "x3")
    eqp, net = _setup("LQR", 20, WIDE, F32, "adaptive", N, T)
    with torch.no_grad():
        net.bn_beta[2][0] = 4.0e4
    sch = _lib.SCHEME_ADAPTIVE
    x0, dw, _ = ops.sample(eqp, _lib.SAMPLE_NORMAL, B, N, seed=9, dtype=F32, device=DEV)
    view = net.mlp_view()
    assert view.status is not None
    monkeypatch.setenv("DPAC_NN_X3", "0")
    ref = [_lean(eqp, sch, x0, dw, T, N, view), _lean(eqp, sch, x0, None, T, N, view, seed=9)]
    assert not ops.x3_fell_back(DEV)
    monkeypatch.delenv("DPAC_NN_X3")
    for r, w in zip(ref, (dw, None)):
        ops.x3_status_reset(DEV)
        got = _lean(eqp, sch, x0, w, T, N, view, seed=9)
        assert ops.x3_fell_back(DEV)
        for a, b in zip(got, r):
            assert torch.isfinite(a.double()).all()
            assert torch.equal(a, b)


def test_in_range_x3_lean_agrees_with_f32_lean(monkeypatch):
    """With the word clear: the split-fp16 and the FAST lean kernels within the tolerance
    tests/test_gpu_nn_x3.py uses for the forward (<= 1e-3 of the paths may flip an exit decision;
    matched paths within 2e-5 (1 + |b|))."""
    B, N, T = 1037, 21, 1.0
    _use(monkeypatch, "x3")
    eqp, net = _setup("LQR", 20, WIDE, F32, "adaptive", N, T)
    sch = _lib.SCHEME_ADAPTIVE
    x0, _, _ = ops.sample(eqp, _lib.SAMPLE_NORMAL, B, N, seed=41, dtype=F32, device=DEV, want_dw=False)
    view = net.mlp_view()
    a = _lean(eqp, sch, x0, None, T, N, view, seed=41)
    assert not ops.x3_fell_back(DEV)
    monkeypatch.setenv("DPAC_NN_X3", "0")
    b = _lean(eqp, sch, x0, None, T, N, view, seed=41)
    assert not torch.equal(a[0], b[0]), "the x3 path did not run (bitwise the f32 kernel)"
    same = a[4] == b[4]
    flips = float((~same).double().mean())
    print(f"\n[x3 lean vs f32 lean] flips {flips:.2e}")
    assert flips <= 1e-3
    for u, v in zip(a[:4], b[:4]):
        err = float(((u[same] - v[same]).abs() / (1 + v[same].abs())).max())
        assert err <= 2e-5, err


def test_beyond_the_trajectory_arrays_limit():
    """B = 600 000 at lqr_d20, N = 100, float32: x [N+1, B, d] would take 4.8 GB, past the 32-bit
    descriptor of the full path; the lean call keeps about 100 MB.  Both slices are above 1024
    rows, so they run the large call's kernel."""
    B, N, T, K = 600_000, 100, 1.0, 2048
    eqp, net = _setup("LQR", 20, WIDE, F32, "adaptive", N, T)
    sch = _lib.SCHEME_ADAPTIVE
    x0, _, _ = ops.sample(eqp, _lib.SAMPLE_NORMAL, B, N, seed=2, dtype=F32, device=DEV, want_dw=False)
    view = net.mlp_view()
    big = _lean(eqp, sch, x0, None, T, N, view, seed=6)
    for t in big:
        assert bool(torch.isfinite(t.double()).all())
    head = _lean(eqp, sch, x0[:K].contiguous(), None, T, N, view, seed=6)
    tail = _lean(eqp, sch, x0[B - K:].contiguous(), None, T, N, view, seed=6, traj_offset=B - K)
    for a, h, t in zip(big, head, tail):
        assert torch.equal(a[:K], h)
        assert torch.equal(a[B - K:], t)


def _close(a, b, rtol=1e-12):
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a - b).abs() <= rtol * b.abs()).all())


@pytest.mark.parametrize("scheme,T", [("naive", 0.2), ("adaptive", 1.0)])
def test_evaluate_policy(scheme, T):
    """Under the naive scheme at T = 0.2 a path moves by |dx|^2 ~ 2 d T / N = 0.095 per step, so
    from |x0| = 0.42 .. 0.86 some of the 256 paths leave the unit ball and some do not."""
    S, P, N = 3, 256, 21
    cfg = full_config("LQR", 5, T=T, N=N, hidden=(16, 16), scheme=scheme, dtype="float64")
    bp = peq.LQR(cfg.eqn_config)
    sol = psol.ActorCriticSolver(cfg, bp, seed=1)
    eqp = bp.params()
    x0 = np.array([[0.1, -0.2, 0.3, 0.0, 0.2], [0.5, 0.5, -0.4, 0.1, 0.0], [0.0, 0.0, 0.05, -0.8, 0.3]])
    calls = sol._calls
    ev = sol.evaluate_policy(x0, P, seed=77)
    assert sol._calls == calls and ev.num_paths == P
    # the same quantities from sample + rollout_nn + NN_value on the same keys (row g = s P + k)
    rep = torch.as_tensor(x0, device=DEV).repeat_interleave(P, 0)
    _, dw, _ = ops.sample(eqp, _lib.SAMPLE_NORMAL, S * P, N, seed=77, dtype=F64, device=DEV)
    with torch.no_grad():
        x, dt, coef, _, y, disc, _ = ops.rollout_nn(eqp, SCHEMES[scheme], rep, dw, T, N,
                                                    sol.model_actor.NN_control.mlp_view(), want_u=False,
                                                    cost_order=_lib.COST_ACTOR)
        terms = {"critic": sol.model_critic.NN_value(x[N])[:, 0], "true": ops.v_true(eqp, x[N]),
                 "none": torch.zeros_like(y)}
    tau = (coef * dt).sum(1).view(S, P).mean(1)
    exits = (coef.sum(1) < N).double().view(S, P).mean(1)
    print(f"\n[evaluate_policy {scheme}] exit fractions {exits.tolist()}")
    if scheme == "naive":
        assert 0 < float(exits.sum()) < S
    for name, term in terms.items():
        got = ev if name == "critic" else sol.evaluate_policy(x0, P, seed=77, terminal=name)
        c = (y + term * disc).view(S, P)
        assert _close(got.cost, c.mean(1)), name
        assert _close(got.stderr, (c.var(1, unbiased=True) / P).sqrt()), name
        assert _close(got.mean_tau, tau) and _close(got.exit_frac, exits), name
        # only the terminal term changes (the moments are summed with atomics: tau to rounding)
        assert _close(got.mean_tau, ev.mean_tau) and torch.equal(got.exit_frac, ev.exit_frac)
    small = sol.evaluate_policy(torch.as_tensor(x0), P, seed=77, chunk_rows=100)
    for a, b in zip(small[:4], ev[:4]):
        assert _close(a, b)
    fresh = sol.evaluate_policy(x0, P)  # a key of the solver's own: another sample, same state
    assert sol._calls == calls and not torch.equal(fresh.cost, ev.cost)
    deep = full_config("LQR", 5, T=T, N=N, hidden=(8,) * 5, dtype="float64")
    with pytest.raises(ValueError):
        psol.ActorCriticSolver(deep, peq.LQR(deep.eqn_config), seed=1).evaluate_policy(x0, 4)
    with pytest.raises(ValueError):
        bp.policy_cost(scheme, rep, T, N, psol.DeepNN(deep, "actor", None, F64, DEV))
