"""The optimizer: tf.keras Adam + PiecewiseConstantDecay (solver.py:16-21), with TensorFlow's
arithmetic, and its alpha schedule as a device table (dpac_adam_step)."""
import numpy as np
import torch

from . import ops


class PiecewiseConstantDecay:
    def __init__(self, boundaries, values):
        if len(values) != len(boundaries) + 1:
            raise ValueError("values must have one more entry than boundaries")
        self.boundaries, self.values = list(boundaries), list(values)

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


def tf_adam_scalars(lr, t, b1, b2, dtype):
    """ResourceApplyAdam's scalars in the variables' dtype T, as TF forms them (Keras
    Adam casts lr, beta_1, beta_2 to T, beta_i_power = pow(beta_i, t) in T; the op computes
    alpha = lr * sqrt(T(1) - beta2_power) / (T(1) - beta1_power) and T(1) - beta_i in T):
    (alpha, 1 - b1, 1 - b2) as Python floats holding T values."""
    f = np.float32 if dtype == torch.float32 else np.float64
    one, b1t, b2t = f(1), f(b1), f(b2)
    b1p, b2p = np.power(b1t, f(t)), np.power(b2t, f(t))
    alpha = f(lr) * np.sqrt(one - b2p) / (one - b1p)
    return float(alpha), float(one - b1t), float(one - b2t)


ADAM_TABLE_CAP = 1 << 22  # entries; betas whose table would be longer keep the host path

_ALPHA_TABLES = {}


def _alpha_saturated(t, b1, b2, dtype):
    """Whether both bias corrections of step t round to exactly 1 in the variables' dtype
    (T(1) - beta_i^t == T(1)): then alpha == T(lr), and since beta_i^t only shrinks, for every
    later step too."""
    f = np.float32 if dtype == torch.float32 else np.float64
    one = f(1)
    return bool(one - np.power(f(b1), f(t)) == one and one - np.power(f(b2), f(t)) == one)


def adam_alpha_table(schedule, beta_1, beta_2, dtype):
    """The alphas dpac_adam_step reads, as a numpy array in the variables' dtype: entry t-1 is
    tf_adam_scalars(schedule(t-1), t, ...)[0], up to the first t that is past the schedule's last
    boundary and at which alpha == T(values[-1]) for good (_alpha_saturated), so that clamping
    the index at the table's end gives every later step's alpha exactly.  None when that takes
    more than ADAM_TABLE_CAP entries (betas within an ulp of 1).  A pure host function."""
    f = np.float32 if dtype == torch.float32 else np.float64
    key = (tuple(schedule.boundaries), tuple(schedule.values), float(beta_1), float(beta_2), f)
    if key in _ALPHA_TABLES:
        return _ALPHA_TABLES[key]
    first = (max(schedule.boundaries) + 2) if schedule.boundaries else 1  # schedule(t-1) is the last value
    table = None
    if first <= ADAM_TABLE_CAP and _alpha_saturated(ADAM_TABLE_CAP, beta_1, beta_2, dtype):
        out, t = [], 1
        while True:
            out.append(tf_adam_scalars(schedule(t - 1), t, beta_1, beta_2, dtype)[0])
            if t >= first and _alpha_saturated(t, beta_1, beta_2, dtype):
                break
            t += 1
        table = np.asarray(out, dtype=f)
        table.setflags(write=False)
    _ALPHA_TABLES[key] = table
    return table


class TFAdam:
    """Adam with TensorFlow's update (ResourceApplyAdam):
        alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
        m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  var -= m*alpha / (sqrt(v) + eps)
    every scalar formed in the variables' dtype (tf_adam_scalars);
    lr = schedule(iterations) before the increment, t = iterations + 1.  None
    gradients are skipped (Keras filters them), iterations still advance.

    device_schedule (default): on the GPU the step count also lives in device memory and alpha
    comes from a device table (dpac_adam_step reads it from adam_alpha_table's), so a step can be
    captured in a HIP graph (launch()) and follows the schedule under replay; `iterations` stays
    the host's count, advanced by apply_gradients or, for a replayed step, by the caller.
    False: the schedule and the bias correction on the host, alpha passed by value to
    dpac_adam_apply (the earlier path, and the bitwise reference of the device one)."""

    def __init__(self, schedule, beta_1=0.9, beta_2=0.999, epsilon=1e-8, device_schedule=True):
        self.schedule, self.b1, self.b2, self.eps = schedule, beta_1, beta_2, epsilon
        self.device_schedule = device_schedule
        self.iterations = 0
        self.state = {}
        self._dev = None    # ops.adam_state() once a step ran on the GPU (device_schedule)
        self._snap = None   # a copy of it made by snapshot(), for a part of a step on another stream
        self._table = None  # adam_alpha_table on that device; False: no table, host path

    def device_ready(self, like) -> bool:
        """Make the device counter (from the host count) and the alpha table on `like`'s device
        in its dtype, once; False when the step stays on the host path (no device_schedule, or
        betas without a table)."""
        if not self.device_schedule or self._table is False:
            return False
        if self._table is None:
            tab = adam_alpha_table(self.schedule, self.b1, self.b2, like.dtype)
            if tab is None:
                self._table = False
                return False
            self._table = torch.from_numpy(tab.copy()).to(like.device)
            self._dev = ops.adam_state(like.device)
            self._dev[0] = self.iterations
            self._snap = self._dev.clone()
        elif self._table.dtype != like.dtype or self._table.device != like.device:
            raise TypeError("TFAdam: the variables changed dtype or device")
        return True

    def _gather(self, grads_and_vars):
        gs, vs, ms, ss = [], [], [], []
        for g, v in grads_and_vars:
            if g is None:
                continue
            st = self.state.get(v)
            if st is None:
                st = self.state[v] = (torch.zeros_like(v), torch.zeros_like(v))
            gs.append(g); vs.append(v); ms.append(st[0]); ss.append(st[1])
        return gs, vs, ms, ss

    @torch.no_grad()
    def prepare(self, grads_and_vars) -> bool:
        """Everything launch() needs that must not be made inside a graph capture: the moments
        of the variables with a gradient, the device counter and the table.  False: host path."""
        gs, vs, _, _ = self._gather(grads_and_vars)
        return bool(vs) and vs[0].is_cuda and self.device_ready(vs[0])

    @torch.no_grad()
    def snapshot(self):
        """Copy the device counter (current stream; capturable) for launch(snap=True)."""
        self._snap.copy_(self._dev)

    @torch.no_grad()
    def launch(self, grads_and_vars, advance=True, snap=False):
        """One dpac_adam_step launch on the current stream, the host count untouched: the form a
        HIP graph captures (after prepare()).  t is the device counter's; snap: that of the last
        snapshot() instead (never advanced), for a part of a step that another stream's part,
        unordered with this one, completes and advances."""
        gs, vs, ms, ss = self._gather(grads_and_vars)
        ops.adam_step([v.data for v in vs], [g.detach().contiguous() for g in gs], ms, ss,
                      self._snap if snap else self._dev, self._table, self.b1, self.b2, self.eps,
                      advance and not snap)

    @torch.no_grad()
    def apply_gradients(self, grads_and_vars, advance=True):
        """advance=False leaves `iterations` unchanged, so one optimizer step can be
        applied in parts (disjoint variable sets, same lr and t)."""
        lr = self.schedule(self.iterations)
        t = self.iterations + 1
        gs, vs, ms, ss = self._gather(grads_and_vars)
        if gs and gs[0].is_cuda and self.device_ready(vs[0]):  # alpha and t read on the device
            self.launch(zip(gs, vs), advance)
            if advance:
                self.iterations += 1
            return
        if not gs and advance and self._dev is not None:  # no gradient at all: the step still counts
            ops.adam_step([], [], [], [], self._dev, self._table, self.b1, self.b2, self.eps, True)
        if gs:
            alpha, omb1, omb2 = tf_adam_scalars(lr, t, self.b1, self.b2, vs[0].dtype)
        if gs and gs[0].is_cuda:  # one dpac_adam_apply launch (same arithmetic, same order)
            ops.adam_apply([v.data for v in vs], [g.detach().contiguous() for g in gs], ms, ss, alpha,
                           self.b1, self.b2, self.eps)
        elif gs:
            torch._foreach_add_(ms, torch._foreach_mul(torch._foreach_sub(gs, ms), omb1))
            g2 = torch._foreach_mul(gs, gs)
            torch._foreach_add_(ss, torch._foreach_mul(torch._foreach_sub(g2, ss), omb2))
            den = torch._foreach_add(torch._foreach_sqrt(ss), self.eps)
            torch._foreach_sub_(vs, torch._foreach_div(torch._foreach_mul(ms, alpha), den))
        if advance:
            self.iterations += 1

    def device_iterations(self):
        """The device counter (synchronises), or None while no step has run on the device path."""
        if self._dev is None:
            return None
        return int(self._dev[0].item())

    def state_dict(self, variables=None):
        """`iterations` and, per variable in order (`variables`, default: in the order the
        optimizer first saw them), the moments m and v on the CPU (None: no moments yet)."""
        vs = list(self.state) if variables is None else list(variables)
        c = lambda t: t.detach().to("cpu").clone()
        sts = [self.state.get(v) for v in vs]
        return {"iterations": self.iterations,
                "m": [None if st is None else c(st[0]) for st in sts],
                "v": [None if st is None else c(st[1]) for st in sts]}

    @torch.no_grad()
    def load_state_dict(self, sd, variables=None):
        """Restore state_dict(): the host count, the device counter and the moments, written in
        place where they exist (captured graphs hold their addresses)."""
        vs = list(self.state) if variables is None else list(variables)
        ms, ss = sd.get("m", []), sd.get("v", [])
        if len(ms) != len(vs) or len(ss) != len(vs):
            raise ValueError(f"TFAdam.load_state_dict: moments for {len(ms)} variables, have {len(vs)}")
        for v, m, s in zip(vs, ms, ss):
            st = self.state.get(v)
            if m is None:
                if st is not None:
                    st[0].zero_(); st[1].zero_()
                continue
            if st is None:
                st = self.state[v] = (torch.zeros_like(v), torch.zeros_like(v))
            st[0].copy_(torch.as_tensor(m).to(st[0]))
            st[1].copy_(torch.as_tensor(s).to(st[1]))
        self.iterations = int(sd["iterations"])
        if self._dev is not None:
            self._dev[0] = self.iterations
