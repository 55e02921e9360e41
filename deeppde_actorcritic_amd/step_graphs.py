"""The training steps as HIP graphs: one capture recipe (_warm_up, _capturing, _copy_in), the
backward chain with its deferred range-guard fallbacks and its optimizer step (_BackwardChain),
and the graphs the solver replays.  Its DPAC_* knobs arrive as arguments (defer=, join=, steps)."""

import contextlib

import torch

from .equation import TrajectoryBatch

# HIP-graph captures are thread-local: with a torch.distributed "nccl" (RCCL) process group
# alive, its watchdog thread queries events concurrently, and under the default global
# capture mode such a query invalidates an ongoing capture ("operation failed due to a
# previous error during capture", seen intermittently in round 3's RCCL test).
_CAPTURE_MODE = "thread_local"


@contextlib.contextmanager
def _capturing():
    """Capture the body's launches into the HIP graph this yields: the package's only capture."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE):
        yield graph


@contextlib.contextmanager
def _warm_up(side):
    """The warm-up in front of a capture (allocator, autograd), on `side` behind the current
    stream's work and joined back: `for _ in twice` around the body runs it two times."""
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield range(2)
    torch.cuda.current_stream().wait_stream(side)


def _copy_in(static: TrajectoryBatch, batch: TrajectoryBatch):
    for dst, src in zip(static, batch):
        if dst.data_ptr() != src.data_ptr():  # drawn in place by prefetch_samples: no copy
            dst.copy_(src)


class _GraphStep:
    """An optimizer step (or one part of it) that a graph appends to its gradients in the
    capture only: the graph constructors' warm-up runs apply no step.  prepare(grads), outside the
    capture, makes what the launch needs and tells whether the optimizer's step can be captured
    (TFAdam.prepare); calling it with the captured gradient buffers launches dpac_adam_step."""

    def __init__(self, opt, variables, advance=True, snap=False):
        """snap: the step reads the counter's snapshot (TFAdam.launch) and leaves the counter."""
        self.opt, self.variables, self.advance, self.snap = opt, list(variables), advance, snap

    def prepare(self, grads) -> bool:
        return self.opt.prepare(zip(grads, self.variables))

    def __call__(self, grads):
        self.opt.launch(zip(grads, self.variables), self.advance, self.snap)


class _GradGraph:
    """One gradient evaluation (forward + backward) captured as a HIP graph over static
    input buffers, with the optimizer step on those gradients at its end when `step` (a
    _GraphStep) is given and can be captured (`stepped`); otherwise the optimizer runs
    eagerly on the returned gradients, whose buffers the next replay overwrites.
    Replaying it after copying a fresh batch in replaces the ~10^3 kernel launches of a
    step (the actor's reverse time loop, the critic's G network and TD assembly) with one
    graph launch.  Parameters are updated in place, so every replay sees the current
    weights."""

    def __init__(self, fn, batch: TrajectoryBatch, step=None):
        self.static = TrajectoryBatch(*[t.clone() for t in batch])
        with _warm_up(torch.cuda.Stream()) as twice:
            for _ in twice:
                out = fn(self.static)
        self.stepped = step is not None and step.prepare(out)
        with _capturing() as self.graph:
            self.out = fn(self.static)
            if self.stepped:
                step(self.out)

    def __call__(self, batch: TrajectoryBatch):
        _copy_in(self.static, batch)  # a caller's batch, never the static buffers: every tensor copied
        self.graph.replay()
        return list(self.out)


class _BackwardChain:
    """A backward chain as a HIP graph: body(x) -> gradients under defer(), which collects the
    chain's deferred range-guard fallbacks (ops.deferred_fallbacks) into `redo_fns`; then those
    fallbacks (no-op kernels while the split-fp16 status word is clear, the exact-f32
    recomputation of the chain once it is set); then, when `stepped`, the optimizer step on the
    gradients (`step`, a _GraphStep).  join (DPAC_GUARD_DEFER=join): the fallbacks and the step
    leave the chain's graph for a second one, `g_redo`, which redo() replays once the caller has
    joined the chains' streams; otherwise g_redo is None and redo() does nothing.  defer: a context
    manager factory (ActorCriticSolver._deferring); None: no deferral, redo_fns stays empty."""

    def __init__(self, body, defer=None, step=None, join=False):
        self.body, self.step, self.join = body, step, join
        self.defer = defer or (lambda: contextlib.nullcontext([]))

    def warm(self, x):
        """One warm-up run: the body and its fallbacks, no step."""
        with self.defer() as fns:
            out = self.body(x)
        for f in fns:
            f()
        return out

    def capture(self, x, stepped):
        self.stepped, self.g_redo = stepped, None
        with _capturing() as self.graph:
            with self.defer() as self.redo_fns:
                self.out = self.body(x)
            if not self.join:  # the fallbacks at the chain's end, in the same graph
                self._tail()
        if self.join and (self.redo_fns or stepped):  # the step behind the joined fallbacks
            with _capturing() as self.g_redo:
                self._tail()
        # the solver's methods, and the solver holds this chain: no reference cycle, or a dead solver's
        # graphs wait for a garbage collection, which can come inside a later capture and abort it
        del self.body, self.defer, self.step

    def _tail(self):
        for f in self.redo_fns:
            f()
        if self.stepped:
            self.step(self.out)

    def redo(self):
        if self.g_redo is not None:
            self.g_redo.replay()


class _SplitActorGraphs:
    """The actor step as two HIP graphs: the fused forward rollout with its backward
    saves (replayed on a side stream, so it runs beside the critic step: it reads only
    the actor's parameters, which the critic step does not change) and the gradient
    from those saves (after the critic update, which the terminal value V(x_N) needs;
    solver.py:67-70 order), a _BackwardChain (`chain`).  The backward graph reads the forward
    graph's outputs in place: nothing is copied between them.  With `step` (a _GraphStep that
    can be captured: `stepped`) the actor's optimizer step ends the chain."""

    def __init__(self, fwd_fn, bwd_fn, batch: TrajectoryBatch, side, defer=None, step=None, join=False):
        self.static = TrajectoryBatch(*[t.clone() for t in batch])
        self.side = side
        self.chain = _BackwardChain(bwd_fn, defer, step, join)
        with _warm_up(side) as twice:
            for _ in twice:
                out = self.chain.warm(fwd_fn(self.static))
        self.stepped = step is not None and step.prepare(out)
        with _capturing() as self.g_fwd:
            self.fwd = fwd_fn(self.static)
        self.chain.capture(self.fwd, self.stepped)

    def launch_forward(self, batch: TrajectoryBatch):
        """On the side stream, after the work queued so far on the current stream."""
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            _copy_in(self.static, batch)
            self.g_fwd.replay()

    def grads(self):
        """The gradients (valid once redo() has run after them)."""
        torch.cuda.current_stream().wait_stream(self.side)
        self.chain.graph.replay()
        return list(self.chain.out)


class _SplitCriticGraphs:
    """The critic step as three HIP graphs, split at the G network's output: the head
    (rollout, G forward with saves, TD assembly, V forward, the loss's gradient at V's
    output and at G's TD1 dots), V's backward (its parameter gradients), and the G
    network's backward (input-gradient chain + parameter gradients), a _BackwardChain (`chain`).
    The G backward reads only the head's outputs, so it is launched on a side stream as soon as
    the head is done: it runs beside V's backward, V's Adam step and the actor's terminal V(x_N)
    (a chain of small kernels that leaves most CUs idle) and then beside the actor's BPTT, which
    needs the updated V only (solver.py:221), not G.

    With v_step and g_step (_GraphSteps that can be captured: `stepped`) the critic's optimizer
    step is captured in its two parts: V's ends V's backward graph and G's, which advances the
    step counter, ends the chain on the side stream.  The two are not ordered with each
    other (DPAC_GBACK=early launches the G backward before V's step), so V's part reads t from a
    snapshot of the counter that the head graph takes before either can run: the advance cannot
    reach what V's part reads."""

    def __init__(self, head_fn, v_fn, back_fn, batch: TrajectoryBatch, side, defer=None,
                 v_step=None, g_step=None, join=False):
        self.static = TrajectoryBatch(*[t.clone() for t in batch])
        self.side = side
        self.chain = _BackwardChain(lambda back: back_fn((None,) + tuple(back)), defer, g_step, join)
        with _warm_up(side) as twice:
            for _ in twice:
                h = head_fn(self.static)
                gv = v_fn(h[0])
                gb = self.chain.warm(h[1])
        self.stepped = (v_step is not None and g_step is not None and v_step.prepare(gv)
                        and g_step.prepare(gb))
        with _capturing() as self.g_head:
            if self.stepped:  # this step's t for V's part, before G's part can advance the counter
                v_step.opt.snapshot()
            self.head_out = head_fn(self.static)
        with _capturing() as self.g_v:
            self.v_out = v_fn(self.head_out[0])
            if self.stepped:
                v_step(self.v_out)
        self.chain.capture(self.head_out[1], self.stepped)

    def head(self, batch: TrajectoryBatch):
        """The head graph on the current stream."""
        _copy_in(self.static, batch)
        self.g_head.replay()

    def grads_v(self):
        """V's parameter gradients, and then V's captured step (current stream, after head())."""
        self.g_v.replay()
        return list(self.v_out)

    def launch_back(self, after: torch.cuda.Event):
        """G's parameter gradients (and then G's captured step), replayed on the side stream once
        `after` (recorded behind head()) has passed; use them on the side stream (valid once
        redo() has run)."""
        self.side.wait_event(after)
        with torch.cuda.stream(self.side):
            self.chain.graph.replay()
        return list(self.chain.out)
