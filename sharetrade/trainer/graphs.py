"""HIP-graph capture and replay of a learner's iteration: one host-side driver for DeepDQN and RecurrentDQN.

The learner hands its operations over as plain callables and holds an ``IterationDriver``; the driver owns every
captured graph, the counters and the schedule: which graph an iteration replays, when the online weight sets
alternate and where the target-net copy (host work between graphs) falls.  Nothing here launches a kernel or loads a
native library, so the whole schedule runs on the CPU with stand-in hooks (tests/test_learner_driver.py).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch

# HIP-graph capture mode: "thread_local" -- with an RCCL process group alive, its watchdog thread
# polls collective events during our captures; in the default global mode that poll invalidates the
# capture (hipErrorStreamCaptureInvalidated) and kills the watchdog.  Our own thread stays checked.
CAPTURE_MODE = "thread_local"


def capture_graph(fn: Callable[[], None]):
    """``fn``'s launches on the current stream, captured into a new HIP graph."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
        fn()
    return g


def driver_attr(name: str) -> property:
    """A learner's view of its driver's ``name`` (a counter, ``par``, ``captured``): readable and assignable."""
    return property(lambda self: getattr(self._drv, name), lambda self, v: setattr(self._drv, name, v))


def driver_graph(kind: str) -> property:
    """A learner's view of its driver's ``kind`` graph of weight set 0 (None if not captured)."""
    return property(lambda self: self._drv.g(kind))


class IterationDriver:
    """Warm-up, graph capture and replay dispatch of act + update iterations.

    Hooks (each launches on the current stream and reads the current weight set from ``par``): ``act()``;
    ``update(with_act, flip)``, a whole update, with the act step beside it and / or re-packing into the other
    weight set; ``grads(with_act)`` and ``apply()``, its two halves around the host all-reduce ``sync_bucket()``;
    ``sync_target()``.  They must not keep the learner alive (it holds the driver: reach it through a
    ``weakref.proxy``), so that a dropped learner frees its graphs at once: left to the cycle collector, a graph
    may be destroyed in the middle of a later capture, which HIP refuses and the process does not survive.
    ``whole_graph()``: the update captures whole (no gradient all-reduce, or one that captures); otherwise the
    split pair "grads | sync_bucket | apply" is captured and the weight sets never alternate.  ``target_every()``:
    updates between target-net copies, 0 = never; read at every use.  ``n_sets``: 1, or 2 online weight sets that
    alternate with every overlapped iteration.  ``graph(fn)`` returns something with ``replay()``; ``device=None``
    runs the warm-up in place, not on a side stream (both for runs without a GPU).

    ``updates`` and ``acts`` count what ran, ``par`` is the weight set the next operation reads; ``graphs[kind,
    set]``: "act", "upd", "iter" (the overlapped iteration), "iter_k" (k of them); "pre", "pre_act", "post" (set 0)."""

    def __init__(self, *, act, update, grads, apply, sync_target, sync_bucket, whole_graph, target_every,
                 overlap_act: bool, n_sets: int = 1, device: Optional[torch.device] = None,
                 graph: Callable = capture_graph):
        self.act, self.update, self.grads, self.apply = act, update, grads, apply
        self.sync_target, self.sync_bucket = sync_target, sync_bucket
        self.whole_graph, self.target_every = whole_graph, target_every
        self.overlap_act, self.n_sets, self.device, self.graph = bool(overlap_act), int(n_sets), device, graph
        self._alt = self.n_sets - 1        # par ^= _alt: the other set of two, the same set of one
        self.updates = self.acts = self.par = 0
        self.graphs: Dict[Tuple[str, int], object] = {}
        self.k, self.captured = 1, False   # k: iterations per "iter_k" graph

    def g(self, kind: str, par: int = 0):
        return self.graphs.get((kind, par))

    def _updated(self, n: int = 1) -> None:
        """Count n updates; the target-net copy when the count lands on its cadence."""
        self.updates += n
        te = self.target_every()
        if te and self.updates % te == 0:
            self.sync_target()

    def _warm_up(self, fn) -> None:
        if self.device is None:
            return fn()
        main, s = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
        s.wait_stream(main)
        with torch.cuda.stream(s):
            fn()
        main.wait_stream(s)

    def capture(self, iters_per_graph: int = 1) -> None:
        """One warm-up iteration (counted), then per weight set the act step, the update and (overlap_act) the
        whole iteration as graphs.  ``iters_per_graph`` k > 1 (overlapped iterations whose update captures
        whole; even with two sets): also k whole iterations per graph, which ``iterations(n)`` replays."""
        k, whole = int(iters_per_graph), self.whole_graph()
        many = self.overlap_act and whole and k > 1
        if many and self.n_sets == 2 and k % 2:
            raise ValueError("iters_per_graph must be even (the online sets alternate)")
        self.graphs, self.k = {}, 1
        self._warm_up(self.iteration)      # no graphs: one eager iteration, counted, in the captured one's op order
        cur = self.par
        for p in range(self.n_sets):
            self.par = p
            self.graphs["act", p] = self.graph(self.act)
            if whole:
                self.graphs["upd", p] = self.graph(lambda: self.update(False, False))
                if self.overlap_act:
                    self.graphs["iter", p] = self.graph(lambda: self.update(True, True))
        if many:
            def k_iterations():
                for _ in range(k):
                    self.update(True, True)
                    self.par ^= self._alt
            for p in range(self.n_sets):
                self.par = p
                self.graphs["iter_k", p] = self.graph(k_iterations)
            self.k = k
        self.par = cur
        if not whole:
            # data parallel: the gradient all-reduce runs between two graphs (act + gradients | Adam), the
            # collective itself stays outside the capture; the weight set never alternates here
            self.graphs["pre", 0] = self.graph(lambda: self.grads(False))
            if self.overlap_act:
                self.graphs["pre_act", 0] = self.graph(lambda: self.grads(True))
            self.graphs["post", 0] = self.graph(self.apply)
        self.captured = True

    def _replay_split(self, pre) -> None:
        pre.replay()
        self.sync_bucket()
        self.graphs["post", 0].replay()

    def act_step(self) -> None:
        """One counted act step: its graph if captured."""
        g = self.g("act", self.par)
        if g is not None:
            g.replay()
        else:
            self.act()
        self.acts += 1

    def update_step(self) -> None:
        """One counted update without an act step: the split pair or the update graph if captured."""
        pre, g = self.g("pre"), self.g("upd", self.par)
        if pre is not None:
            self._replay_split(pre)
        elif g is not None:
            g.replay()
        else:
            self.update(False, False)
        self._updated()

    def iteration(self, updates: int = 1) -> None:
        """One act step and ``updates`` updates; with overlap_act the first update runs beside the act step."""
        if self.overlap_act and updates >= 1:
            pre, g = self.g("pre_act"), self.g("iter", self.par)
            if pre is not None:
                self._replay_split(pre)
            elif g is not None:
                g.replay()
                self.par ^= self._alt
            else:
                flip = self.n_sets == 2 and self.whole_graph()
                self.update(True, flip)
                if flip:
                    self.par ^= 1
            self.acts += 1
            self._updated()
            updates -= 1
        else:
            self.act_step()
        for _ in range(updates):
            self.update_step()

    def iterations(self, n: int) -> None:
        """n single-update iterations: whole k-iteration graphs where no target-net copy falls inside one (it runs
        on the host between graphs), single iterations otherwise."""
        k = self.k
        while n > 0:
            g, te = self.g("iter_k", self.par), self.target_every()
            if g is not None and n >= k and (not te or self.updates // te == (self.updates + k - 1) // te):
                g.replay()                 # two sets: k is even, the set alternates back
                self.acts += k
                self._updated(k)
                n -= k
            else:
                self.iteration()
                n -= 1
