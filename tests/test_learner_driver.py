"""The learners' graph-replay driver (sharetrade/trainer/graphs.py) on the CPU, against a naive loop.

``IterationDriver`` decides which captured graph an iteration of DeepDQN / RecurrentDQN replays, when the GRU's
two online weight sets alternate and where the target-net copy falls (host work between graphs, so never inside a
k-iteration graph).  None of that needs a GPU: the hooks here append tokens to a log, and the stand-in ``graph(fn)``
records the tokens ``fn`` emits into a private list -- nothing "runs" during a capture, as in a real one -- and
appends them to the log at every ``replay()``.  The log of the driver must then equal the log of ``_reference``: single
eager iterations, one after the other, transcribed from the learners' ``iteration()`` as it was before the driver
existed (commit 9a7cd56), with k-iteration graphs wherever the rule allows one, the rule spelled out update by
update.  Four broken drivers show that the comparison notices each part of the rule."""
import itertools

import pytest

from sharetrade.trainer.graphs import IterationDriver

MODES = ("whole", "whole_sync", "split")     # no all-reduce | an all-reduce that captures | one that does not
TARGETS, KS, NS = (0, 1, 3, 6, 7), (1, 2, 4), range(14)


class _Graph:
    def __init__(self, rig, body):
        self.rig, self.body = rig, body

    def replay(self):
        rig = self.rig
        kind = next(key[0] for key, g in rig.d.graphs.items() if g is self)
        rig.spans.append((kind, len(rig.log), len(rig.log) + len(self.body), rig.d.par, self.body))
        rig.log.extend(self.body)


class _Rig:
    """A driver over token-logging hooks.  With one weight set the update hook drops ``flip``, as DeepDQN's does."""

    def __init__(self, cls, n_sets, overlap, mode, te):
        self.log = self.sink = []
        self.spans = []                      # (kind, start, end, par at replay, body) per graph replay
        self.te = te
        emit = lambda *tok: self.sink.append(tok)   # noqa: E731
        par = lambda: self.d.par                    # noqa: E731

        def update(with_act, flip):
            emit("update", with_act, flip and n_sets == 2, par())
            if mode != "whole":
                emit("sync")                 # the learners' update all-reduces inside, captured or eager
        self.d = cls(act=lambda: emit("act", par()), update=update,
                     grads=lambda with_act: emit("grads", with_act, par()), apply=lambda: emit("apply", par()),
                     sync_target=lambda: emit("target"), sync_bucket=lambda: emit("sync"),
                     whole_graph=lambda: mode != "split", target_every=lambda: self.te, overlap_act=overlap,
                     n_sets=n_sets, device=None, graph=self.graph)

    def graph(self, fn):
        outer, self.sink = self.sink, []
        try:
            fn()
            return _Graph(self, self.sink)
        finally:
            self.sink = outer

    def run(self, calls):
        for name, arg in calls:
            getattr(self.d, name)(arg)
        return self


def _reference(n_sets, overlap, mode, te, calls):
    """(log, offsets of the k-graph launches in it, (updates, acts, par)) of single iterations run one by one."""
    log, kstarts = [], []
    s = dict(updates=0, acts=0, par=0, captured=False, k=1)
    whole = mode != "split"

    def update(with_act):
        if s["captured"] and not whole:      # once captured: gradients | host all-reduce | Adam
            log.extend([("grads", with_act, s["par"]), ("sync",), ("apply", s["par"])])
        else:
            flip = with_act and whole and n_sets == 2
            log.append(("update", with_act, flip, s["par"]))
            if mode != "whole":
                log.append(("sync",))
            if flip:
                s["par"] ^= 1
        s["updates"] += 1
        if te and s["updates"] % te == 0:
            log.append(("target",))

    def iteration(u=1):
        if overlap and u >= 1:
            update(True)
            u -= 1
        else:
            log.append(("act", s["par"]))
        s["acts"] += 1
        for _ in range(u):
            update(False)

    for name, arg in calls:
        if name == "capture":                # the warm-up is one eager iteration
            iteration()
            s["captured"], s["k"] = True, arg if overlap and whole and arg > 1 else 1
        elif name == "iteration":
            iteration(arg)
        else:
            n, k = arg, s["k"]
            while n > 0:
                # a k-graph: captured, enough iterations left, and none of its updates but the last is a target copy
                if k > 1 and n >= k and not any(te and (s["updates"] + j) % te == 0 for j in range(1, k)):
                    kstarts.append(len(log))
                    for _ in range(k):
                        iteration()
                    n -= k
                else:
                    iteration()
                    n -= 1
    return log, kstarts, (s["updates"], s["acts"], s["par"])


def _cases():
    for overlap, mode, te, k in itertools.product((False, True), MODES, TARGETS, KS):
        for n in NS:
            yield overlap, mode, te, [("capture", k), ("iterations", n)]
        for n, u in itertools.product((0, 6, 13), (0, 1, 3)):
            yield overlap, mode, te, [("capture", k), ("iteration", u), ("iterations", n), ("iteration", u)]
        yield overlap, mode, te, [("iteration", 1), ("iteration", 3), ("iteration", 0), ("capture", k),
                                  ("iterations", 5)]


def _schedule_errors(cls, n_sets):
    """Cases of the grid in which ``cls`` departs from the reference: log, k-graph launches or counters."""
    for overlap, mode, te, calls in _cases():
        rig = _Rig(cls, n_sets, overlap, mode, te).run(calls)
        log, kstarts, counters = _reference(n_sets, overlap, mode, te, calls)
        d = rig.d
        if (rig.log != log or [sp[1] for sp in rig.spans if sp[0] == "iter_k"] != kstarts
                or (d.updates, d.acts, d.par) != counters):
            yield overlap, mode, te, calls


@pytest.mark.parametrize("n_sets", [1, 2])
def test_schedule_equals_the_naive_loop(n_sets):
    assert sum(1 for _ in _cases()) == 2 * 3 * 5 * 3 * (14 + 9 + 1)
    assert list(_schedule_errors(IterationDriver, n_sets)) == []


@pytest.mark.parametrize("n_sets", [1, 2])
def test_graphs_replay_for_their_set_and_keep_the_target_copy_outside(n_sets):
    replays = kgraphs = 0
    for overlap, mode, te, calls in _cases():
        rig = _Rig(IterationDriver, n_sets, overlap, mode, te).run(calls)
        log = _reference(n_sets, overlap, mode, te, calls)[0]
        assert n_sets == 2 or rig.d.par == 0
        for kind, start, end, par, body in rig.spans:
            # captured for the set it is replayed for (the split pair is captured for the one set in use)
            assert body[0][0] in ("act", "update", "grads", "apply") and body[0][-1] == par, (kind, calls)
            assert ("target",) not in body
            replays += 1
            if kind == "iter_k":
                # the naive loop copies the target net nowhere strictly inside the graph's span
                assert mode != "split" and ("target",) not in log[start:end] + rig.log[start:end]
                assert sum(t[0] == "update" for t in body) == dict(calls)["capture"]
                kgraphs += 1
        if mode == "split":
            for i, tok in enumerate(rig.log):
                if tok[0] == "grads":
                    assert rig.log[i + 1] == ("sync",) and rig.log[i + 2][0] == "apply", (i, calls)
                assert tok[0] != "apply" or rig.log[i - 1] == ("sync",)
    assert replays > 1000 and kgraphs > 100


def test_two_sets_refuse_an_odd_k():
    for k in (3, 5):
        rig = _Rig(IterationDriver, 2, True, "whole", 6)
        with pytest.raises(ValueError, match=r"iters_per_graph must be even \(the online sets alternate\)"):
            rig.d.capture(k)
        assert rig.log == [] and not rig.d.captured      # refused before anything ran
    _Rig(IterationDriver, 1, True, "whole", 6).d.capture(3)       # one set: any k
    _Rig(IterationDriver, 2, True, "split", 6).d.capture(3)       # no k-graph is captured: nothing to refuse
    _Rig(IterationDriver, 2, False, "whole", 6).d.capture(3)


class _BoundaryOffByOne(IterationDriver):
    """Refuses a k-graph whose last update is a target copy (``updates + k`` for ``updates + k - 1``)."""

    def iterations(self, n):
        k = self.k
        while n > 0:
            g, te = self.g("iter_k", self.par), self.target_every()
            if g is not None and n >= k and (not te or self.updates // te == (self.updates + k) // te):
                g.replay()
                self.acts += k
                self._updated(k)
                n -= k
            else:
                self.iteration()
                n -= 1


class _NoFlipAfterReplay(IterationDriver):
    """Stays on its weight set after a replayed iteration graph."""

    def iteration(self, updates=1):
        par = self.par
        replayed = (self.overlap_act and updates >= 1 and self.g("pre_act") is None
                    and self.g("iter", par) is not None)
        super().iteration(updates)
        if replayed:
            self.par = par


class _NoTargetCheckAfterWarmUp(IterationDriver):
    def capture(self, iters_per_graph=1):
        self._warm = True
        super().capture(iters_per_graph)

    def _updated(self, n=1):
        if getattr(self, "_warm", False):
            self._warm = False
            self.updates += n
        else:
            super()._updated(n)


class _KGraphsInSplitMode(IterationDriver):
    """Captures and replays k whole updates per graph although the all-reduce cannot be captured."""

    def capture(self, iters_per_graph=1):
        super().capture(iters_per_graph)
        if self.overlap_act and not self.whole_graph() and iters_per_graph > 1:
            def k_iterations():
                for _ in range(iters_per_graph):
                    self.update(True, False)
            for p in range(self.n_sets):
                self.graphs["iter_k", p] = self.graph(k_iterations)
            self.k = iters_per_graph


@pytest.mark.parametrize("cls,n_sets", [(_BoundaryOffByOne, 1), (_BoundaryOffByOne, 2), (_NoFlipAfterReplay, 2),
                                        (_NoTargetCheckAfterWarmUp, 1), (_NoTargetCheckAfterWarmUp, 2),
                                        (_KGraphsInSplitMode, 1), (_KGraphsInSplitMode, 2)])
def test_the_schedule_check_catches_a_broken_driver(cls, n_sets):
    """(With one weight set there is no flip to leave out: ``_NoFlipAfterReplay`` is the driver itself there.)"""
    assert next(_schedule_errors(cls, n_sets), None) is not None


def test_target_every_zero_never_copies():
    for n_sets in (1, 2):
        rig = _Rig(IterationDriver, n_sets, True, "whole", 0).run([("capture", 4), ("iterations", 13)])
        assert ("target",) not in rig.log and rig.d.updates == 14


def test_hooks_over_a_weak_proxy_leave_no_cycle():
    """The learners' construction: the owner holds the driver, the hooks reach the owner through a weak proxy.
    Dropping the owner then frees every graph at once, without the cycle collector (which could otherwise destroy
    a HIP graph in the middle of a later learner's capture)."""
    import gc
    import weakref

    freed = []

    class Graph:
        def replay(self):
            pass

        def __del__(self):
            freed.append(self)

    class Owner:
        def __init__(self):
            me, self.ops = weakref.proxy(self), 0
            op = lambda *a: me.op()     # noqa: E731
            self.drv = IterationDriver(act=op, update=op, grads=op, apply=op, sync_target=op, sync_bucket=op,
                                       whole_graph=lambda: True, target_every=lambda: 3, overlap_act=True, n_sets=2,
                                       device=None, graph=lambda fn: (fn(), Graph())[1])

        def op(self):
            self.ops += 1

    gc.disable()
    try:
        o = Owner()
        o.drv.capture(2)
        o.drv.iterations(5)
        assert len(o.drv.graphs) == 8 and o.ops > 8 and not freed
        del o
        assert len(freed) == 8
    finally:
        gc.enable()
