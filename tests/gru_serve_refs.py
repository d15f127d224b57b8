"""Shared drivers of the GRU serving tests (tests/test_gru_serve.py on the CPU, tests/test_gpu_gru_serve.py on the
GPU): serving the bars of tests/gru_backtest_refs.py to sessions bar by bar, in lockstep or raggedly, and the
bit-pattern comparison of a served trace with a rollout's.

A served bar returns the realised reward of the session's *previous* bar, so column i of a served ``reward``
trace is column i - 1 of the rollout's, and a session's running return after n bars is the sequential float32
sum of the rollout's rewards 0 .. n - 2.
"""
import torch

TRACE = ("actions", "q", "reward", "pos")


def bits(t):
    return t.view(torch.int32) if t.is_floating_point() else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def empty_trace(E, steps):
    return {"actions": torch.full((E, steps), -9, dtype=torch.int8), "q": torch.zeros(E, steps, 3),
            "reward": torch.zeros(E, steps), "pos": torch.full((E, steps), -9, dtype=torch.int32)}


def put(tr, rows, col, d):
    """Store a decision's rows at trace column(s) ``col`` of envs ``rows``."""
    tr["actions"][rows, col] = d.actions.cpu()
    tr["q"][rows, col] = d.q.cpu()
    tr["reward"][rows, col] = d.reward.cpu()
    tr["pos"][rows, col] = d.position.cpu()


def serve_lockstep(srv, slots, close, feat, start, steps, *, shuffle_seed=0, flag_bar=None, before_bar=None, **kw):
    """Bars start .. start + steps - 1 of env e to session slots[e], every session on every call, the row order
    re-shuffled on every call.  ``flag_bar``: the bar at which every row carries the new-episode flag;
    ``before_bar(t)`` runs before bar t is served."""
    E = len(slots)
    sl = torch.as_tensor(slots, dtype=torch.int64)
    g = torch.Generator().manual_seed(shuffle_seed)
    tr = empty_trace(E, steps)
    for i in range(steps):
        t = start + i
        if before_bar is not None:
            before_bar(t)
        perm = torch.randperm(E, generator=g)
        ne = torch.ones(E, dtype=torch.bool) if flag_bar == t else None
        d = srv.step(sl[perm], feat[perm, t], close[perm, t], new_episode=ne, return_q=True, **kw)
        put(tr, perm, i, d)
    return tr


def serve_ragged(srv, slots, close, feat, bars_each, *, seed=0, first_sizes=(1, 32, 33), after_call=None):
    """Every session gets bars 0 .. bars_each - 1 in order, but on each call only a random subset sends its next
    bar (the first calls have the given sizes).  ``after_call(batch_slots)`` runs after each call.  Returns the
    per-session trace and the batch sizes used."""
    E = len(slots)
    sl = torch.as_tensor(slots, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    nxt = torch.zeros(E, dtype=torch.int64)
    tr = empty_trace(E, bars_each)
    sizes, forced = [], list(first_sizes)
    while bool((nxt < bars_each).any()):
        left = torch.nonzero(nxt < bars_each).flatten()
        left = left[torch.randperm(left.numel(), generator=g)]
        k = forced.pop(0) if forced and forced[0] <= left.numel() else \
            int(torch.randint(1, left.numel() + 1, (1,), generator=g))
        rows = left[:k]
        t = nxt[rows]
        d = srv.step(sl[rows], feat[rows, t], close[rows, t], return_q=True)
        put(tr, rows, t, d)
        nxt[rows] += 1
        sizes.append(k)
        if after_call is not None:
            after_call(sl[rows])
    return tr, sizes


def seq_sum(reward):
    """The sequential float32 sum of the columns of ``reward`` [E, n]."""
    s = torch.zeros(reward.shape[0])
    for i in range(reward.shape[1]):
        s = s + reward[:, i]
    return s


def against_rollout(tr, st, roll, steps):
    """Names of everything in a served trace of ``steps`` bars (``tr``, final state ``st``) that differs by bit
    pattern from a rollout's traced result dict ``roll`` over the same bars."""
    bad = []
    for k in ("actions", "q"):
        if not same(tr[k], roll[k][:, :steps]):
            bad.append(k)
    if not same(tr["reward"][:, 1:], roll["reward"][:, :steps - 1]) or bool((tr["reward"][:, 0] != 0).any()):
        bad.append("reward")
    if not same(st["ret"].cpu(), seq_sum(roll["reward"][:, :steps - 1])):
        bad.append("ret")
    for k in ("position", "entry", "h", "trades", "long"):
        if k in roll and not same(st[k].cpu(), roll[k]):
            bad.append(k)
    return bad
