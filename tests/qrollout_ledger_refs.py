"""An independent reference for the 2x128 backtest's risk ledger (``csrc/qrollout.hip``'s ledger instance and
``sharetrade/serve/rollout.py::ledger_from_trace``), the inputs on which it is exact, and comparison helpers.

:func:`walk` is plain Python in float64 and is written differently from ``ledger_from_trace``: it first runs the
env and keeps the lists (equity, trade prices, shares before and after), then reads every ledger field off the
lists.  ``mut=`` makes one deliberate error (``MUTATIONS``), for the tests that show each one is caught.

On :func:`exact_prices` (a walk on quarters between 8 and 64, budget 120, shares 0) every fp32 operation of the
ledger is exact, so the float64 walk and an fp32 ledger agree to the bit: equities are multiples of 1/4 below
2^9, squared day changes multiples of 1/16, ``d * d <= 56^2`` sums to under 2^18 over 67 days, all far inside 24
bits.
"""
import numpy as np
import torch

H = 201
BUDGET = 120.0
SEED = 3
CHUNK = 16
F32 = ("eq_prev", "eq0", "v0", "v_last", "peak", "max_dd", "sumsq", "sum_d", "sum_d2", "sum_sd")
INTS = ("run", "dd_days", "days", "chose_buy", "chose_sell", "refused_buy", "refused_sell", "flat_days", "max_shares",
        "sum_s", "sum_s2")
MUTATIONS = ("peak_after_drawdown", "drawdown_before_equity", "pnl_against_eq0", "position_before_trade",
             "refused_buy_as_executed", "d_from_first_trade_price", "run_not_reset", "pad_rows_live")


def exact_prices(E, steps, extra=0, seed=7):
    """[E, H + steps + extra] fp32: start at 32, move k / 4 per day with k uniform in -4 .. 4, clipped to [8, 64]."""
    g = np.random.default_rng(seed)
    k = g.integers(-4, 5, size=(E, H + steps + extra)).astype(np.float64) / 4.0
    P = np.empty((E, H + steps + extra), dtype=np.float64)
    x = np.full(E, 32.0)
    for j in range(P.shape[1]):
        if j:
            x = np.clip(x + k[:, j], 8.0, 64.0)
        P[:, j] = x
    return torch.from_numpy(P.astype(np.float32))


def lognormal_prices(E, steps, extra=0):
    """The prices of tests/test_gpu_backtest.py."""
    g = np.random.default_rng(3)
    p = 50.0 * np.exp(np.cumsum(g.normal(0, 0.02, size=(E, H + steps + extra)), axis=1))
    return torch.from_numpy(p.astype(np.float32))


def random_actions(E, steps, start=0, env_offset=0, seed=SEED):
    """[E, steps] int8: the uniform random actions of the backtest's draws (Philox stream 4 over (env, day), the
    second uniform: min(int(u2 * 3), 2)) -- what ``greedy=False`` with epsilon 0 plays."""
    from sharetrade.utils import rng

    ids = (np.arange(E, dtype=np.uint64) + np.uint64(env_offset)).astype(np.uint32)
    out = np.empty((E, steps), dtype=np.int8)
    for i in range(steps):
        _, u2 = rng.uniforms(seed, 0, ids, start + i, stream=4)
        out[:, i] = np.minimum((u2 * np.float32(3)).astype(np.int64), 2)
    return torch.from_numpy(out)


def walk(prices, actions, *, start=0, budget0=BUDGET, shares0=0, budget=None, shares=None, mut=None):
    """The ledger of every env as a dict of float64 / int64 tensors [E] plus ``curve`` float64 [steps]."""
    assert mut is None or mut in MUTATIONS, mut
    P = prices.double().tolist()
    A = actions.tolist()
    E, steps = len(A), len(A[0])
    rows = {k: [] for k in F32 + INTS}
    gains = []
    for e in range(E):
        b = float(budget0 if budget is None else budget[e])
        s = int(shares0 if shares is None else shares[e])
        v0 = P[e][start + H - 1]
        eq0 = b + s * v0
        # the env first: what was held and traded at, day by day
        eq, vs, before, after = [], [], [], []
        for i, a in enumerate(A[e]):
            v = P[e][start + i + H]
            before.append(s)
            if a == 0 and b >= v:
                b, s = b - v, s + 1
            elif a == 1 and s > 0:
                b, s = b + v, s - 1
            after.append(s)
            vs.append(v)
            eq.append(b + s * v)
        # the equity curve and its drawdowns, read off the list
        prev = [eq0] + eq[:-1]
        sumsq = sum((x - (eq0 if mut == "pnl_against_eq0" else p)) ** 2 for x, p in zip(eq, prev))
        peaks, top = [], eq0
        for x in eq:
            if mut == "peak_after_drawdown":     # the day's drawdown against the peak of the days before
                peaks.append(top)
                top = max(top, x)
            else:
                top = max(top, x)
                peaks.append(top)
        against = prev if mut == "drawdown_before_equity" else eq     # ... or of the equity before the day's trade
        max_dd = max([0.0] + [pk - x for pk, x in zip(peaks, against)])
        run, dd_days = 0, 0
        for pk, x in zip(peaks, eq):
            run = run + 1 if x < pk else (run if mut == "run_not_reset" else 0)
            dd_days = max(dd_days, run)
        # price moves against the start, positions, counts
        base = vs[0] if mut == "d_from_first_trade_price" else v0
        d = [v - base for v in vs]
        held = before if mut == "position_before_trade" else after
        refused_buy = sum(1 for a, x, y in zip(A[e], before, after) if a == 0 and x == y)
        vals = {"eq_prev": eq[-1], "eq0": eq0, "v0": v0, "v_last": vs[-1], "peak": max([eq0] + eq), "max_dd": max_dd,
                "sumsq": sumsq, "sum_d": sum(d), "sum_d2": sum(x * x for x in d),
                "sum_sd": sum(float(h) * x for h, x in zip(held, d)), "run": run, "dd_days": dd_days, "days": steps,
                "chose_buy": A[e].count(0), "chose_sell": A[e].count(1),
                "refused_buy": 0 if mut == "refused_buy_as_executed" else refused_buy,
                "refused_sell": sum(1 for a, x, y in zip(A[e], before, after) if a == 1 and x == y),
                "flat_days": sum(1 for h in held if h == 0), "max_shares": max([0] + held), "sum_s": sum(held),
                "sum_s2": sum(h * h for h in held)}
        for k, x in vals.items():
            rows[k].append(x)
        gains.append([x - eq0 for x in eq])
    if mut == "pad_rows_live":   # the rows that pad the last 16-env chunk repeat the last env
        gains += [gains[-1]] * (-E % CHUNK)
    out = {k: torch.tensor(rows[k], dtype=torch.float64) for k in F32}
    out.update({k: torch.tensor(rows[k], dtype=torch.int64) for k in INTS})
    out["curve"] = torch.tensor(gains, dtype=torch.float64).sum(0)
    return out


def bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def differs_from_walk(led, w):
    """Names of the ledger fields (and ``curve``) that are not exactly the walk's values."""
    bad = [k for k in F32 if not torch.equal(led.field(k).double().cpu(), w[k])]
    bad += [k for k in INTS if not torch.equal(led.field(k).to(torch.int64).cpu(), w[k])]
    if led.curve is not None and not torch.equal(led.curve.cpu(), w["curve"]):
        bad.append("curve")
    return bad


def same_as_walk(led, w, label=""):
    assert led.state.dtype == torch.int32 and led.state.shape == (w["days"].numel(), 24), label
    assert led.curve is None or (led.curve.dtype == torch.float64 and led.curve.shape == w["curve"].shape), label
    assert differs_from_walk(led, w) == [], (label, differs_from_walk(led, w))
    assert bool((led.state[:, 19] == 0).all()), (label, "pad word")


def same_ledger(a, b, label=""):
    """Two ledgers equal bit for bit: the records and the curve."""
    assert a.state.dtype == b.state.dtype == torch.int32 and a.state.shape == b.state.shape, label
    diff = (a.state.cpu() != b.state.cpu()).any(0).nonzero().flatten().tolist()
    assert diff == [], (label, "record words", diff)
    assert (a.curve is None) == (b.curve is None), label
    if a.curve is not None:
        assert a.curve.dtype == b.curve.dtype == torch.float64 and a.curve.shape == b.curve.shape, label
        assert torch.equal(bits(a.curve.cpu()), bits(b.curve.cpu())), (label, "curve")


def pieces_reproduce(whole, a, b, label=""):
    """A run cut in two with the state carried: the second piece's records are the whole run's and the curves
    concatenate."""
    assert torch.equal(b.state.cpu(), whole.state.cpu()), (label, "state")
    assert torch.equal(bits(torch.cat([a.curve, b.curve]).cpu()), bits(whole.curve.cpu())), (label, "curve")
