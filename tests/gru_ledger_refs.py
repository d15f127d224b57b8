"""Shared pieces of the GRU risk-ledger tests (tests/test_gru_ledger.py on the CPU, tests/test_gpu_gru_ledger.py on
the GPU): an independent plain-Python float64 walk of the minute env and its ledger, hand-built runs whose bar
returns and cost are dyadic (every float32 sum and product is exact, so the float64 walk and a float32 ledger
agree to the bit), and the comparisons both tests use.

The walk is written differently from ``sharetrade/serve/gru_rollout.py::ledger_from_trace`` on purpose: it keeps
the whole equity list and reads drawdowns off it afterwards, collects each round trip's rewards in a list, and
groups the bars of an episode column by index.  ``mut`` applies one deliberate error (what a wrong kernel would
compute); tests/test_gru_ledger.py shows that the comparisons notice each.
"""
import torch

MUTATIONS = ("peak_after_dd", "dd_before_cum", "cost_at_forced_flat", "pad_rows_live")
CHUNK = 32
STATS = ("max_dd", "dd_bars", "sumsq", "trips", "wins", "win_sum", "loss_sum")


def walk(actions, ret, cost, *, start, origin, ep_len, position=None, mut=""):
    """actions [E][steps] ints, ret [E][T] floats (the return of bar t), ``position`` [E] before bar ``start``.
    Returns per-env lists (and ``curve`` [steps], ``reward`` [E][steps]) in float64, a fresh ledger."""
    E, steps = len(actions), len(actions[0])
    es0 = origin + (start - origin) // ep_len * ep_len
    n_ep = (start + steps - 1 - es0) // ep_len + 1
    out = {k: [] for k in STATS + ("cum", "peak", "trip", "ep", "run", "ep_tr", "ep_ret", "ep_trades", "reward",
                                   "position")}
    for e in range(E):
        pos = 0 if position is None else int(position[e])
        equity, rewards, trades_at = [], [], []
        trips, open_trip = [], None     # closed trips as lists of rewards; the open one
        if pos == 1:
            open_trip = []
        eq = 0.0
        for i in range(steps):
            t = start + i
            done = (t + 1 - origin) % ep_len == 0
            a = actions[e][i]
            new = 1 if a == 0 else 0 if a == 1 else pos
            trade = new != pos
            rw = new * ret[e][t] - (cost if trade else 0.0)
            forced = done and new == 1
            if forced and mut == "cost_at_forced_flat":
                rw -= cost
            if trade and new == 1:
                open_trip = [rw]
            elif pos == 1:
                open_trip.append(rw)
            if (trade and new == 0) or forced:
                trips.append(open_trip)
                open_trip = None
            pos = 0 if done else new
            eq += rw
            equity.append(eq)
            rewards.append(rw)
            trades_at.append(1 if trade else 0)
        # drawdowns off the equity list (the peak starts at 0, the curve's value before the first bar)
        peak, max_dd, run, dd_bars = 0.0, 0.0, 0, 0
        for j, v in enumerate(equity):
            if mut == "dd_before_cum":     # the drawdown of the curve before this bar's reward
                prev = equity[j - 1] if j else 0.0
                peak = max(peak, v)
                max_dd = max(max_dd, peak - prev)
            elif mut == "peak_after_dd":
                max_dd = max(max_dd, peak - v)
                peak = max(peak, v)
            else:
                peak = max(peak, v)
                max_dd = max(max_dd, peak - v)
            run = run + 1 if v < peak else 0
            dd_bars = max(dd_bars, run)
        sums = [sum(tr) for tr in trips]
        cols = [[i for i in range(steps) if (start + i - es0) // ep_len == k] for k in range(n_ep)]
        last_col_open = (start + steps - es0) % ep_len != 0     # the run ends inside an episode
        out["reward"].append(rewards)
        out["position"].append(pos)
        out["cum"].append(eq)
        out["peak"].append(peak)
        out["trip"].append(sum(open_trip) if open_trip is not None else 0.0)
        out["ep"].append(sum(rewards[i] for i in cols[-1]) if last_col_open else 0.0)
        out["ep_tr"].append(sum(trades_at[i] for i in cols[-1]) if last_col_open else 0)
        out["run"].append(run)
        out["max_dd"].append(max_dd)
        out["dd_bars"].append(dd_bars)
        out["sumsq"].append(sum(r * r for r in rewards))
        out["trips"].append(len(trips))
        out["wins"].append(sum(1 for s in sums if s > 0))
        out["win_sum"].append(sum(s for s in sums if s > 0))
        out["loss_sum"].append(sum(s for s in sums if not s > 0))
        out["ep_ret"].append([sum(rewards[i] for i in c) for c in cols])
        out["ep_trades"].append([sum(trades_at[i] for i in c) for c in cols])
    pad = (-E) % CHUNK if mut == "pad_rows_live" else 0
    out["curve"] = [sum(out["reward"][e][i] for e in range(E)) + pad * out["reward"][E - 1][i] for i in range(steps)]
    out["full"] = [es0 + k * ep_len >= start and es0 + (k + 1) * ep_len <= start + steps for k in range(n_ep)]
    return out


def check_against_walk(led, w):
    """Every field of a fresh-ledger ``GruLedger`` equals the walk's exactly (dyadic inputs: no rounding)."""
    def same(name, got, want):
        want = torch.tensor(want, dtype=torch.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert torch.equal(got.double().cpu(), want), (name, got.tolist(), want.tolist())

    for k in STATS:
        same(k, getattr(led, k), w[k])
    for k in ("cum", "peak", "trip", "ep", "run", "ep_tr"):
        same(k, led.state_field(k), w[k])
    same("ep_ret", led.ep_ret, w["ep_ret"])
    same("ep_trades", led.ep_trades, w["ep_trades"])
    same("curve", led.curve, w["curve"])
    assert list(led.full) == w["full"]
    assert bool((led.state[:, 6:] == 0).all())


def bits(t):
    return t.view(torch.int32) if t.is_floating_point() else t


def same_ledger(a, b, fields=None, label=""):
    """Two ledgers equal bit for bit (all tensor fields, or ``fields``)."""
    names = fields or ("ep_ret", "ep_trades", "state", "curve") + STATS
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape, (label, k, x.dtype, y.dtype, x.shape, y.shape)
        assert torch.equal(bits(x.cpu()), bits(y.cpu())), (label, k)
    if fields is None:
        assert list(a.full) == list(b.full), label


def pieces_reproduce(whole, a, b, cut_col, label=""):
    """A run cut in two with the state carried: the second piece's state is the whole's, the curves concatenate,
    the episode columns are the first piece's up to the split episode's (``cut_col``) and the second piece's from
    there on (``ep`` is carried, so the second piece's first column holds the whole split episode), counts add
    and the per-piece maxima combine to the whole's."""
    assert torch.equal(b.state.cpu(), whole.state.cpu()), (label, "state")
    assert torch.equal(bits(torch.cat([a.curve, b.curve]).cpu()), bits(whole.curve.cpu())), (label, "curve")
    for k in ("ep_ret", "ep_trades"):
        got = torch.cat([getattr(a, k)[:, :cut_col], getattr(b, k)], dim=1)
        assert torch.equal(bits(got.cpu()), bits(getattr(whole, k).cpu())), (label, k)
    for k in ("trips", "wins"):
        assert torch.equal((getattr(a, k) + getattr(b, k)).cpu(), getattr(whole, k).cpu()), (label, k)
    for k in ("max_dd", "dd_bars"):
        assert torch.equal(bits(torch.maximum(getattr(a, k), getattr(b, k)).cpu()), bits(getattr(whole, k).cpu())), \
            (label, k)


def closed_trips_and_carried_longs(actions, position, start, origin, ep_len):
    """From an action trace: (closed round trips per env, longs held across an episode end in all)."""
    acts = actions.tolist()
    trips, carried = [], 0
    for e, row in enumerate(acts):
        pos, n = (0 if position is None else int(position[e])), 0
        for i, a in enumerate(row):
            t = start + i
            done = (t + 1 - origin) % ep_len == 0
            new = 1 if a == 0 else 0 if a == 1 else pos
            if (new != pos and new == 0) or (done and new == 1):
                n += 1
            carried += 1 if done and new == 1 else 0
            pos = 0 if done else new
        trips.append(n)
    return trips, carried
