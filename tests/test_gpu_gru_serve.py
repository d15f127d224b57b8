"""The GRU serving kernel (``csrc/gru_serve.hip``) against the rollout kernel it shares its per-bar arithmetic
with, against the PyTorch oracle, and against itself under other batch compositions.

Serving T bars one launch at a time must give what one rollout launch gives, bit for bit (the rollout's own
"pieces reproduce the whole" taken to pieces of one bar): actions, Q rows, rewards (a served bar returns the
reward of the session's previous bar), the running return, position, entry, h, trades and bars long.
Independently of the rollout kernel, the served trace is held to the three teacher-forced rules of
tests/gru_backtest_refs.py against the oracle, with the project's bound (a quarter of the quantisation effect).
Inputs: bars and centred weights of tests/gru_backtest_refs.py, 33 sessions x 23 bars, episodes of 5.
"""
import ctypes as C
import math

import pytest
import torch

import gru_backtest_refs as R
import gru_serve_refs as SR

pytestmark = pytest.mark.gpu

SEED = 3
E, STEPS, EP = 33, 23, 5
ROLL_KEYS = ("ret", "trades", "long", "position", "entry", "h", "actions", "q", "reward")


def _policy(params=None, seed=SEED):
    from sharetrade.serve.gru_rollout import GruPolicy

    return GruPolicy(params or R.centred_params(3, E, STEPS, EP), device=torch.device("cuda", 0), seed=seed)


def _server(pol=None, S=64, ep_len=EP):
    from sharetrade.serve.gru_serve import GruSessionServer

    return GruSessionServer(pol or _policy(), S, ep_len=ep_len, backend="hip")


def _open_shuffled(srv, n, seed=5):
    """n sessions on a shuffled choice of slots (slot != row), draw ids = env indices."""
    want = torch.randperm(srv.S, generator=torch.Generator().manual_seed(seed))[:n].tolist()
    got = srv.open(srv.S)
    srv.close([s for s in got if s not in set(want)])
    srv.view("draw_id")[torch.tensor(want, device="cuda")] = torch.arange(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return want


def _rollout(pol, close, feat, **kw):
    res = pol.backtest(close.cuda(), feat.cuda(), trace=True, **kw)
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu() for k in ROLL_KEYS}


def _state(srv, slots):
    return {k: v.cpu() for k, v in srv.state(slots).items()}


_served = {}


def _case1(eps):
    """Case 1's run, once per epsilon: 23 served bars, the state after them, then a 24th bar that realises the
    reward of bar 22 (for the oracle check); the rollout launch over the same 23 bars."""
    if eps not in _served:
        close, feat = R.bars(E, STEPS + 8)
        pol = _policy()
        srv = _server(pol)
        slots = _open_shuffled(srv, E)
        kw = {} if eps is None else dict(greedy=False, epsilon=eps)
        tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS, **kw)
        st = _state(srv, slots)
        last = SR.serve_lockstep(srv, slots, close, feat, STEPS, 1, shuffle_seed=9, **kw)
        roll = _rollout(pol, close, feat, steps=STEPS, ep_len=EP, **kw)
        _served[eps] = (tr, st, last, _state(srv, slots), roll)
    return _served[eps]


@pytest.mark.parametrize("eps", [None, 0.6, 0.0])
def test_served_bar_by_bar_equals_one_rollout_launch(native_built, eps):
    tr, st, _, _, roll = _case1(eps)
    assert SR.against_rollout(tr, st, roll, STEPS) == []
    assert bool((st["bars"] == STEPS).all()) and bool((st["elapsed"] == STEPS % EP).all())
    if eps == 0.0:
        ex, rnd = R.mirror_draws(SEED, E, 0, STEPS, 0.0)
        assert not bool(ex.any()) and torch.equal(tr["actions"].long(), rnd)
    elif eps is None:
        assert min(R.action_shares(tr["actions"])) >= 0.10
    assert int(st["trades"].sum()) > 0 and len(set(tr["actions"].flatten().tolist())) == 3


@pytest.mark.parametrize("eps", [None, 0.6])
def test_served_trace_against_the_oracle(native_built, eps):
    """Rules (a), (b), (c) on the served trace alone: the oracle replays the served actions."""
    tr, st, last, st_last, _ = _case1(eps)
    close, feat = R.bars(E, STEPS + 8)
    params = R.centred_params(3, E, STEPS, EP)
    # rewards 0 .. 22 as served at bars 1 .. 23; the return after bar 23 is their sum
    reward = torch.cat([tr["reward"][:, 1:], last["reward"]], dim=1)
    out = {"actions": tr["actions"], "q": tr["q"], "reward": reward, "ret": st_last["ret"],
           "trades": st["trades"], "long": st["long"], "position": st["position"], "entry": st["entry"]}
    bound, ref = R.q_bound(params, close, feat, out["actions"], steps=STEPS, ep_len=EP)
    ex = rnd = None
    if eps is not None:
        ex, rnd = R.mirror_draws(SEED, E, 0, STEPS, eps)
        assert 0.3 < float(ex.float().mean()) < 0.9
    R.check_trace(out, ref, bound, exploit=ex, rnd=rnd, label=f"served E={E} steps={STEPS} ep_len={EP} eps={eps}")


def test_ragged_progress_equals_lockstep(native_built):
    n, bars_each, S = 48, 20, 64
    close, feat = R.bars(n, bars_each + 8)
    pol = _policy()
    a, b = _server(pol, S), _server(pol, S)
    sa, sb = a.open(n), b.open(n)
    # never-opened slots carry a sentinel pattern
    b.table["h"][n:] = 7.5
    b.table["rec"][n:] = 0x5A5A5A5A
    snap = {k: t.clone() for k, t in b.table.items()}

    def untouched(batch_slots):
        torch.cuda.synchronize()
        keep = torch.ones(S, dtype=torch.bool, device="cuda")
        keep[batch_slots.cuda()] = False
        for k, t in b.table.items():
            assert torch.equal(SR.bits(t[keep]), SR.bits(snap[k][keep])), k
            assert not torch.equal(SR.bits(t[~keep]), SR.bits(snap[k][~keep])), k   # the batch's rows did move
            snap[k].copy_(t)

    base = SR.serve_lockstep(a, sa, close, feat, 0, bars_each)
    tr, sizes = SR.serve_ragged(b, sb, close, feat, bars_each, after_call=untouched)
    assert {1, 32, 33} <= set(sizes)
    for k in SR.TRACE:
        assert SR.same(tr[k], base[k]), k
    x, y = _state(a, sa), _state(b, sb)
    for k in x:
        assert SR.same(x[k], y[k]), k
    assert bool((b.table["h"][n:] == 7.5).all()) and bool((b.table["rec"][n:] == 0x5A5A5A5A).all())


def _step_into(srv, slots, feat, close, flags=None, grid=0, eps=math.inf):
    B = slots.numel()
    out = {"actions": torch.full((B,), -9, dtype=torch.int8, device="cuda"),
           "position": torch.full((B,), -9, dtype=torch.int32, device="cuda"),
           "reward": torch.full((B,), -9.0, device="cuda"), "q": torch.full((B, 3), -9.0, device="cuda")}
    srv.step_into(slots.to(torch.int32).cuda(), feat.cuda().contiguous(), close.cuda().contiguous(), flags,
                  out["actions"], out["position"], out["reward"], out["q"], epsilon=eps, grid=grid)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_padding_rows(native_built):
    """slot = -1 (and one past the table) mixed into a batch of 40 rows, on the third bar of the sessions."""
    n, S = 34, 64
    close, feat = R.bars(n, STEPS + 8)
    pol = _policy()
    a, b = _server(pol, S), _server(pol, S)
    sa, sb = a.open(n), b.open(n)
    for t in range(2):
        SR.serve_lockstep(a, sa, close, feat, t, 1)
        SR.serve_lockstep(b, sb, close, feat, t, 1)
    rows = torch.full((40,), -1, dtype=torch.int64)
    where = torch.randperm(40, generator=torch.Generator().manual_seed(1))[:n].sort().values
    rows[where] = torch.arange(n)
    pad = rows < 0
    slots = torch.where(pad, torch.tensor(-1), torch.tensor(sa)[rows.clamp(min=0)])
    slots[torch.nonzero(pad).flatten()[0]] = S   # one past the table
    f, c = feat[rows.clamp(min=0), 2], close[rows.clamp(min=0), 2]
    snap = {k: t.clone() for k, t in a.table.items()}
    got = _step_into(a, slots, f, c)
    want = _step_into(b, slots[~pad], f[~pad], c[~pad])
    assert bool((got["actions"][pad] == -1).all()) and bool((got["actions"][~pad] >= 0).all())
    for k in got:
        assert SR.same(got[k][~pad], want[k]), k
    for k in a.table:
        assert torch.equal(SR.bits(a.table[k]), SR.bits(b.table[k])), k
        assert torch.equal(SR.bits(a.table[k][n:]), SR.bits(snap[k][n:])), k


def test_grid_strides_over_chunks(native_built):
    """100 requests = 4 chunks (the last partial) on 1 and 3 workgroups: bit-equal to the default grid."""
    n, bars_n, S = 100, 7, 128
    close, feat = R.bars(n, bars_n + 8)
    pol = _policy()
    runs = []
    for grid in (0, 1, 3):
        srv = _server(pol, S, ep_len=4)
        slots = _open_shuffled(srv, n)
        tr = SR.serve_lockstep(srv, slots, close, feat, 0, bars_n, grid=grid)
        runs.append((tr, _state(srv, slots)))
    roll = _rollout(pol, close, feat, steps=bars_n, ep_len=4)
    assert SR.against_rollout(runs[0][0], runs[0][1], roll, bars_n) == []
    for tr, st in runs[1:]:
        for k in SR.TRACE:
            assert SR.same(tr[k], runs[0][0][k]), k
        for k in st:
            assert SR.same(st[k], runs[0][1][k]), k


def test_new_episode_flag(native_built):
    """The flag at bar 9: from there on the trace of a fresh backtest(start=9, origin=9); reward 0 at bar 9."""
    close, feat = R.bars(E, STEPS + 8)
    pol = _policy()
    srv = _server(pol)
    slots = _open_shuffled(srv, E)
    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS, flag_bar=9)
    st = _state(srv, slots)
    fresh = _rollout(pol, close, feat, start=9, steps=STEPS - 9, ep_len=EP, origin=9)
    assert SR.same(tr["actions"][:, 9:], fresh["actions"]) and SR.same(tr["q"][:, 9:], fresh["q"])
    assert bool((tr["reward"][:, 9] == 0).all()) and SR.same(tr["reward"][:, 10:], fresh["reward"][:, :-1])
    for k in ("position", "entry", "h"):
        assert SR.same(st[k], fresh[k]), k
    before = _rollout(pol, close, feat, steps=9, ep_len=EP)
    assert SR.same(tr["actions"][:, :9], before["actions"])
    # the counters stay: bars served, trades and bars long run on over the flag
    assert bool((st["bars"] == STEPS).all())
    assert torch.equal(st["trades"], before["trades"] + fresh["trades"])
    assert torch.equal(st["long"], before["long"] + fresh["long"])
    assert SR.same(st["ret"], SR.seq_sum(torch.cat([before["reward"][:, :8], fresh["reward"][:, :-1]], dim=1)))


def test_hot_swap_keeps_the_sessions(native_built):
    """load_policy at bar 10 = the rollout continued in pieces with the second policy."""
    from sharetrade.models import gru_qnet as gq

    close, feat = R.bars(E, STEPS + 8)
    pb = gq.init_params(7)
    pb["w_q"] = 30.0 * pb["w_q"]
    pol_a, pol_b = _policy(), _policy(pb)
    srv = _server(pol_a)
    slots = _open_shuffled(srv, E)
    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS,
                           before_bar=lambda t: srv.load_policy(pol_b) if t == 10 else None)
    st = _state(srv, slots)
    a = _rollout(pol_a, close, feat, steps=10, ep_len=EP)
    b = _rollout(pol_b, close, feat, start=10, steps=STEPS - 10, ep_len=EP, origin=0, h0=a["h"].cuda(),
                 position=a["position"].cuda(), entry=a["entry"].cuda())
    both = {k: torch.cat([a[k], b[k]], dim=1) for k in ("actions", "q", "reward")}
    for k in ("position", "entry", "h"):
        both[k] = b[k]
    both["trades"], both["long"] = a["trades"] + b["trades"], a["long"] + b["long"]
    assert SR.against_rollout(tr, st, both, STEPS) == []
    assert not SR.same(tr["q"][:, 10:], _case1(None)[0]["q"][:, 10:])


def test_stream_and_refusals(native_built):
    from sharetrade.ops import gru as G
    from sharetrade.ops import native

    close, feat = R.bars(E, STEPS + 8)
    pol = _policy()
    a, b = _server(pol), _server(pol)
    sa, sb = a.open(E), b.open(E)
    sl = torch.tensor(sa)
    want = [_step_into(a, sl, feat[:, t], close[:, t]) for t in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = [_step_into(b, sl, feat[:, t], close[:, t]) for t in range(3)]
    for w, g in zip(want, got):
        for k in w:
            assert SR.same(w[k], g[k]), k
    for k in a.table:
        assert torch.equal(SR.bits(a.table[k]), SR.bits(b.table[k])), k
    # the host API
    f, c = feat[:2, 3], close[:2, 3]
    snap = {k: t.clone() for k, t in a.table.items()}
    for bad in ([sa[0], sa[0]], [sa[0], a.S], [sa[0], -1]):
        with pytest.raises(ValueError):
            a.step(bad, f, c)
    a.close([sa[1]])
    with pytest.raises(ValueError, match="not open"):
        a.step([sa[0], sa[1]], f, c)
    # the launcher: return codes only, hipErrorInvalidValue before anything is launched
    B = 4
    dev = dict(device="cuda")
    slot = torch.tensor(sa[2:2 + B], dtype=torch.int32, **dev)
    ff, cc = feat[:B, 3].cuda().contiguous(), close[:B, 3].cuda().contiguous()
    outs = {"action": torch.full((B,), -7, dtype=torch.int8, **dev),
            "position": torch.full((B,), -7, dtype=torch.int32, **dev), "reward": torch.full((B,), -7.0, **dev)}

    def args(**over):
        p = G.ServeArgs()
        for n, t in pol.packed.items():
            setattr(p, n, t.data_ptr())
        p.slot, p.feat, p.close, p.flags = slot.data_ptr(), ff.data_ptr(), cc.data_ptr(), None
        p.h, p.rec = a.table["h"].data_ptr(), a.table["rec"].data_ptr()
        for k, t in outs.items():
            setattr(p, k, t.data_ptr())
        p.q = None
        p.B, p.S, p.ep_len = B, a.S, EP
        p.eps, p.cost, p.inv_ep_len = math.inf, 0.01, 0.2
        for k, v in over.items():
            setattr(p, k, v)
        return p

    L = G.lib()
    INVALID = 1
    for over in (dict(B=0), dict(S=0), dict(ep_len=0), dict(slot=None), dict(h=None), dict(rec=None),
                 dict(action=None), dict(whh8=None), dict(close=None)):
        assert L.st_gru_serve_launch(C.byref(args(**over)), 0, native.stream_handle()) == INVALID, over
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == -7).all()), k   # nothing ran
    for k in a.table:
        assert torch.equal(SR.bits(a.table[k]), SR.bits(snap[k])), k
    assert L.st_gru_serve_launch(C.byref(args()), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert bool((outs["action"] >= 0).all())


def test_serve_struct_matches(native_built):
    """The ctypes mirrors against the C++ structs' sizes (no HIP call)."""
    from sharetrade.ops import gru as G

    L = G.lib()
    n = L.st_abi_gru_serve(None, 0)
    out = (C.c_int * n)()
    assert L.st_abi_gru_serve(out, n) == n
    assert list(out) == [C.sizeof(G.ServeArgs), C.sizeof(G.ServeRec), 4 * G.SERVE_REC_WORDS]
    assert C.sizeof(G.ServeArgs) == 15 * 8 + 8 * 4 and 0 < L.st_gru_serve_lds_bytes() <= 160 * 1024
