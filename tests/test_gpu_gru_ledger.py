"""The ledger instance of the GRU rollout kernel (``csrc/gru_rollout.hip``: ``st_gru_rollout_ledger_launch``) against
``ledger_from_trace`` of its own trace, the plain instance, itself on another grid and itself cut in two.

Shape: 37 series (two chunks, the second with 5 live rows), 70 bars, episodes of 13 bars from bar 1, bars 3 .. 63:
a partial first column (3 .. 13), the whole episodes 14 .. 26, 27 .. 39 and 40 .. 52, and a partial last column
(53 .. 63): five columns, three of them whole (61 bars from bar 3 cannot hold a fourth whole episode of 13).  The policy is randomly initialised and run with epsilon 0.5, so its actions vary; seed 3 gives every
series at least three closed round trips and 68 longs held across an episode end on the CPU (torch backend).

The ledger is exact float32 arithmetic downstream of the rewards, so every comparison is bit for bit; the
portfolio curve is also held to the bound of an fp32 summation of E terms against the float64 column sum.
"""
import pytest
import torch

import gru_backtest_refs as R
import gru_ledger_refs as LR

pytestmark = pytest.mark.gpu

SEED = 3
E, T, EP_LEN, START, ORIGIN, STEPS, COST = 37, 70, 13, 3, 1, 61, 0.01
PLAIN = ("ret", "trades", "long", "position", "entry", "h")
KW = dict(ep_len=EP_LEN, cost=COST, origin=ORIGIN, greedy=False, epsilon=0.5)


@pytest.fixture(scope="module")
def runs(native_built):
    """The launches every test reads: plain, ledger, ledger with trace, ledger on one and two workgroups."""
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import GruPolicy

    close, feat = R.bars(E, T)
    close, feat = close.cuda(), feat.cuda()
    pol = GruPolicy(gq.init_params(SEED), device=torch.device("cuda", 0), seed=SEED)
    kw = dict(start=START, steps=STEPS, **KW)
    out = {"pol": pol, "close": close, "feat": feat,
           "plain": pol.backtest(close, feat, **kw),
           "ledger": pol.backtest(close, feat, ledger=True, **kw),
           "traced": pol.backtest(close, feat, ledger=True, trace=True, **kw),
           "grid1": pol.backtest(close, feat, ledger=True, grid=1, **kw),
           "grid2": pol.backtest(close, feat, ledger=True, grid=2, **kw)}
    torch.cuda.synchronize()
    return out


def _same_plain(a, b, label):
    for k in PLAIN:
        assert torch.equal(LR.bits(getattr(a, k)), LR.bits(getattr(b, k))), (label, k)


def test_trace_has_trips_and_longs_across_episode_ends(runs):
    tr = runs["traced"]
    trips, carried = LR.closed_trips_and_carried_longs(tr.actions.cpu(), None, START, ORIGIN, EP_LEN)
    print(f"[meas] closed trips per env min {min(trips)} max {max(trips)}, longs held across an episode end {carried}")
    assert max(trips) >= 2 and carried >= 1
    assert len(set(tr.actions.cpu().flatten().tolist())) == 3


def test_ledger_equals_ledger_from_trace_bit_for_bit(runs):
    from sharetrade.serve.gru_rollout import ledger_from_trace

    tr, led = runs["traced"], runs["ledger"].ledger
    assert runs["plain"].ledger is None and runs["ledger"].actions is None
    want = ledger_from_trace(tr.actions.cpu(), tr.reward.cpu(), start=START, origin=ORIGIN, ep_len=EP_LEN)
    assert want.ep_ret.shape == (E, 5) and want.full == [False, True, True, True, False]
    assert int(want.trips.sum()) > 0 and float(want.max_dd.max()) > 0 and int(want.dd_bars.max()) > 1
    LR.same_ledger(led, want, label="ledger launch")
    LR.same_ledger(tr.ledger, want, label="ledger launch with trace")
    assert bool((led.state[:, 6:] == 0).all())
    # the same oracle on the GPU tensors (what the ledger launch replaces on the device)
    LR.same_ledger(ledger_from_trace(tr.actions, tr.reward, start=START, origin=ORIGIN, ep_len=EP_LEN), want,
                   label="oracle on the device")


def test_curve_within_the_fp32_summation_bound(runs):
    rw = runs["traced"].reward.double().cpu()
    curve = runs["ledger"].ledger.curve.double().cpu()
    assert curve.shape == (STEPS,)
    err = (curve - rw.sum(0)).abs()
    bound = (E - 1) * 2.0 ** -24 * rw.abs().sum(0)
    print(f"[meas] curve: max |err| {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}")
    assert bool((err <= bound).all())


def test_plain_outputs_of_the_ledger_launch_equal_the_plain_launch(runs):
    _same_plain(runs["ledger"], runs["plain"], "ledger vs plain")
    _same_plain(runs["traced"], runs["plain"], "ledger with trace vs plain")
    assert torch.equal(LR.bits(runs["ledger"].ledger.state_field("cum")), LR.bits(runs["plain"].ret))


def test_grid_one_and_two_give_identical_ledgers(runs):
    LR.same_ledger(runs["grid1"].ledger, runs["grid2"].ledger, label="grid 1 vs 2")
    LR.same_ledger(runs["grid1"].ledger, runs["ledger"].ledger, label="grid 1 vs one workgroup per chunk")
    _same_plain(runs["grid1"], runs["plain"], "grid 1 vs plain")


def test_pieces_reproduce_the_whole(runs):
    """Bars 3 .. 22 then 23 .. 63 with h, position, entry and the ledger state carried."""
    from sharetrade.serve.gru_rollout import episode_columns

    pol, close, feat, whole = runs["pol"], runs["close"], runs["feat"], runs["ledger"]
    cut = 20
    a = pol.backtest(close, feat, start=START, steps=cut, ledger=True, **KW)
    b = pol.backtest(close, feat, start=START + cut, steps=STEPS - cut, ledger=True, h0=a.h, position=a.position,
                     entry=a.entry, ledger_state=a.ledger.state, **KW)
    torch.cuda.synchronize()
    n_a = episode_columns(START, cut, ORIGIN, EP_LEN)[1]
    assert n_a == 2 and (START + cut - ORIGIN) % EP_LEN != 0     # the cut lies inside the second column
    LR.pieces_reproduce(whole.ledger, a.ledger, b.ledger, n_a - 1, label="20 + 41")
    for k in ("position", "entry", "h"):
        assert torch.equal(LR.bits(getattr(b, k)), LR.bits(getattr(whole, k))), k
    assert torch.equal(a.trades + b.trades, whole.trades) and torch.equal(a.long + b.long, whole.long)


def test_one_bar_of_one_full_chunk(runs):
    from sharetrade.serve.gru_rollout import ledger_from_trace

    pol, close, feat = runs["pol"], runs["close"][:32].contiguous(), runs["feat"][:32].contiguous()
    res = pol.backtest(close, feat, start=START, steps=1, ledger=True, trace=True, **KW)
    torch.cuda.synchronize()
    led = res.ledger
    assert led.ep_ret.shape == (32, 1) and led.curve.shape == (1,) and led.full == [False]
    want = ledger_from_trace(res.actions.cpu(), res.reward.cpu(), start=START, origin=ORIGIN, ep_len=EP_LEN)
    LR.same_ledger(led, want, label="one bar")
    assert torch.equal(LR.bits(led.ep_ret[:, 0]), LR.bits(res.ret))


def test_launcher_refuses_inconsistent_ledger_arguments(runs):
    """Return codes only: hipErrorInvalidValue before anything is launched."""
    import ctypes as C
    import math

    from sharetrade.ops import gru as G
    from sharetrade.ops import native

    pol, close, feat = runs["pol"], runs["close"], runs["feat"]
    ret = torch.zeros(E, T, device="cuda")
    i32 = torch.int32
    keep = {"out_ret": torch.zeros(E, device="cuda"), "out_trades": torch.zeros(E, dtype=i32, device="cuda"),
            "out_long": torch.zeros(E, dtype=i32, device="cuda"), "out_position": torch.zeros(E, dtype=i32, device="cuda"),
            "out_entry": torch.zeros(E, device="cuda")}
    led = {"ep_ret": torch.full((E, 5), -7.0, device="cuda"), "ep_trades": torch.zeros(E, 5, dtype=i32, device="cuda"),
           "state_out": torch.zeros(E, 8, dtype=i32, device="cuda"), "stats": torch.zeros(E, 8, dtype=i32, device="cuda"),
           "part": torch.zeros(2, 64, device="cuda"), "curve": torch.full((STEPS,), -7.0, device="cuda")}

    def args(**over):
        q = G.RolloutLedgerArgs()
        a = q.r
        for n, t in pol.packed.items():
            setattr(a, n, t.data_ptr())
        a.feat, a.close, a.ret = feat.data_ptr(), close.data_ptr(), ret.data_ptr()
        for k, t in keep.items():
            setattr(a, k, t.data_ptr())
        a.E, a.T, a.start, a.steps, a.origin, a.ep_len = E, T, START, STEPS, ORIGIN, EP_LEN
        a.eps, a.cost, a.inv_ep_len = math.inf, COST, 1.0 / EP_LEN
        for k, t in led.items():
            setattr(q.l, k, t.data_ptr())
        q.l.n_ep, q.l.part_stride = 5, 64
        for k, v in over.items():
            setattr(q.l if hasattr(q.l, k) else a, k, v)
        return q

    L = G.lib()
    INVALID = 1
    for over in (dict(n_ep=4), dict(n_ep=6), dict(part_stride=61), dict(part_stride=96), dict(ep_ret=None),
                 dict(stats=None), dict(part=None), dict(curve=None), dict(steps=0), dict(out_ret=None)):
        assert L.st_gru_rollout_ledger_launch(C.byref(args(**over)), 0, native.stream_handle()) == INVALID, over
    torch.cuda.synchronize()
    assert bool((led["ep_ret"] == -7).all()) and bool((led["curve"] == -7).all())   # nothing ran
    # the ledger without a curve, and the curve without a ledger, are launches of their own
    assert L.st_gru_rollout_ledger_launch(C.byref(args(part=None, curve=None)), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert bool((led["curve"] == -7).all()) and not bool((led["ep_ret"] == -7).any())
    led["ep_ret"].fill_(-7.0)
    q = args(ep_ret=None, ep_trades=None, state_out=None, stats=None)
    assert L.st_gru_rollout_ledger_launch(C.byref(q), 0, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert bool((led["ep_ret"] == -7).all()) and not bool((led["curve"] == -7).any())
