"""Serving a GRU(256) policy through sessions, on the CPU: the torch backend of ``GruSessionServer`` (the oracle
``reference_gru_serve``) against ``reference_gru_rollout``, ragged against lockstep serving, the batcher's
per-session order, the HTTP routes and the CLI's choice of path.  The inputs are those of
tests/gru_backtest_refs.py: bars(33, 31) and the centred weights whose greedy policy uses every action."""
import argparse

import pytest
import torch

import gru_backtest_refs as R
import gru_serve_refs as SR

E, STEPS, EP = 33, 23, 5
CPU = torch.device("cpu")


def _policy(params=None, seed=3):
    from sharetrade.serve.gru_rollout import GruPolicy

    return GruPolicy(params or R.centred_params(3, E, STEPS, EP), device=CPU, seed=seed)


def _server(pol=None, S=64, **kw):
    from sharetrade.serve.gru_serve import GruSessionServer

    return GruSessionServer(pol or _policy(), S, ep_len=EP, backend="torch", **kw)


def _shuffled_slots(S, n, seed=5):
    return torch.randperm(S, generator=torch.Generator().manual_seed(seed))[:n].tolist()


def _open(srv, n):
    """n sessions on shuffled slots (slot != row), draw ids = env indices."""
    want = _shuffled_slots(srv.S, n)
    got = srv.open(srv.S)
    srv.close([s for s in got if s not in set(want)])
    for e, s in enumerate(want):
        srv.view("draw_id")[s] = e
    return want


@pytest.fixture(scope="module")
def rollout():
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    close, feat = R.bars(E, STEPS + 8)
    return reference_gru_rollout(R.centred_params(3, E, STEPS, EP), close, feat, steps=STEPS, ep_len=EP, seed=3)


@pytest.mark.parametrize("eps", [None, 0.6])
def test_served_bar_by_bar_equals_the_rollout_oracle(rollout, eps):
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    close, feat = R.bars(E, STEPS + 8)
    roll = rollout if eps is None else reference_gru_rollout(R.centred_params(3, E, STEPS, EP), close, feat,
                                                             steps=STEPS, ep_len=EP, seed=3, epsilon=eps)
    srv = _server()
    slots = _open(srv, E)
    kw = {} if eps is None else dict(greedy=False, epsilon=eps)
    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS, **kw)
    st = srv.state(slots)
    assert SR.against_rollout(tr, st, roll, STEPS) == []
    assert bool((st["bars"] == STEPS).all()) and bool((st["elapsed"] == STEPS % EP).all())
    assert min(R.action_shares(tr["actions"])) >= 0.10
    assert srv.bars_served == E * STEPS and srv.batches == STEPS


def test_a_stale_state_is_rejected(rollout):
    """A session served with another session's h at bar 21 (no reset follows): the comparison with the rollout
    fails."""
    close, feat = R.bars(E, STEPS + 8)
    srv = _server()
    slots = _open(srv, E)

    def swap(t):
        if t == 21:
            h = srv.view("h")
            h[slots[0]], h[slots[1]] = h[slots[1]].clone(), h[slots[0]].clone()

    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS, before_bar=swap)
    bad = SR.against_rollout(tr, srv.state(slots), rollout, STEPS)
    assert "q" in bad and "h" in bad


def test_ragged_progress_equals_lockstep():
    n, bars_each = 48, 20
    close, feat = R.bars(n, bars_each + 8)
    a, b = _server(), _server()
    sa, sb = _open(a, n), _open(b, n)
    base = SR.serve_lockstep(a, sa, close, feat, 0, bars_each)
    tr, sizes = SR.serve_ragged(b, sb, close, feat, bars_each)
    assert {1, 32, 33} <= set(sizes)
    for k in SR.TRACE:
        assert SR.same(tr[k], base[k]), k
    x, y = a.state(sa), b.state(sb)
    for k in x:
        assert SR.same(x[k], y[k]), k


def test_new_episode_flag_and_padding_rows():
    from sharetrade.serve.gru_rollout import reference_gru_rollout
    from sharetrade.serve.gru_serve import new_table, reference_gru_serve

    close, feat = R.bars(E, STEPS + 8)
    params = R.centred_params(3, E, STEPS, EP)
    srv = _server()
    slots = _open(srv, E)
    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS, flag_bar=9)
    fresh = reference_gru_rollout(params, close, feat, start=9, steps=STEPS - 9, ep_len=EP, origin=9)
    assert SR.same(tr["actions"][:, 9:], fresh["actions"]) and SR.same(tr["q"][:, 9:], fresh["q"])
    assert bool((tr["reward"][:, 9] == 0).all()) and SR.same(tr["reward"][:, 10:], fresh["reward"][:, :-1])
    # padding rows: action -1, nothing touched, the others as without them
    ta, tb = new_table(8, CPU, torch.float64), new_table(8, CPU, torch.float64)
    sl = torch.tensor([3, -1, 5, 8, 0])
    keep = sl.ge(0) & sl.lt(8)
    oa = reference_gru_serve(params, ta, sl, feat[:5, 0], close[:5, 0], ep_len=EP)
    ob = reference_gru_serve(params, tb, sl[keep], feat[:5, 0][keep], close[:5, 0][keep], ep_len=EP)
    assert oa["actions"][~keep].tolist() == [-1, -1]
    for k in oa:
        assert SR.same(oa[k][keep], ob[k]), k
    assert torch.equal(ta["rec"], tb["rec"]) and torch.equal(ta["h"], tb["h"])
    assert bool((ta["rec"][[1, 2, 4, 6, 7]] == 0).all())


def test_host_checks_and_hot_swap():
    from sharetrade.models import gru_qnet as gq
    from sharetrade.serve.gru_rollout import reference_gru_rollout

    close, feat = R.bars(E, STEPS + 8)
    srv = _server(S=8)
    s = srv.open(3)
    assert s == [0, 1, 2] and srv.view("draw_id")[:3].tolist() == [0, 1, 2]
    f, c = feat[:2, 0], close[:2, 0]
    for bad in ([0, 0], [0, 8], [0, -1], [0, 5]):
        with pytest.raises(ValueError):
            srv.step(bad, f, c)
    srv.close([1])
    with pytest.raises(ValueError, match="not open"):
        srv.step([0, 1], f, c)
    assert srv.batches == 0 and not bool(srv.table["rec"][:, :10].any())
    assert srv.open(1) == [1]
    with pytest.raises(RuntimeError):
        srv.open(6)
    # weights swapped at bar 10: the rollout continued in pieces with the second policy
    pa, pb = R.centred_params(3, E, STEPS, EP), gq.init_params(7)
    pb["w_q"] = 30.0 * pb["w_q"]
    srv = _server(_policy(pa))
    slots = _open(srv, E)
    tr = SR.serve_lockstep(srv, slots, close, feat, 0, STEPS,
                           before_bar=lambda t: srv.load_policy(_policy(pb)) if t == 10 else None)
    # (the oracle carries h in float64 within a call and hands it over in float32: compare the actions, and
    # the Q rows to float32 resolution)
    a = reference_gru_rollout(pa, close, feat, steps=10, ep_len=EP)
    b = reference_gru_rollout(pb, close, feat, start=10, steps=STEPS - 10, ep_len=EP, origin=0, h0=a["h"],
                              position=a["position"], entry=a["entry"])
    assert SR.same(tr["actions"][:, :10], a["actions"]) and SR.same(tr["q"][:, :10], a["q"])
    assert torch.allclose(tr["q"][:, 10:], b["q"], rtol=1e-5, atol=1e-6)
    assert float((tr["actions"][:, 10:] == b["actions"]).float().mean()) > 0.98


def test_batcher_keeps_a_sessions_bars_in_order():
    from sharetrade.serve.gru_serve import GruBatcher

    close, feat = R.bars(E, STEPS + 8)
    base_srv = _server()
    base_slots = base_srv.open(4)
    base = SR.serve_lockstep(base_srv, base_slots, close[:4], feat[:4], 0, 6)
    srv = _server()
    slots = srv.open(4)
    with GruBatcher(srv, max_batch=8, max_delay_us=20000.0) as bat:
        # one client sends all its bars back to back, the others one at a time
        futs = {e: [] for e in range(4)}
        for t in range(6):
            futs[0].append(bat.submit(slots[0], feat[0, t].float(), float(close[0, t])))
        for t in range(6):
            for e in (1, 2, 3):
                futs[e].append(bat.submit(slots[e], feat[e, t].float(), float(close[e, t])))
        got = {e: [f.result(timeout=60) for f in fs] for e, fs in futs.items()}
        with pytest.raises(ValueError):
            bat.submit(63, feat[0, 0].float(), 1.0)
    for e in range(4):
        assert [g[0] for g in got[e]] == base["actions"][e].tolist()
        assert [g[1] for g in got[e]] == base["pos"][e].tolist()
        assert SR.same(torch.tensor([g[2] for g in got[e]]), base["reward"][e])
    assert max(bat.batch_sizes) <= 4 and sum(bat.batch_sizes) == 24 and len(bat.batch_sizes) >= 6


def test_http_session_routes():
    from fastapi.testclient import TestClient

    from sharetrade.serve.gru_serve import GruBatcher
    from sharetrade.serve.http import make_gru_app

    close, feat = R.bars(E, STEPS + 8)
    base_srv = _server()
    base = SR.serve_lockstep(base_srv, base_srv.open(1), close[:1], feat[:1], 0, 7)
    srv = _server()
    with GruBatcher(srv, max_batch=8, max_delay_us=100.0) as bat:
        cl = TestClient(make_gru_app(srv, bat))
        sid = cl.post("/session").json()["session"]
        names = []
        for t in range(7):
            r = cl.post(f"/session/{sid}/bar", json={"features": feat[0, t].float().tolist(),
                                                      "close": float(close[0, t])})
            assert r.status_code == 200, r.text
            j = r.json()
            assert j["index"] == int(base["actions"][0, t]) and j["position"] == int(base["pos"][0, t])
            assert j["reward"] == pytest.approx(float(base["reward"][0, t]), abs=0, rel=1e-7)
            names.append(j["action"])
        assert set(names) <= {"Buy", "Sell", "Hold"}
        st = cl.get(f"/session/{sid}").json()
        assert st["bars"] == 7 and st["elapsed"] == 7 % EP and "h" not in st
        assert st["ret"] == pytest.approx(float(base_srv.state([0])["ret"][0]), rel=1e-7)
        assert cl.post(f"/session/{sid}/bar", json={"features": [0.0] * 7, "close": 1.0}).status_code == 400
        assert cl.get("/health").json()["bars"] == 7
        assert "sharetrade_gru_bars_total 7.0" in cl.get("/metrics").text
        assert cl.delete(f"/session/{sid}").status_code == 200
        assert cl.get(f"/session/{sid}").status_code == 404
        assert cl.post(f"/session/{sid}/bar", json={"features": [0.0] * 8, "close": 1.0}).status_code == 404


def test_cli_serves_a_recurrent_checkpoint_through_sessions(tmp_path, monkeypatch):
    import uvicorn
    from fastapi.testclient import TestClient

    from sharetrade import __main__ as M
    from sharetrade.persist import checkpoint as ck

    params = R.centred_params(3, E, STEPS, EP)
    flat = torch.cat([params[n].reshape(-1) for n in ("w_ih", "w_hh", "b_ih", "b_hh", "w_q", "b_q")])
    ck.save(str(tmp_path / "run.stck"), {"flat": flat}, {"kind": "recurrent", "config": {"agent": {"seed": 3}}})
    assert M._gru_path(argparse.Namespace(policy="auto", ckpt=str(tmp_path / "run.stck")))
    seen = {}

    def fake_run(app, **kw):
        cl = TestClient(app)
        sid = cl.post("/session").json()["session"]
        close, feat = R.bars(E, STEPS + 8)
        seen["bar"] = cl.post(f"/session/{sid}/bar", json={"features": feat[0, 0].float().tolist(),
                                                            "close": float(close[0, 0])}).json()
        seen["health"] = cl.get("/health").json()

    monkeypatch.setattr(uvicorn, "run", fake_run)
    assert M.main(["serve", "--ckpt", str(tmp_path / "run.stck"), "--device", "cpu", "--max-sessions", "4",
                   "--ep-len", str(EP)]) == 0
    assert seen["health"]["policy"] == "gru" and seen["health"]["max_sessions"] == 4
    assert seen["bar"]["action"] in ("Buy", "Sell", "Hold") and seen["bar"]["reward"] == 0.0
    base_srv = _server()
    base = SR.serve_lockstep(base_srv, base_srv.open(1), *(x[:1] for x in R.bars(E, STEPS + 8)), 0, 1)
    assert seen["bar"]["index"] == int(base["actions"][0, 0])
