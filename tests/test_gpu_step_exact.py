"""The fused bf16 step kernels (csrc/qstep_ws.hip, csrc/qstep_wide.hip, csrc/qstep_fused.hip) and the target pass
(csrc/qtarget.hip) against the float64 step model of tests/step_refs.py, bit for bit.

On the exact cases every sum the kernels form needs fewer than 24 bits (checked per case by the builder), so the
summation order, the MFMA internals, the k permutation and the tile grouping cannot show.  Per launch: actions with
zero mismatches, rewards and every state field, every per-workgroup slab row in its layout (fp32 [grid][P], or bf16
[P/32][grid][32] with one round-to-nearest-even per element), the reduced gradient and the statistics row
(``loss_sum`` and ``qslot_sum`` included) equal the model's bit patterns.  Slabs are compared on the parameters
(``step_refs.real_mask``: their pad entries are unspecified, the slab pass masks them), the reduced gradient on every
entry, pads included (exactly 0).

tests/test_step_refs.py ties the model to the torch oracle and shows that the same ``check_step`` catches every
mutation of the model; profiles/step_refs.md has the case table and the results."""
import time

import numpy as np
import pytest
import torch

import step_refs as sr
from guard_band import Band, bits
from test_gpu_qstep_ws import KERNELS, _cfg

pytestmark = pytest.mark.gpu

_RES = {}


def model(c, bank):
    key = (c.name, bank)
    if key not in _RES:
        _RES[key] = sr.step_model(c, bank=bank)
    return _RES[key]


def engine(c, kernel, grid, slab, bank16="auto", waves=8, sched="static"):
    """A VectorEngine set up for case ``c``: its knobs, parameters, state, step index; the slabs, the gradient and
    the QT buffer moved into guard-banded allocations this test owns."""
    from sharetrade.trainer.engine import VectorEngine

    k = c.knobs
    cfg = _cfg(k["compat"], kernel)
    a, e = cfg.agent, cfg.engine
    a.epsilon, a.ramp, a.gamma, a.seed = k["epsilon"], k["ramp"], k["gamma"], k["seed"]
    a.reward_mode, a.td_clip = k["reward_mode"], k["td_clip"]
    cfg.env.budget, cfg.env.shares, cfg.env.features = k["budget0"], k["shares0"], k["feature_mode"]
    if c.target is not None:
        a.target_every, a.double_dqn, a.reward_scale = 1000, k["double_dqn"], k["reward_scale"]
        a.ramp_mode = "global" if k["ramp_global"] else "position"
    e.grid, e.slab_dtype, e.bank16, e.step_waves, e.chunk_schedule = grid, slab, bank16, waves, sched
    dev = torch.device("cuda", 0)
    eng = VectorEngine(cfg, prices=torch.from_numpy(c.prices), device=dev, envs=c.E)
    assert eng.step_kernel == kernel and eng.grid == grid and eng.chunk_schedule == sched
    assert eng.slab_bf16 == (slab == "bf16" and kernel != "narrow")
    eng.loss_coef, eng.env_offset = k["loss_coef"], k["env_offset"]
    bands = {"slab": Band(eng.slab.numel(), eng.slab.dtype, -7.0, dev).set(0),
             "stat_slab": Band(eng.stat_slab.numel(), torch.float32, -7.0, dev).set(0),
             "grad": Band(eng.grad.numel(), torch.float32, -7.0, dev).set(0)}
    eng.slab = bands["slab"].v.view(eng.slab.shape)
    eng.stat_slab = bands["stat_slab"].v.view(eng.stat_slab.shape)
    eng.grad = bands["grad"].v
    if eng.qt_buf is not None:
        bands["qt"] = Band(eng.qt_buf.numel(), torch.float32, -7.0, dev).set(0)
        eng.qt_buf = bands["qt"].v
    eng._build_structs()
    eng.set_params(torch.from_numpy(c.params))
    if c.target is not None:
        eng.params_target.copy_(torch.from_numpy(c.target))
    for kk in sr.STATE_KEYS:
        getattr(eng.state, kk).copy_(torch.from_numpy(c.state[kk]))
    eng.ctrl.fill_(k["step"])
    return eng, bands


def read_only(eng):
    ro = {"params": eng.params, "params_bf": eng.params_bf, "prices": eng.prices, "mask": eng.mask,
          "ctrl0": eng.ctrl[:1]}
    for name in ("_wimg", "prices4", "ticks", "tscale", "params_target"):
        t = getattr(eng, name, None)
        if t is not None:
            ro[name] = t
    return ro


def launch(c, kernel, grid, slab, **kw):
    """One native_grad() launch -> (eng, got, bank): everything the launch left behind, on the host."""
    eng, bands = engine(c, kernel, grid, slab, **kw)
    before = {n: bits(t.contiguous()).clone() for n, t in read_only(eng).items()}
    eng.native_grad()
    torch.cuda.synchronize()
    assert int(eng.kernel_err.sum()) == 0, "ring wait gave up"
    for n, t in read_only(eng).items():
        assert torch.equal(bits(t.contiguous()), before[n]), f"the launch changed {n}, which it only reads"
    for n, b in bands.items():
        assert b.guards_intact(), f"bytes around {n} changed"
    P = sr.LAYOUT.numel
    if eng.slab_bf16:
        slab_h = eng.slab.view(torch.int16)[:P * grid].cpu().numpy().view(np.uint16).reshape(P // 32, grid, 32)
        assert not eng.slab.view(torch.int16)[P * grid:].any(), "slab tail written"
    else:
        slab_h = eng.slab.cpu().numpy()
    got = dict(actions=eng.actions_out.cpu().numpy(), reward=eng.rewards_out.cpu().numpy(),
               state={kk: getattr(eng.state, kk).cpu().numpy() for kk in sr.STATE_KEYS},
               slab=slab_h, grad=eng.grad.cpu().numpy().copy(), stats=eng.stat_slab.cpu().numpy())
    return eng, got, ("ticks" if eng.ticks is not None else "fp32")


def assert_exact_launch(c, kernel, grid, slab, chunk, **kw):
    eng, got, bank = launch(c, kernel, grid, slab, **kw)
    res = model(c, bank)
    d = sr.check_step(got, c, res, chunk, grid, eng.slab_bf16, mask=sr.real_mask())
    tag = f"{kernel} {c.name} grid={grid} slab={slab} bank={bank} {kw}"
    print(f"[exact] {tag}: differing " + " ".join(f"{n}={v[0]}" for n, v in d.items()))
    assert sr.total(d) == 0, (tag, {n: v for n, v in d.items() if v[0]})
    if c.pinned is not None:
        ex = res["exploit"]
        assert np.array_equal(got["actions"][ex], c.pinned[ex]), tag
    return eng, got


# (kind, E, grid, compat): E = 64 one chunk; 128 on one workgroup: the 4-slot ring wraps, paired slots; 192: an odd
# slot count for the pair logic; 640 / 2 and 1024 / 3: uneven rounds
WS_CASES = [("edges", 64, 1, False), ("edges", 64, 1, True), ("rounding", 128, 1, False), ("t01", 128, 1, False),
            ("t12", 128, 1, False), ("t012", 128, 1, False), ("t01", 128, 1, True), ("t12", 128, 1, True),
            ("t012", 128, 1, True), ("growth", 128, 1, False), ("raw", 128, 1, False), ("rounding", 192, 1, False),
            ("edges", 192, 1, True), ("clip", 192, 1, False), ("base", 640, 2, False), ("base", 640, 2, True),
            ("rel", 640, 2, False), ("t01", 640, 2, False), ("raw", 640, 2, False), ("base", 1024, 3, False),
            ("edges", 1024, 3, False), ("edges", 1024, 3, True)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind,E,grid,compat", WS_CASES)
def test_ws_exact(native_built, kernel, kind, E, grid, compat):
    """The ws kernel on every exact case, with the tick bank and the fp32 bank, fp32 and bf16 slabs."""
    c = sr.exact_case(kind, E, compat)
    t0 = time.time()
    for bank16 in ("auto", "off"):
        for slab in ("fp32", "bf16"):
            eng, _ = assert_exact_launch(c, kernel, grid, slab, 64, bank16=bank16)
            assert (eng.ticks is not None) == (bank16 == "auto" and c.knobs["feature_mode"] == "relative")
    print(f"[time] ws {c.name}: {time.time() - t0:.2f} s for 4 launches")


@pytest.mark.parametrize("wimg", ["1", "0"])
def test_ws_exact_with_and_without_weight_image(native_built, monkeypatch, wimg):
    """SHARETRADE_WS_WIMG = 1 (the prologue copies the weight image) and 0 (it gathers from wq / wf)."""
    monkeypatch.setenv("SHARETRADE_WS_WIMG", wimg)
    for kind, E, grid in (("rounding", 192, 1), ("base", 640, 2)):
        eng, _ = assert_exact_launch(sr.exact_case(kind, E), "ws", grid, "bf16", 64)
        assert (eng._wimg is not None) == (wimg == "1")


WIDE_CASES = [("edges", 64, 1, False), ("edges", 64, 1, True), ("rounding", 192, 2, False), ("t01", 192, 2, False),
              ("t12", 192, 2, True), ("t012", 192, 2, True), ("raw", 192, 2, False), ("clip", 192, 2, False),
              ("base", 512, 3, False), ("base", 512, 3, True), ("rel", 512, 3, False), ("edges", 512, 3, False)]


@pytest.mark.parametrize("kind,E,grid,compat", WIDE_CASES)
def test_wide_exact(native_built, kind, E, grid, compat):
    """The 64-env-chunk kernel with 4 and 8 waves, fp32 and bf16 slabs."""
    c = sr.exact_case(kind, E, compat)
    for waves in (4, 8):
        for slab in ("fp32", "bf16"):
            assert_exact_launch(c, "wide", grid, slab, 64, waves=waves)


FUSED_CASES = [("edges", 32, 1, False), ("edges", 96, 2, True), ("rounding", 96, 2, False), ("t01", 96, 2, False),
               ("t12", 96, 2, True), ("t012", 96, 2, False), ("raw", 96, 2, False), ("growth", 96, 2, False),
               ("clip", 96, 3, False), ("base", 96, 3, True)]


@pytest.mark.parametrize("kind,E,grid,compat", FUSED_CASES)
def test_fused_exact(native_built, kind, E, grid, compat):
    """The 32-env-chunk kernel (fp32 slabs only)."""
    assert_exact_launch(sr.exact_case(kind, E, compat), "narrow", grid, "fp32", 32)


@pytest.mark.parametrize("kind,E,grid", [("knobs05", 128, 1), ("knobs-t01", 128, 1), ("knobs2", 640, 2),
                                         ("knobs05", 640, 2)])
@pytest.mark.parametrize("bank16", ["auto", "off"])
def test_ws_knob_build_and_target_pass_exact(native_built, kind, E, grid, bank16):
    """Target net, double DQN, reward_scale 0.5 / 2 and the global ramp: the QT buffer equals the float64 target
    forward of all three candidate next states (column 3 zero), then the step is exact."""
    c = sr.exact_case(kind, E)
    for slab in ("fp32", "bf16"):
        eng, got = assert_exact_launch(c, "ws", grid, slab, 64, bank16=bank16)
        bank = "ticks" if eng.ticks is not None else "fp32"
        n, where = sr.check_f32(eng.qt_buf.cpu().numpy().reshape(E, 3, 4), sr.qt_model(c, bank))
        print(f"[exact] qtarget {c.name} bank={bank}: differing {n}")
        assert n == 0, where
        assert not eng.qt_buf.view(E, 3, 4)[:, :, 3].any()


@pytest.mark.parametrize("kernel", ["ws", "wide"])
def test_dynamic_schedule_exact(native_built, kernel):
    """The dynamic chunk schedule: actions, state and the statistics total equal the model; with fp32 slabs the reduced
    gradient does too (exact sums do not depend on which workgroup took a chunk).  bf16 slabs under the dynamic
    schedule are compared by tests/test_gpu_qstep_ws.py only."""
    E, grid = 1024, 8
    c = sr.exact_case("edges", E)
    eng, got, bank = launch(c, kernel, grid, "fp32", sched="dynamic")
    res = model(c, bank)
    whole = sr.grad_of(res, np.arange(E))
    d = {"actions": sr.check_int(got["actions"], res["actions"]), "reward": sr.check_f32(got["reward"], res["reward"]),
         "grad": sr.check_f32(got["grad"], whole),
         "stats": sr.check_f32(got["stats"].astype(np.float64).sum(0), res["terms"].sum(0))}
    for kk in sr.STATE_KEYS:
        ref = res["state"][kk]
        d["state." + kk] = sr.check_int(got["state"][kk], ref) if ref.dtype == np.int32 else \
            sr.check_f32(got["state"][kk], ref)
    print(f"[exact] dynamic {kernel}: differing " + " ".join(f"{n}={v[0]}" for n, v in d.items()))
    assert sr.total(d) == 0, d
    if eng.chunk_heads is not None:
        assert int(eng.chunk_heads.abs().sum()) == 0, "claim heads not re-zeroed"


# ----------------------------------------------------------------------------- the bounded random case
RANDOM_SEED = 3
_RB = {}


def random_ref(E):
    if E not in _RB:
        c = sr.random_case(E, RANDOM_SEED)
        _RB[E] = (c, sr.random_bounds(c))
    return _RB[E]


@pytest.mark.parametrize("kernel,E,grid,slab", [("ws", 256, 3, "bf16"), ("ws", 256, 3, "fp32"), ("ws", 1024, 3, "bf16"),
                                                ("ws", 1024, 3, "fp32"), ("wide", 256, 3, "bf16"),
                                                ("wide", 256, 3, "fp32"), ("narrow", 96, 2, "fp32")])
def test_random_case_within_reference_bounds(native_built, kernel, E, grid, slab):
    """Realistic magnitudes (random-walk bank, default init): each row and column of every weight gradient and each
    bias group within 4 x the reference's own flip-noise floor + the counted fp32 accumulation term (bf16 slabs: + one
    rounding per partial).  Actions may differ from the float64 reference only on envs whose two largest Q lie within
    the counted forward bound of each other (at most 2 % of the envs, checked on the reference in
    tests/test_step_refs.py); rewards and state are then bit-equal for the kernel's actions."""
    c, rb0 = random_ref(E)
    chunk = 32 if kernel == "narrow" else 64
    eng, got, bank = launch(c, kernel, grid, slab)
    unc = sr.uncertain_envs(rb0)
    mism = got["actions"] != rb0["ref"]["actions"]
    print(f"[random] {kernel} E={E} grid={grid} slab={slab} bank={bank}: action mismatches {int(mism.sum())} "
          f"(uncertain envs {int(unc.sum())} = {unc.mean():.4f})")
    assert unc.mean() <= 0.02
    assert not (mism & ~unc).any(), np.nonzero(mism & ~unc)[0][:8]
    rb = sr.random_bounds(c, actions=got["actions"]) if mism.any() else rb0
    d = {"reward": sr.check_f32(got["reward"], rb["ref"]["reward"])}
    for kk in sr.STATE_KEYS:
        ref = rb["ref"]["state"][kk]
        d["state." + kk] = sr.check_int(got["state"][kk], ref) if ref.dtype == np.int32 else \
            sr.check_f32(got["state"][kk], ref)
    assert sr.total(d) == 0, d
    nbad, worst = sr.check_random(got["grad"], rb, sr.slice_bounds(c, rb, chunk, grid, eng.slab_bf16))
    print(f"[random] {kernel} E={E} grid={grid} slab={slab}: largest err / bound per layer "
          + " ".join(f"{n}={v:.3f}" for n, v in worst.items()) + f"; slices over the bound {nbad}")
    assert nbad == 0, worst
