"""The float64 step model of tests/step_refs.py against the torch oracle, and against itself with one mutation at a
time (no GPU).

1. On every exact case the model equals ``engine_step_ref(..., emulate_bf16=True)`` bit for bit in fp32: gradient,
   rewards, new state, actions, Q values and the TD target.  The oracle has no statistics row, no schedule, no slabs
   and no tick bank: those parts of the model are pinned by the mutation table below and by the kernels
   (tests/test_gpu_step_exact.py).
2. Every mutation of ``step_refs.MUTATIONS`` is caught by the same ``check_step`` the GPU file uses, on the case
   named beside it.  The counts are recorded in profiles/step_refs.md."""
import numpy as np
import pytest
import torch

import step_refs as sr
from sharetrade.env import trading as tr

CPU_CASES = [("base", 256, False), ("base", 256, True), ("edges", 256, False), ("edges", 128, True),
             ("rounding", 128, False), ("rounding", 96, False), ("rounding", 192, False), ("t01", 128, False),
             ("t12", 128, False), ("t012", 128, False), ("t01", 128, True), ("t12", 128, True), ("t012", 128, True),
             ("rel", 256, False), ("raw", 256, False),
             ("growth", 128, False), ("clip", 256, False), ("knobs05", 128, False), ("knobs2", 256, False),
             ("knobs-t01", 128, False), ("base", 1024, False)]


def oracle(c, forced=None):
    k = c.knobs
    st = tr.EnvState(**{kk: torch.from_numpy(c.state[kk].copy()) for kk in sr.STATE_KEYS})
    E = c.E
    return tr.engine_step_ref(
        torch.from_numpy(c.prices), st, torch.from_numpy(c.params.copy()), sr.LAYOUT, history=sr.H,
        feature_mode=k["feature_mode"], budget0=k["budget0"], shares0=k["shares0"], compat_env=k["compat"],
        target_slot="compat" if k["compat"] else "action", gamma=k["gamma"], output_relu=k["output_relu"],
        epsilon=k["epsilon"], ramp=k["ramp"], seed=k["seed"], rank=0, step=k["step"], loss_coef=k["loss_coef"],
        env_offset=k["env_offset"], emulate_bf16=True, forced_actions=forced, reward_mode=k["reward_mode"],
        td_clip=k["td_clip"], target_params=None if c.target is None else torch.from_numpy(c.target.copy()),
        double_dqn=k["double_dqn"], reward_scale=k["reward_scale"],
        ramp_pos=torch.full((E,), k["step"], dtype=torch.int32) if k["ramp_global"] else None)


@pytest.mark.parametrize("kind,E,compat", CPU_CASES)
def test_model_equals_torch_oracle_bit_for_bit(kind, E, compat):
    c = sr.exact_case(kind, E, compat)
    print(f"[case] {c.name} bits {({k: round(v, 1) for k, v in c.notes['bits'].items()})} "
          f"rounded/ties {c.notes['counts']} q_ties {c.notes['q_ties']} cover {c.notes.get('cover')}")
    for bank in ("fp32", "ticks") if c.knobs["feature_mode"] == "relative" else ("fp32",):   # (ticks: relative only)
        res = sr.step_model(c, bank=bank)
        ns, grad, info = oracle(c)
        n = {"actions": sr.check_int(info["actions"].numpy(), res["actions"]),
             "reward": sr.check_f32(info["reward"].numpy(), res["reward"]),
             "q": sr.check_f32(info["q"].numpy(), res["q"]),
             "q_next": sr.check_f32(info["q_next"].numpy(), res["q_next"]),
             "target": sr.check_f32(info["target"].numpy(), res["target"]),
             "grad": sr.check_f32(grad.numpy(), sr.grad_of(res, np.arange(E)))}
        for kk in sr.STATE_KEYS:
            ref = res["state"][kk]
            got = getattr(ns, kk).numpy()
            n["state." + kk] = sr.check_int(got, ref) if ref.dtype == np.int32 else sr.check_f32(got, ref)
        assert sr.total(n) == 0, (bank, n)
        # the loss the oracle reports (float64 here, fp32 there: the one statistic it has) agrees
        assert float(info["loss"]) == float(np.float32(res["terms"][:, 1].sum()))
    if c.pinned is not None:
        ex = res["exploit"]
        assert np.array_equal(info["actions"].numpy()[ex], c.pinned[ex])


def test_schedule_slabs_and_reduce_are_consistent():
    """The per-workgroup partials add up to the whole gradient for every (chunk, grid); both slab formats reduce to
    it exactly on an exact case; the bf16 layout is [P/32][grid][32]."""
    c = sr.exact_case("base", 256)
    res = sr.step_model(c)
    whole = sr.grad_of(res, np.arange(c.E))
    for chunk, grid in ((64, 1), (64, 3), (64, 4), (32, 5), (32, 8)):
        part = sr.partials(c, res, chunk, grid)
        assert np.array_equal(part.sum(0), whole)
        own = sr.owner(c.E, chunk, grid)
        assert np.array_equal(own[::chunk], np.arange(c.E // chunk) % grid)
        f = sr.slab_model(part, False)
        assert np.array_equal(sr.reduce_model(f, False), whole)
        b = sr.slab_model(part, True)
        assert b.shape == (sr.LAYOUT.numel // 32, grid, 32)
        i = sr.LAYOUT.segments["W1"].offset + 77
        assert np.array_equal(sr.bf16_val(b[i >> 5, :, i & 31]), sr.bf16_round64(part[:, i]))
        st = sr.stats_model(c, res, chunk, grid)
        assert np.array_equal(st.sum(0), res["terms"].sum(0))


def test_precondition_rejects_an_inexact_case():
    """A case whose sums need 24 bits or more is a bug in the case: the builder raises."""
    with pytest.raises(AssertionError, match="not exact in fp32"):
        sr.make_case("dense", 256, 1, pvals=dict(w2_density=1.0, w1_density=0.5, bias_step=0.125))


# mutation -> (case kind, E, compat, chunk, grid, bf16 slabs)
MUTANT_CASE = {
    "win_first_late": ("base", 256, False, 64, 2, True), "win_last_late": ("base", 256, False, 64, 2, True),
    "win_last_dropped": ("raw", 256, False, 64, 2, True), "xn_tail_old": ("base", 256, False, 64, 2, True),
    "shares_next_price": ("base", 256, False, 64, 2, True), "no_bias_col": ("base", 256, False, 64, 2, True),
    "tie_last": ("t01", 128, False, 64, 1, False), "next_tie_last": ("t01", 128, True, 64, 1, False),
    "next_first": ("base", 256, False, 64, 2, False), "u2_explore": ("base", 256, False, 64, 2, False),
    "thr_no_min": ("base", 256, False, 64, 2, False), "no_env_offset": ("edges", 256, False, 64, 2, False),
    "gamma_on_reward": ("base", 256, False, 64, 2, False), "scale_stored_reward": ("knobs2", 256, False, 64, 2, False),
    "clip_after_coef": ("clip", 256, False, 64, 2, False), "dq_unrounded": ("rounding", 128, False, 64, 2, False),
    "relu_mask_ge": ("base", 256, False, 64, 2, False), "no_out_relu_mask": ("base", 256, True, 64, 2, False),
    "db_tile_dropped": ("base", 256, False, 64, 2, True), "slab_trunc": ("rounding", 128, False, 64, 2, True),
    "slab_row_next": ("base", 256, False, 64, 3, True), "slab_block_shift4": ("base", 256, False, 64, 2, True),
    "no_reset": ("edges", 256, False, 64, 2, False), "loss_from_clipped": ("clip", 256, False, 64, 2, False),
}
STEP_SIDE = set(sr.MUTATIONS) - {"db_tile_dropped", "slab_trunc", "slab_row_next", "slab_block_shift4", "no_bias_col"}


def mutant_diffs(mut):
    kind, E, compat, chunk, grid, bf16 = MUTANT_CASE[mut]
    c = sr.exact_case(kind, E, compat)
    ref = sr.step_model(c)
    bad = sr.step_model(c, mut=mut) if mut in STEP_SIDE else ref
    got = sr.model_outputs(c, bad, chunk, grid, bf16, mut=mut)
    return c, sr.check_step(got, c, ref, chunk, grid, bf16)


def test_unmutated_model_has_no_differences():
    for mut in ("win_first_late", "slab_row_next", "tie_last", "no_reset"):
        kind, E, compat, chunk, grid, bf16 = MUTANT_CASE[mut]
        c = sr.exact_case(kind, E, compat)
        ref = sr.step_model(c)
        assert sr.total(sr.check_step(sr.model_outputs(c, ref, chunk, grid, bf16), c, ref, chunk, grid, bf16)) == 0


@pytest.mark.parametrize("mut", sr.MUTATIONS)
def test_every_mutation_is_caught(mut):
    assert set(MUTANT_CASE) == set(sr.MUTATIONS)
    c, d = mutant_diffs(mut)
    print(f"[mutant] {mut} on {c.name}: " + " ".join(f"{k}={v[0]}" for k, v in d.items() if v[0]))
    assert sr.total(d) > 0, mut


def test_last_window_column_is_dead_under_relative_features():
    """An equivalent mutant: with relative features the window's last column is last / last - 1 = 0 on every env, so
    dropping it changes nothing, bit for bit.  (Only the raw-feature case can see that column; "win_last_late" pins its
    read address on the relative cases.)"""
    for kind in ("base", "edges"):
        c = sr.exact_case(kind, 256)
        ref, bad = sr.step_model(c), sr.step_model(c, mut="win_last_dropped")
        assert not ref["x"][:, sr.H - 1].any() and not ref["x_next"][:, sr.H - 1].any()
        got = sr.model_outputs(c, bad, 64, 2, True)
        assert sr.total(sr.check_step(got, c, ref, 64, 2, True)) == 0


def test_tie_mutants_show_in_the_pinned_action():
    """The tie cases pin the action itself: with the last index winning, every exploiting env differs."""
    c = sr.exact_case("t01", 128)
    bad = sr.step_model(c, mut="tie_last")
    ex = bad["exploit"]
    assert ex.sum() > 100 and np.all(bad["actions"][ex] != c.pinned[ex])
    c = sr.exact_case("knobs-t01", 128)
    ref, bad = sr.step_model(c), sr.step_model(c, mut="next_tie_last")
    assert np.count_nonzero(ref["target"] != bad["target"]) > 100   # the double-DQN action values another target row


@pytest.mark.parametrize("E", [96, 256, 1024])
def test_random_case_bounds_come_from_the_reference_and_catch_mutants(E):
    """The bounded case of tests/test_gpu_step_exact.py on the reference alone: the share of envs whose action is
    left open (two largest float64 Q within the counted forward bound) stays under the 2 % cap for the seed the GPU
    file uses, and a late or missing column exceeds the per-slice bounds by a wide margin."""
    c = sr.random_case(E, 3)
    rb = sr.random_bounds(c)
    unc = sr.uncertain_envs(rb)
    bound = sr.slice_bounds(c, rb)
    rel = bound / np.maximum(sr.slice_norms(rb["grad"]), 1e-300)
    share = np.median(4 * rb["floor"][bound > 0] / bound[bound > 0])
    print(f"[random] E={E}: uncertain envs {int(unc.sum())} ({unc.mean():.4f}); bound / slice norm median "
          f"{np.median(rel):.4f}; floor share of the bound median {share:.3f}")
    assert unc.mean() <= 0.02
    assert sr.check_random(rb["grad"], rb, bound)[0] == 0
    whole = np.arange(E)
    for mut in ("win_first_late", "win_last_late", "no_bias_col", "xn_tail_old", "relu_mask_ge"):
        bad = sr.step_model(c, mut=mut, forced=rb["ref"]["actions"])
        nbad, worst = sr.check_random(sr.grad_of(bad, whole, mut), rb, bound)
        print(f"[random] E={E} mutant {mut}: slices over the bound {nbad}, "
              f"largest err / bound {max(worst.values()):.1f}")
        assert nbad > 0, (mut, worst)
