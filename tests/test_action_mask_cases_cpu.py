"""Action masks without a GPU: the numpy restatement of the set rule has the properties the contract states, the bars of the masked
loss and gradient kernels are 4 x the measured distance of a plain fp32 restatement from fp64 (printed here), every planted mistake
breaks a bar or an exact check on every case it applies to, the sampled-action check of the GPU test leaves out few enough pairs,
and the new entries are declared, exported, mirrored in ``_lib`` and refuse bad arguments before any device call."""
import ctypes as C

import numpy as np
import pytest

from jolineedle_amd import _lib
from jolineedle_amd.engine import make_jn_config
from tests import action_mask_cases as am
from tests import train_cases as tc
from tests.helpers import model_config

NEW_ENTRIES = {"jn_set_rollout_action_mask": 3, "jn_action_sets": 11, "jn_reinforce_loss_masked": 18, "jn_logits_grad_masked": 11}


# ---- the rule of the sets -----------------------------------------------------------------------------------------------------------
def _all_states():
    pos, vis, ext = am.states(am.CANVAS)
    return pos, vis, ext


@pytest.mark.parametrize("nA", [8, 9])
@pytest.mark.parametrize("policy", list(am.POLICIES))
def test_sets_are_never_empty_hold_stop_and_forced_and_fall_back_in_order(policy, nA):
    pos, vis, ext = _all_states()
    forced = am.forced_for(len(pos), nA)
    plain, with_forced = am.sets_of(policy, pos, vis, ext, nA), am.sets_of(policy, pos, vis, ext, nA, forced)
    for i, (y, x) in enumerate(pos.tolist()):
        gh, gw = ext[i].tolist()
        m = int(plain[i])
        assert 0 < m < (1 << nA)
        assert (m >> 8 & 1) == (1 if nA == 9 else 0)                                   # STOP: always with nine actions, never with eight
        assert int(with_forced[i]) == m | (1 << int(forced[i]))                        # the forced action, and nothing else, is added
        inside = [a for a in range(8) if 0 <= y + am.DY[a] < gh and 0 <= x + am.DX[a] < gw]
        fresh = [a for a in inside if not vis[i][y + am.DY[a]][x + am.DX[a]]]
        moves = [a for a in am.members(m, nA) if a < 8]
        if policy == "unvisited" and fresh:
            assert moves == fresh
        elif inside:
            assert moves == inside                                                     # grid, or nothing fresh: the inside moves
        else:
            assert (gh, gw) == (1, 1) and moves == list(range(8))                      # nowhere to go: every move
    # the three patterns do what their names say: "empty" leaves every inside move fresh, "full" and "ring" leave none
    n_fresh = [sum(1 for a in range(8) if 0 <= y + am.DY[a] < ext[i][0] and 0 <= x + am.DX[a] < ext[i][1] and not vis[i][y + am.DY[a]][x + am.DX[a]])
               for i, (y, x) in enumerate(pos.tolist())]
    assert all(n == 0 for n in n_fresh[1::3]) and all(n == 0 for n in n_fresh[2::3]) and any(n > 0 for n in n_fresh[0::3])
    assert len(pos) == 69 and (ext < np.array(am.CANVAS)).any(axis=1).sum() == 69 - 36


def test_a_corner_of_the_headline_grid_keeps_three_moves_and_an_edge_five():
    v = np.zeros((10, 10), dtype=np.uint8)
    assert am.members(am.action_set("grid", 0, 0, 10, 10, v, 8), 8) == [1, 3, 7]         # RIGHT, DOWN, RIGHT_DOWN
    assert len(am.members(am.action_set("grid", 0, 4, 10, 10, v, 8), 8)) == 5
    assert len(am.members(am.action_set("grid", 4, 4, 10, 10, v, 9), 9)) == 9
    v[1, 1] = 1
    assert am.members(am.action_set("unvisited", 0, 0, 10, 10, v, 9), 9) == [1, 3, 8]


@pytest.mark.parametrize("policy", list(am.POLICIES))
def test_the_set_mistakes_change_a_set_on_every_case_they_apply_to(policy):
    """STOP dropped: every case with nine actions.  Fallback skipped: every "unvisited" case (the sets of the visited borders)."""
    pos, vis, ext = _all_states()
    for nA in (8, 9):
        for forced in (None, am.forced_for(len(pos), nA)):
            good = am.sets_of(policy, pos, vis, ext, nA, forced)
            if nA == 9:
                assert (am.sets_of(policy, pos, vis, ext, nA, forced, "no_stop") != good).any()
            if policy == "unvisited":
                assert (am.sets_of(policy, pos, vis, ext, nA, forced, "no_fallback") != good).any()


# ---- the bars mean something --------------------------------------------------------------------------------------------------------
def test_fp32_restatements_stay_within_every_bar_and_the_bars_are_four_times_their_distance():
    worst, at = {}, {}
    for c in am.LOSS_CASES:
        ref, got = am.reference(c), am.compute(c)
        assert not am.over_bars(c, got, ref), (c, am.over_bars(c, got, ref))
        w = worst.setdefault((c.kind, c.big), {})
        for k, v in am.distances(c, got, ref).items():
            if v > w.get(k, -1.0):
                w[k], at[c.kind, c.big, k] = v, am.case_id(c)
    for kind in ("rf", "lg"):
        for big, measured, bar in ((0, am.FP32_MEASURED[kind], am.BAR[kind]), (1, am.BIG_FP32_MEASURED[kind], am.BIG_BAR[kind])):
            print(f"fp32 restatement, {kind}{', logits x 30' if big else ''}: " +
                  ", ".join(f"{k} {worst[kind, big][k]:.2e} ({at[kind, big, k]})" for k in measured))
            for k in measured:
                assert 0.8 * measured[k] <= worst[kind, big][k] <= measured[k], (kind, big, k, worst[kind, big][k])
                assert bar[k] == pytest.approx(tc.bar_of(measured[k]), rel=1e-9), (kind, big, k)


@pytest.mark.parametrize("mutant", am.MUTANTS)
def test_every_mistake_in_the_masked_softmax_misses_a_bar_on_every_case(mutant):
    for c in am.LOSS_CASES:
        assert am.over_bars(c, am.compute(c, mutant), am.reference(c)), (mutant, c)


def test_cases_hold_one_element_sets_outside_logits_and_actions_inside_their_sets():
    assert {(c.B, c.T) for c in am.LOSS_CASES} == {(3, 5), (65, 7)} and {c.nA for c in am.LOSS_CASES} == {8, 9}
    assert {c.stop for c in am.LOSS_CASES} == {0, 1} and {c.big for c in am.LOSS_CASES} == {0, 1}
    for c in am.LOSS_CASES:
        d = am.inputs(c)
        n_bits = d["bits"].sum(axis=-1)
        assert n_bits.min() == 1 and n_bits.flat[0] == c.nA and (n_bits < c.nA).any()
        assert (d["logits"].numpy()[~d["bits"]] == np.float32(am.OUTSIDE)).all() and np.abs(d["logits"].numpy()[d["bits"]]).max() < 1e3
        assert np.take_along_axis(d["bits"], d["actions"].numpy()[..., None], axis=-1).all()
        assert (am.in_set(d["sets"], c.nA) == d["bits"]).all()
        assert d["S"] == (c.T - 2 if c.stop else c.T)
        ref = am.reference(c)
        assert (ref["dlogits"].numpy()[~d["bits"]] == 0).all() and np.isfinite(ref["dlogits"].numpy()).all()
        # a one-element set: log-prob 0, entropy 0, no gradient
        single = n_bits == 1
        logp, _, H = am.parts64(d["logits"].numpy(), d["sets"])
        assert (H[single] == 0).all() and (np.take_along_axis(logp, d["actions"].numpy()[..., None], axis=-1)[..., 0][single] == 0).all()
        assert (ref["dlogits"].numpy()[single] == 0).all()


def test_full_sets_give_the_unmasked_reference():
    """With every bit set the fp64 parts are log_softmax and its entropy."""
    import torch
    lg = torch.randn((4, 3, 9), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    logp, p, H = am.parts64(lg.numpy(), np.full((4, 3), 0x1FF, dtype=np.uint16))
    want = torch.log_softmax(lg, dim=-1)
    assert np.allclose(logp, want.numpy(), rtol=0, atol=1e-14) and np.allclose(H, -(want.exp() * want).sum(-1).numpy(), rtol=0, atol=1e-14)


def test_the_inverse_cdf_check_leaves_out_at_most_one_pair_in_a_hundred():
    """The GPU test leaves out the (agent, step) pairs whose uniform lies within 1e-5 of a boundary of the fp64 masked CDF.  On the
    uniforms of its own seeds and random logits and sets of its shapes, the share left out stays under its cap of 1 in 100."""
    rng = np.random.default_rng(11)
    out = total = 0
    for seed in SAMPLE_SEEDS:
        for b in range(65):
            for t in range(6):
                m = int(rng.integers(1, 1 << 9))
                _, gap = am.inverse_cdf64(rng.normal(size=9) * 3.0, m, am.sample_uniform(seed, b, t), 9)
                out += gap < CDF_MARGIN
                total += 1
    print(f"pairs within {CDF_MARGIN:g} of a CDF boundary: {out} of {total}")
    assert out * 100 <= total


SAMPLE_SEEDS = (1000004, 2000007, 3000010)      # the rollout seeds of the GPU test's sampled walks (trainer seeds 1, 2, 3, rollout 1)
CDF_MARGIN = 1e-5


def test_inverse_cdf_walks_the_members_in_index_order_and_ends_on_the_last():
    lg = np.zeros(9)
    assert am.inverse_cdf64(lg, 0b100100010, 0.0, 9)[0] == 1 and am.inverse_cdf64(lg, 0b100100010, 0.34, 9)[0] == 5
    assert am.inverse_cdf64(lg, 0b100100010, 0.99, 9)[0] == 8
    assert am.inverse_cdf64(lg, 0b000100010, 1.0, 9)[0] == 5                               # none passes: the last member
    assert am.greedy64(np.array([5.0, 1.0, 3.0, 3.0]), np.array(0b1110)) == 2               # the first maximum among the members


# ---- the entries ------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_mirrored():
    lib = _lib.load_library()
    assert lib.jn_abi_version() == 2 == _lib.ABI_VERSION                                   # added exports: the ABI stays
    header = (_lib.LIB_PATH.parents[2] / "include" / "jnroll.h").read_text()
    for name, n_args in NEW_ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert res is C.c_int and len(args) == n_args and fn.restype is C.c_int and list(fn.argtypes) == args
        assert f"int {name}(" in header
    assert "int jn_set_rollout_action_mask(jn_ctx* ctx, int policy, uint16_t* sets_out_dev);" in header
    assert "enum { JN_MASK_NONE = 0, JN_MASK_GRID = 1, JN_MASK_UNVISITED = 2 };" in header
    # the masked entries are the unmasked ones plus the sets
    assert _lib.SIGNATURES["jn_reinforce_loss_masked"][1][:-2] == _lib.SIGNATURES["jn_reinforce_loss"][1][:-1]
    assert _lib.SIGNATURES["jn_logits_grad_masked"][1][:-2] == _lib.SIGNATURES["jn_logits_grad"][1][:-1]


def test_setter_refuses_unknown_policies_on_a_context_made_without_a_gpu():
    lib = _lib.load_library()
    cfg = make_jn_config(model_config(patch_size=64, block_size=6, image_processor=None, with_detector=False), 0, 8, 9)
    h = C.c_void_p()
    assert lib.jn_create(C.byref(cfg), C.byref(h)) == 0, lib.jn_last_error()
    try:
        for policy in (1, 2, 0):
            assert lib.jn_set_rollout_action_mask(h, policy, None) == 0, lib.jn_last_error()
        for bad in (3, -1):
            assert lib.jn_set_rollout_action_mask(h, bad, None) == -1                      # JN_EINVAL
            err = lib.jn_last_error().decode()
            assert "jn_set_rollout_action_mask" in err and f"policy {bad}" in err, err
        assert lib.jn_set_rollout_action_mask(None, 1, None) == -1
    finally:
        lib.jn_destroy(h)


def test_context_free_entries_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load_library()
    p = C.c_void_p(16)      # never dereferenced: every call below is refused first
    assert lib.jn_action_sets(None, p, None, None, 4, 3, 4, 1, 9, p, None) == -1
    assert lib.jn_action_sets(p, p, None, None, 0, 3, 4, 1, 9, p, None) == -1
    for policy, nA in ((0, 9), (3, 9), (1, 7), (1, 10)):
        assert lib.jn_action_sets(p, p, None, None, 4, 3, 4, policy, nA, p, None) == -1
    assert lib.jn_reinforce_loss_masked(p, p, p, p, p, None, 2, 3, 9, 1, 0.0, 1.0, 0.01, 1.0, p, p, None, None) == -1      # no sets
    assert lib.jn_reinforce_loss_masked(p, p, p, p, p, None, 2, 3, 17, 1, 0.0, 1.0, 0.01, 1.0, p, p, p, None) == -1       # 17 actions
    assert lib.jn_logits_grad_masked(p, p, p, p, None, 2, 3, 9, p, None, None) == -1
    assert lib.jn_logits_grad_masked(p, p, p, p, None, 2, 3, 17, p, p, None) == -1


def test_python_keyword_is_checked_and_the_flag_parses():
    from jolineedle_amd.config import args_to_config, get_args
    from jolineedle_amd.rollouts import _mask_policy
    assert [_mask_policy(m) for m in (None, "grid", "unvisited")] == [0, 1, 2]
    with pytest.raises(ValueError, match="action_mask"):
        _mask_policy("border")
    assert args_to_config(get_args([]))[0].action_mask is None
    assert args_to_config(get_args(["--action-mask", "unvisited"]))[0].action_mask == "unvisited"
