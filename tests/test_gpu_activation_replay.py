"""Activation replay (``jn_set_activation_slots``): a train-mode rollout keeps a ring of activation
slots and the per-step BatchNorm state of every step; the backward re-runs the forward of each chunk of steps from the
kept statistics just before it differentiates it.  The replay reproduces a slot bit for bit, so the gradients are those
of the default (every step resident) up to the order of the atomics.

Shapes: gpt-nano + yolox-nano patch encoder, no detector, 64-px patches unless a test says otherwise.  Every test fails
on the parent commit, where the setter does not exist."""
import ctypes as C

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib
from jolineedle_amd._lib import JnError
from jolineedle_amd.views import ImageViews
from tests.helpers import make_pair, model_config, synth_batch
from tests.test_gpu_parity import _cfg, _check_grads, _oracle_reinforce_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 64
BASE = dict(patch_size=P, with_detector=False, image_processor=None)
# "equal to the order of the atomics" (test_headline_shape_backward_does_not_depend_on_the_step_batching)
LOSS_BAR, L2_BAR, MAX_BAR = 1e-5, 2e-5, 2e-4


def _twin(state, max_batch, **kw):
    """A fresh product model holding `state` (so that the runs of a comparison start from equal weights)."""
    product = ja.GPT(model_config(**kw), max_batch=max_batch)
    product.load_state_dict(state)
    return product


def _state(seed, **kw):
    from oracle.gpt_ref import build_gpt_ref
    return {k: v.clone() for k, v in build_gpt_ref(seed, **kw).state_dict().items()}


def _bn_statistics(product):
    product.pull_bn_statistics()
    return {k: v.detach().cpu().clone() for k, v in product.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def _assert_same_to_the_atomics(a, b, tag, min_checked=150):
    """a, b: (loss, {name: gradient}, {name: running statistic} or None)."""
    assert abs(a[0] - b[0]) < LOSS_BAR, (tag, a[0], b[0])
    checked, worst = 0, (0.0, 0.0)
    for k, ga in a[1].items():
        gb = b[1][k]
        if float(ga.abs().max()) < 1e-12:
            continue
        l2, mx = float((ga - gb).norm() / ga.norm()), float((ga - gb).abs().max() / ga.abs().max())
        worst = (max(worst[0], l2), max(worst[1], mx))
        assert l2 < L2_BAR, (tag, k, l2)
        assert mx < MAX_BAR, (tag, k, mx)
        checked += 1
    print(f"{tag}: loss {a[0]:.7f} vs {b[0]:.7f}, {checked} tensors, worst relative L2 {worst[0]:.2e}, max-norm {worst[1]:.2e}")
    assert checked > min_checked, (tag, checked)
    if a[2] is not None:
        assert a[2].keys() == b[2].keys() and len(a[2]) > 50
        for k, sa in a[2].items():
            d = float((sa - b[2][k]).norm() / sa.norm().clamp_min(1e-30))
            assert d < L2_BAR, (tag, k, d)


def _iteration(state, n, images, bboxes, start, forced, T, max_batch, env=None, **kw):
    """One REINFORCE iteration without the optimiser on a fresh model under activation_slots = n."""
    product = _twin(state, max_batch, block_size=T, **kw)
    product.set_activation_slots(n)
    tr = ja.ReinforceTrainer(_cfg(T=T, stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    if env is None:
        env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True)
    m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    return (float(m["loss"]), product.engine_grads(), _bn_statistics(product)), int(m["steps"]), product.activation_slots_info()


# ---- 1. the replay is exact ------------------------------------------------------------------------------------------
def _replay_diffs(B, Pp, T, steps, grid=3):
    product, _ = make_pair(5, bn_seed=None, patch_size=Pp, block_size=T, with_detector=False, image_processor=None, max_batch=B)
    images = torch.rand((B, 3, grid * Pp, grid * Pp), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    _, bboxes, start = synth_batch(B, grid, grid, 64, seed=41)
    bboxes = bboxes * (Pp // 64)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(3))
    tr = ja.ReinforceTrainer(_cfg(T=T, stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    env = ja.NeedleGeneralEnv(images, bboxes, Pp, T, 1, True)
    m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    assert m["steps"] == T
    eng = product.engine()
    out = []
    for step in steps:
        n_diff = C.c_longlong(-1)
        _lib.check(eng.lib.jn_debug_replay_diff(eng.handle, step, C.byref(n_diff), _lib.current_stream(torch.device(DEV))),
                   "jn_debug_replay_diff")
        out.append(n_diff.value)
    return product, out


def _deferred_flags(product, B):
    """(op index, deferred) of the BatchNorm convs of a train-mode encoder pass over B patches (jn_debug_forward_plan)."""
    eng = product.engine()
    buf = (C.c_int32 * (3 * 512))()
    n = eng.lib.jn_debug_forward_plan(eng.handle, _lib.JN_NET_GPT_BACKBONE, B, 1, 0, 0, buf, 512)
    assert 0 < n <= 512
    FR_STEM, FR_CONV = 1, 2
    return [(i, bool(buf[3 * i + 2])) for i in range(n) if buf[3 * i] in (FR_STEM, FR_CONV)]


@pytest.mark.parametrize("B", [3, 24])
def test_replay_reproduces_a_step_bit_for_bit(B):
    """B = 3 and B = 24 patches of 64 px, T = 4: the replay of steps 0, 2 and 3 into the eval slot differs from the resident
    slot in no 32-bit word of any buffer.  (At these sizes every layer has at most 24 * 32 * 32 pixels: all tables are
    deferred, every consumer reads the kept fp64 sums.)"""
    product, diffs = _replay_diffs(B, P, 4, (0, 2, 3))
    assert all(d for _, d in _deferred_flags(product, B))
    assert diffs == [0, 0, 0], diffs
    eng = product.engine()
    n_diff = C.c_longlong(-1)
    assert eng.lib.jn_debug_replay_diff(eng.handle, 4, C.byref(n_diff), None) != 0      # not an executed step
    if B == 3:
        # the count is not blind: once an optimiser step has moved the weights, a replay no longer reproduces the slot
        stream = _lib.current_stream(torch.device(DEV))
        _lib.check(eng.lib.jn_optimizer_step(eng.handle, 1e-2, 0.0, 1.0, 1.0, stream), "jn_optimizer_step")
        _lib.check(eng.lib.jn_debug_replay_diff(eng.handle, 2, C.byref(n_diff), stream), "jn_debug_replay_diff")
        assert n_diff.value > 3 * 32 * 32 * 16, n_diff.value                            # more words than the stem's output has


def test_replay_reproduces_a_step_with_both_table_kinds():
    """B = 2 patches of 448 px, T = 2.  JN_DEFER_MAX_M = 65536 counts pixels per launch, so at B = 2 the boundary falls
    between the 224 x 224 map and the 112 x 112 ones: the stem's output (2 * 224 * 224 = 100 352 pixels) gets its table
    from its own finalize launch and the replay reads the KEPT TABLE for it; every later layer (dark2 on: 2 * 112 * 112 =
    25 088 pixels and fewer) is deferred and the replay's consumers read the KEPT SUMS.  Both kinds are replayed."""
    product, diffs = _replay_diffs(2, 448, 2, (0, 1))
    flags = _deferred_flags(product, 2)
    assert flags[0] == (0, False) and all(d for _, d in flags[1:]) and len(flags) > 20, flags
    assert 2 * 224 * 224 > 65536 >= 2 * 112 * 112
    assert diffs == [0, 0], diffs


# ---- 2. gradients do not depend on the ring --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk5():
    B, T = 3, 5
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(3))
    state = _state(5, block_size=T, **BASE)
    base = _iteration(state, 0, images, bboxes, start, forced, T, B, **BASE)
    return dict(B=B, T=T, images=images, bboxes=bboxes, start=start, forced=forced, state=state, base=base)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_gradients_do_not_depend_on_the_ring(walk5, n):
    """B = 3, T = 5, STOP enabled: n = 1, 2, 4 (chunks 1+1+1+1+1, 2+2+1, 4+1) against n = 0 on fresh models with equal
    weights; the BatchNorm running statistics after the iteration agree too (the replay moved none)."""
    w = walk5
    base, steps0, info0 = w["base"]
    run, steps, info = _iteration(w["state"], n, w["images"], w["bboxes"], w["start"], w["forced"], w["T"], w["B"], **BASE)
    assert steps0 == steps == w["T"]
    assert info0["replayed_steps"] == 0 and info["replayed_steps"] == w["T"]
    assert (info["act_slots"], info["table_slots"]) == (n + 1, w["T"] + 1)
    _assert_same_to_the_atomics(base, run, f"ring n={n} vs all resident")


def test_steps_behind_an_early_stop_are_not_replayed(walk5):
    """Forced STOP for every agent at step 2: S = 3 < T = 5 executed steps; the steps behind S are never replayed."""
    w = walk5
    forced = w["forced"].clone()
    forced[:, 2] = 8
    args = (w["images"], w["bboxes"], w["start"], forced, w["T"], w["B"])
    base, steps0, _ = _iteration(w["state"], 0, *args, **BASE)
    run, steps, info = _iteration(w["state"], 2, *args, **BASE)
    assert steps0 == steps == 3
    assert 0 < info["replayed_steps"] <= 3
    _assert_same_to_the_atomics(base, run, "ring n=2, stopped at step 2")


# ---- 3. against the oracle -------------------------------------------------------------------------------------------
def test_reinforce_iteration_under_a_ring_vs_oracle():
    """The (True, 3, 64, 4) case of test_reinforce_iteration_gradients_vs_oracle under n = 2 (chunks 2 + 2)."""
    B, Tn = 3, 4
    product, oracle = make_pair(5, patch_size=P, block_size=Tn, nclasses=9, with_detector=False, image_processor=None)
    product.set_activation_slots(2)
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(3))
    ro, m = _oracle_reinforce_grads(oracle, images, bboxes, start, forced, P, Tn, True, 0.25, 1.5, 0.01)
    tr = ja.ReinforceTrainer(_cfg(T=Tn, stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    tr.last_return_mean, tr.last_return_std = 0.25, 1.5
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    got_m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    assert product.activation_slots_info()["replayed_steps"] == Tn
    for k in ("action_loss", "entropy_loss", "loss", "returns", "episode_length"):
        assert abs(float(got_m[k]) - float(m[k].detach())) < 2e-4, (k, float(got_m[k]), float(m[k].detach()))
    assert _check_grads(product.engine_grads(), oracle, tag="reinforce under a ring of 2") > 150


# ---- 4. the autograd bridge ------------------------------------------------------------------------------------------
def _bridge(state, n, w, flip_before_backward=None):
    product = _twin(state, w["B"], block_size=w["T"], **BASE)
    product.set_activation_slots(n)
    product.train()
    tr = ja.ReinforceTrainer(_cfg(T=w["T"], stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    env = ja.NeedleGeneralEnv(w["images"].to(DEV), w["bboxes"], P, w["T"], 1, True)
    ro = tr.rollout(env, forced_actions=w["forced"], start_positions=w["start"], keep_patches=False)
    assert ro["logprobs"].grad_fn is not None
    loss = tr.compute_metrics(ro)["loss"]
    grads = lambda: {k: p.grad.detach().cpu().clone() for k, p in product.named_parameters() if p.grad is not None}
    if flip_before_backward is not None:
        before = grads()
        product.set_activation_slots(flip_before_backward)
        with pytest.raises(JnError):
            loss.backward()
        after = grads()
        assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
        return None
    loss.backward()
    return float(loss.detach()), grads(), None


def test_the_bridge_replays_and_refuses_a_backward_under_another_setting(walk5):
    """rollout (train mode, grad enabled) -> compute_metrics -> loss.backward() under n = 2 against the same under n = 0;
    a set_activation_slots between the forward and the backward makes the backward raise (stale state) before it launches
    anything: the gradients stay what they were."""
    w = walk5
    _assert_same_to_the_atomics(_bridge(w["state"], 0, w), _bridge(w["state"], 2, w), "bridge: ring n=2 vs all resident")
    _bridge(w["state"], 2, w, flip_before_backward=0)
    _bridge(w["state"], 0, w, flip_before_backward=2)


# ---- 5. views and 8-bit images: staged columns as the replay's source ------------------------------------------------
def test_views_over_uint8_images_under_a_ring():
    B, T, G = 2, 3, 3
    u8 = torch.randint(0, 256, (B, 3, G * P, G * P), device=DEV, dtype=torch.uint8, generator=torch.Generator(device=DEV).manual_seed(29))
    _, bboxes, start = synth_batch(B, G, G, P, seed=31)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(6))
    views = ImageViews(u8, [90, 270], [5, -9], [-6, 4], patch_size=P)
    tb = views.transform_bboxes(bboxes)
    state = _state(5, block_size=T, **BASE)
    runs = []
    for n in (0, 1):
        env = ja.NeedleGeneralEnv(None, tb, P, T, 1, True, views=views)
        run, steps, info = _iteration(state, n, None, None, start, forced, T, B, env=env, **BASE)
        assert steps == T and info["replayed_steps"] == (T if n else 0)
        runs.append(run)
    _assert_same_to_the_atomics(runs[0], runs[1], "uint8 views: ring n=1 vs all resident")


# ---- 6. memory -------------------------------------------------------------------------------------------------------
def test_the_ring_holds_n_plus_one_activation_slots():
    B, T = 2, 6
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(3))
    state = _state(5, block_size=T, **BASE)
    want = {2: (3, 7, T), 0: (7, 7, 0), 8: (7, 7, 0)}           # n: (activation slots, table slots, replayed steps)
    for n, (act, tab, replayed) in want.items():
        _, steps, info = _iteration(state, n, images, bboxes, start, forced, T, B, **BASE)
        assert steps == T
        assert (info["act_slots"], info["table_slots"], info["replayed_steps"]) == (act, tab, replayed), (n, info)
        assert info["slot_bytes"] > 4 * B * 3 * 32 * 32           # at least the stem's output at max_batch


# ---- 7. a long walk: the tiled attention backward and the ring together ----------------------------------------------
def test_a_long_walk_under_a_ring():
    B, T = 2, 70
    images, bboxes, start = synth_batch(B, 4, 5, P, seed=41)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(3))
    state = _state(5, block_size=T, **BASE)
    base, s0, _ = _iteration(state, 0, images, bboxes, start, forced, T, B, **BASE)
    run, s1, info = _iteration(state, 4, images, bboxes, start, forced, T, B, **BASE)
    assert s0 == s1 == T and info["replayed_steps"] == T and info["act_slots"] == 5 and info["table_slots"] == T + 1
    _assert_same_to_the_atomics(base, run, "T=70: ring n=4 vs all resident")


# ---- 8. arguments ----------------------------------------------------------------------------------------------------
def test_arguments_and_the_detached_encoder():
    """n < 0 is refused.  Without a gpt_backbone the detector's PAFPN encodes the patches and gets no policy gradient: the
    switch is accepted and changes nothing (the trainable tensors with a gradient are the decision side's and
    embed_fpn's, fewer than the 150 of the other tests)."""
    kw = dict(patch_size=P, gpt_backbone=None, image_processor="yolox-nano")
    B, T = 3, 4
    state = _state(5, block_size=T, **kw)
    product = _twin(state, B, block_size=T, **kw)
    with pytest.raises(ValueError):
        product.set_activation_slots(-1)
    eng = product.engine()
    assert eng.lib.jn_set_activation_slots(eng.handle, -1) != 0
    assert product.activation_slots == 0
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(3))
    base, s0, i0 = _iteration(state, 0, images, bboxes, start, forced, T, B, **kw)
    run, s1, i1 = _iteration(state, 2, images, bboxes, start, forced, T, B, **kw)
    assert s0 == s1 == T and i1["replayed_steps"] == 0
    assert (i0["act_slots"], i0["table_slots"]) == (i1["act_slots"], i1["table_slots"]) and i1["act_slots"] == i1["table_slots"]
    _assert_same_to_the_atomics(base, run, "detached encoder: n=2 vs n=0", min_checked=20)
