"""Class-conditioned rollouts (``jn_set_rollout_classes``, ``ReinforceTrainer.rollout(classes=...)`` and the ``class_ids``
of the evaluation / inference entry points): the class token of every walk is row ``classes[b]`` of ``embed_class``, on
both decision routes, under both token positions, in the batched backward and through the autograd bridge.

The reference loop is tests/class_rollout_ref.py (``oracle/rollout_ref.py::rollout`` with a ``classes`` argument) over
the oracle GPT and env; engine and oracle load the same N(0, 1) ``embed_class.weight``, and
tests/test_class_rollout_cpu.py asserts on the oracle alone that the ids used here move the logits by at least 1e-2.

Bars (tests/test_gpu_parity.py): eval-mode logits and final_emb TOL_LOGIT = 1e-4, train-mode logits 1e-3, decision-side
gradients L2_DECISION = 1e-3 relative L2.  Two runs of the engine that differ in the batch size are held to 1e-4 too.

Shapes: 64-px patches, a 2 x 3 grid (ragged images of 2 - 3 patches a side), B = 3, T = 4.  At such a shape the GPT
backward is always the batched one (``launch_gpt_backward_batched``): it hands a shape to the per-agent fallback
(``launch_gpt_backward``) only when 4 (T + 1) head_size + 2 (T + 1)^2 floats exceed 64 KiB of LDS: never at the head
sizes of gpt-nano (16) and narrow-128 (32) within the trainable block size of 62, from T = 46 at head size 64 and from
T = 15 at a single head of 256 channels — no shape of this file, so the batched form is the one tested here (the
fallback reads the same nullable pointer from the same record)."""
import ctypes as C

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import ragged
from jolineedle_amd._lib import JnError
from jolineedle_amd.config import model_config
from tests import class_rollout_ref as ref
from tests import ragged_ref
from tests.test_gpu_parity import L2_DECISION, TOL_LOGIT, build_like

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, T, B = ref.P, ref.T, ref.B
TRAIN_LOGIT = 1e-3
ROUTE = {"gpt-nano": 0, "narrow-128": 1}    # jn_debug_decision_route: per-agent kernel, agents-batched (wide) route
INT_KEYS = ("masks", "logit_masks", "positions", "actions")
FLOAT_KEYS = ("rewards", "returns", "logprobs", "entropies", "logits", "final_emb")
ENCODER = ("gpt_backbone.", "yolox.", "embed_fpn.0")     # every other tensor is decision-side (test_gpu_parity.l2_bar)


def _cfg(seed=1, **kw):
    return ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=seed, **kw)


def _keep(ro):
    return {k: ro[k].detach().clone() for k in INT_KEYS + FLOAT_KEYS}


def _same_bits(a, b, tag, rows=slice(None)):
    for k in INT_KEYS + FLOAT_KEYS:
        assert a[k].shape == b[k].shape, (tag, k, a[k].shape, b[k].shape)
        assert torch.equal(a[k][rows], b[k][rows]), (tag, k)


def _arm(eng, ids):
    tab = np.ascontiguousarray(np.array(ids, dtype=np.int64))
    return eng.lib.jn_set_rollout_classes(eng.handle, tab.ctypes.data_as(C.c_void_p), len(tab))


def _decision_product(name):
    """The engine side of ``ref.decision_oracle(name)``, on the route ROUTE[name] (narrow-128 sent down the wide one)."""
    n_layer, n_head, n_embd = ref.DIMS[name]
    with pytest.MonkeyPatch.context() as mp:
        if ROUTE[name]:
            mp.setenv("JN_GPT_WIDE", "1")
        else:
            mp.delenv("JN_GPT_WIDE", raising=False)
        product = ja.GPT(model_config(**dict(ref.BASE, model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd)), max_batch=B + 1)
    eng = product.engine()
    assert eng.lib.jn_debug_decision_route(eng.handle) == ROUTE[name]
    product.load_state_dict(ref.decision_oracle(name).state_dict())
    return product


@pytest.fixture(scope="module")
def eval_models():
    """One eval-mode product per route, shared by the eval tests (nothing they do writes to the model)."""
    return {name: _decision_product(name).eval() for name in ref.DIMS}


def _forced_run(product, tp, classes, trainer=None):
    images, bboxes, start, forced = ref.batch()
    tr = trainer or ja.ReinforceTrainer(_cfg(), product)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True)
    return _keep(tr.rollout(env, forced_actions=forced, start_positions=start, stop_early=False, keep_patches=False,
                            token_positions=tp, classes=classes))


# ---- 1. forced eval rollout with classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("tp", ["recurrent", "sequence"])
@pytest.mark.parametrize("name", list(ref.DIMS))
def test_forced_eval_rollout_under_class_ids_matches_the_reference_loop(eval_models, name, tp):
    product = eval_models[name]
    with torch.no_grad():
        want = ref.forced_rollout(ref.decision_oracle(name, tp == "sequence"), ref.CLASS_IDS)
        got = _forced_run(product, tp, ref.CLASS_IDS)
        plain = _forced_run(product, tp, None)
    for k in ("positions", "actions", "rewards", "masks", "logit_masks"):
        assert torch.equal(got[k].cpu(), want[k]), k
    for k in ("logits", "final_emb"):
        d = float((got[k].cpu() - want[k]).abs().max())
        print(f"{name} {tp}: {k} against the reference loop: {d:.3e}")
        assert d < TOL_LOGIT, (k, d)
    # the agent whose class is 0: the bits of its row of the rollout without a table (both step routes are deterministic)
    zero = ref.CLASS_IDS.index(0)
    _same_bits(got, plain, "the class-0 agent", rows=zero)
    for b, c in enumerate(ref.CLASS_IDS):       # ... and the others walk under another row (the CPU test's precondition)
        if c != 0:
            d = float((got["logits"][b] - plain["logits"][b]).abs().max())
            assert d >= ref.MOVE_BAR - 2 * TOL_LOGIT, (b, c, d)
    with torch.no_grad():
        _same_bits(_forced_run(product, tp, torch.tensor(ref.CLASS_IDS, device=DEV)), got, "ids as a device tensor")
        _same_bits(_forced_run(product, tp, [0] * B), plain, "explicit zeros")


# ---- 2. the table does not leak ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.DIMS))
def test_the_table_is_cleared_after_the_rollout_and_a_wrong_length_is_an_error(eval_models, name):
    product = eval_models[name]
    eng = product.engine()
    with torch.no_grad():
        plain = _forced_run(product, "recurrent", None)
        armed = _forced_run(product, "recurrent", ref.CLASS_IDS)
        assert not torch.equal(armed["logits"], plain["logits"])
        _same_bits(_forced_run(product, "recurrent", None), plain, "right after an armed rollout")
        # armed at the library with another n: refused before any launch, and still refused (sticky) until cleared
        for ids in (ref.CLASS_IDS + [5], ref.CLASS_IDS[:2]):
            try:
                assert _arm(eng, ids) == 0
                for _ in range(2):
                    with pytest.raises(JnError, match="class ids"):
                        _forced_run(product, "recurrent", None)
            finally:
                assert eng.lib.jn_set_rollout_classes(eng.handle, None, 0) == 0
        with pytest.raises(AssertionError, match=r"classes must be \[3\]"):
            _forced_run(product, "recurrent", ref.CLASS_IDS[:2])               # the trainer checks the length itself
        with pytest.raises(AssertionError, match="class id outside embed_class"):
            _forced_run(product, "recurrent", [3, 100, 0])
        _same_bits(_forced_run(product, "recurrent", None), plain, "after the refusals")
        _same_bits(_forced_run(product, "recurrent", ref.CLASS_IDS), armed, "armed again")


# ---- 3. train_iteration(classes=...) ----------------------------------------------------------------------------------
def _decision_grads_close(grads, oracle, tag):
    """Every decision-side gradient within L2_DECISION (relative L2) of the oracle's; returns the number checked."""
    checked = 0
    for name, p in oracle.named_parameters():
        if name.startswith(ENCODER) or p.grad is None or not p.requires_grad:
            continue
        got, want = grads[name].double(), p.grad.double()
        if want.abs().max().item() < 1e-12:
            assert got.abs().max().item() < 1e-9, name
            continue
        l2 = (got - want).norm().item() / want.norm().item()
        if l2 > 0.1 * L2_DECISION:
            print(f"{tag}: {name}: relative L2 {l2:.3e}")
        assert l2 < L2_DECISION, (tag, name, l2)
        checked += 1
    return checked


def _used_rows(grad):
    return sorted(torch.nonzero(grad.abs().amax(dim=1) > 0).flatten().tolist())


@pytest.mark.parametrize("ids", [ref.CLASS_IDS, [3, 99, 3]], ids=["with-class-0", "without-class-0"])
@pytest.mark.parametrize("name", list(ref.DIMS))
def test_train_iteration_under_class_ids_gradients_vs_oracle(name, ids):
    """The batched GPT backward on both step routes (see the module docstring for the per-agent fallback)."""
    oracle = build_like(ref.decision_oracle(name))
    ro, m = ref.reinforce_grads(oracle, ids)
    product = _decision_product(name)
    images, bboxes, start, forced = ref.batch()
    tr = ja.ReinforceTrainer(_cfg(learning_rate=1e-3, gradient_accumulation=1), product)
    tr.last_return_mean, tr.last_return_std = 0.25, 1.5
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True)
    got = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False, classes=ids)
    S = ro["logits"].shape[1]
    assert got["steps"] == S
    d = float((tr._last_train_buffers["logits"][:, :S].cpu() - ro["logits"].detach()).abs().max())
    print(f"{name} {ids}: train-mode logits against the reference loop: {d:.3e}")
    assert d < TRAIN_LOGIT, d
    assert abs(float(got["loss"]) - float(m["loss"].detach())) < 2e-4
    grads = product.engine_grads()
    assert _decision_grads_close(grads, oracle, f"{name} {ids}") > 20
    g = grads["embed_class.weight"]
    assert _used_rows(g) == sorted(set(ids)) == _used_rows(oracle.embed_class.weight.grad)
    if 0 not in ids:
        assert float(g[0].abs().max()) == 0.0


# ---- 4. autograd bridge -----------------------------------------------------------------------------------------------
def test_backward_of_a_rollout_uses_the_classes_of_its_forward_not_the_table_armed_since():
    ids = [3, 7, 3]
    oracle = build_like(ref.decision_oracle("gpt-nano"))
    ref.reinforce_grads(oracle, ids, mean=0.0, std=1.0)
    product = _decision_product("gpt-nano")
    product.train()
    eng = product.engine()
    images, bboxes, start, forced = ref.batch()
    tr = ja.ReinforceTrainer(_cfg(), product)                                  # reward-norm window: mean 0, std 1
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True)
    ro = tr.rollout(env, forced_actions=forced, start_positions=start, keep_patches=False, classes=ids)
    assert ro["logprobs"].grad_fn is not None
    loss = tr.compute_metrics(ro)["loss"]
    try:
        assert _arm(eng, [50, 51, 52]) == 0                                    # another table by the time of the backward
        loss.backward()
    finally:
        assert eng.lib.jn_set_rollout_classes(eng.handle, None, 0) == 0
    g = dict(product.named_parameters())["embed_class.weight"].grad.cpu()
    assert _used_rows(g) == [3, 7], _used_rows(g)
    want = oracle.embed_class.weight.grad
    l2 = float((g.double() - want.double()).norm() / want.double().norm())
    print(f"embed_class.weight gradient through the bridge: relative L2 {l2:.3e}")
    assert l2 < L2_DECISION, l2


# ---- the detector model and the ragged images of cases 5 and 6 --------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    oracle, images = ref.detector_oracle()
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=ref.THR,
                                  max_det_per_patch=128, no_recurrent_embedding=True), max_batch=8)
    state = {k: v.clone() for k, v in oracle.state_dict().items()}
    product.load_state_dict(state)
    product.eval()
    as_f32 = [im.float().div(255) for im, _ in images]                 # ToTensor's values: loop, batch and oracle see the same pixels
    grids = [(-(-im.shape[-2] // P), -(-im.shape[-1] // P)) for im, _ in images]

    def reset():
        """(the teacher-forced validation moves the detector head's running statistics, as the reference's does)"""
        product.load_state_dict(state)
        product.eval()

    return {"product": product, "oracle": oracle, "u8": [im for im, _ in images], "imgs": as_f32, "boxes": [b for _, b in images],
            "grids": grids, "reset": reset}


def _sup_cfg():
    return ja.CfgNode(patch_size=P, max_seq_len=T, test_max_seq_len=T, stop_enabled=True, seed=2, detection_enabled=True)


def _own_env(img_f32, boxes, engine):
    x = ragged_ref.pad_own(img_f32, P).unsqueeze(0).to(DEV).contiguous()
    return ja.NeedleGeneralEnv(x, boxes.reshape(1, -1, 4), P, T, 1, True, engine=engine)


def _walks_agree(a, b, tag):
    assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["positions"], b["positions"]), tag
    d = float((a["logits"] - b["logits"]).abs().max())
    assert d < TOL_LOGIT, (tag, d)
    return d


# ---- 5. eval_on_images / infer_images ---------------------------------------------------------------------------------
def test_eval_on_images_under_class_ids_batched_equals_the_loop_and_the_oracle(det):
    det["reset"]()
    product, imgs, boxes, ids = det["product"], det["imgs"], det["boxes"], ref.IMAGE_CLASS_IDS
    n = len(imgs)
    runs = {}
    for bs in (1, 3, 4):
        tr = ja.SupervisedTrainer(_sup_cfg(), product)
        out = tr.eval_on_images(imgs, boxes, bs, do_detection=False, class_ids=ids)
        assert len(out["episode_length"]) == n and tr._eval_runner()._rollouts == n
        runs[bs] = tr.last_eval_rollouts
    worst = max(_walks_agree(runs[bs][i], runs[1][i], (bs, i)) for bs in (3, 4) for i in range(n))
    print(f"eval_on_images, batch sizes 3 and 4 against the per-image loop: logits differ by {worst:.3e}")
    # the loop's walks are the oracle's greedy walks under the image's class, from the loop's own start cells
    starts = ragged.loop_start_positions(ja.ReinforceTrainer(_cfg(seed=2), product), 1, range(n), det["grids"])
    for i in range(n):
        want = ref.greedy_walk(det["oracle"], det["u8"][i], boxes[i], starts[i].tolist(), ids[i])
        assert want["gap"] >= ref.GAP
        _walks_agree(runs[1][i], want, ("oracle", i))
    # without ids (and with a tensor of ids on the device) ...
    tr = ja.SupervisedTrainer(_sup_cfg(), product)
    tr.eval_on_images(imgs, boxes, 3, do_detection=False)
    for i, c in enumerate(ids):
        same = torch.equal(tr.last_eval_rollouts[i]["logits"][0], runs[3][i]["logits"][0])
        assert same == (c == 0), (i, c)
    tr = ja.SupervisedTrainer(_sup_cfg(), product)
    tr.eval_on_images(imgs, boxes, 3, do_detection=False, class_ids=torch.tensor(ids, device=DEV))
    for i in range(n):
        assert torch.equal(tr.last_eval_rollouts[i]["logits"], runs[3][i]["logits"]), i


class _Spy(ja.ReinforceTrainer):
    """Keeps what every rollout returned."""

    def rollout(self, env, **kw):
        ro = super().rollout(env, **kw)
        self.seen = getattr(self, "seen", []) + [{k: v.clone() for k, v in ro.items() if torch.is_tensor(v)}]
        return ro


def test_infer_images_under_class_ids_batched_equals_the_loop(det):
    det["reset"]()
    product, imgs, boxes, ids = det["product"], det["imgs"], det["boxes"], ref.IMAGE_CLASS_IDS
    n = len(imgs)

    def infer(bs, class_ids):
        tr = _Spy(_cfg(seed=2, patch_size=P), product)
        res = ja.infer_images(tr, imgs, boxes, sample_actions=False, do_detection=False, batch_size=bs, class_ids=class_ids)
        walks = [None] * n
        if bs is None:
            for i, ro in enumerate(tr.seen):
                walks[i] = ragged.slice_rollout(ro, 0, ro["rewards"].shape[1])
        else:
            for ro, chunk in zip(tr.seen, ragged.plan_chunks(imgs, bs, P, 8)):
                steps = ragged.own_steps(ro)
                for b, i in enumerate(chunk["indices"]):
                    walks[i] = ragged.slice_rollout(ro, b, steps[b])
        return res, [{k: w[k][0].cpu() for k in ("actions", "positions", "logits")} for w in walks]

    loop, lw = infer(None, ids)
    bat, bw = infer(3, ids)
    assert bat["steps"] == loop["steps"]
    for i in range(n):
        assert torch.equal(bat["positions"][i], loop["positions"][i]), i
        _walks_agree(bw[i], lw[i], ("infer", i))
    _, zw = infer(None, None)
    for i, c in enumerate(ids):                       # the loop itself hands the image's class to its rollout
        assert torch.equal(zw[i]["logits"][0], lw[i]["logits"][0]) == (c == 0), (i, c)
        if c != 0:
            assert float((zw[i]["logits"][0] - lw[i]["logits"][0]).abs().max()) >= ref.MOVE_BAR - 2 * TOL_LOGIT, i


def test_an_image_keeps_its_walk_under_its_class_when_the_chunk_is_permuted(det):
    """The chunk's rollout itself (the entry points draw an image's start from its index, so a permutation there moves
    the starts): four images in two orders on one canvas, starts and class ids following the images.  Nothing but the
    agent's row differs and no eval-mode kernel sums across agents: integers exact, floats within 1e-6."""
    det["reset"]()
    product, imgs, boxes, ids = det["product"], det["imgs"], det["boxes"], ref.IMAGE_CLASS_IDS
    perm = [2, 0, 3, 1]
    tr = ja.ReinforceTrainer(_cfg(seed=2), product)
    starts = torch.tensor([[gh - 1, gw - 1] for gh, gw in det["grids"]])
    kw = dict(sample_actions=False, stop_early=False, keep_patches=False, token_positions="sequence")
    a = _keep(tr.rollout(ragged.image_env(tr, imgs, boxes), start_positions=starts, classes=ids, **kw))
    b = _keep(tr.rollout(ragged.image_env(tr, [imgs[j] for j in perm], [boxes[j] for j in perm]), start_positions=starts[perm],
                         classes=[ids[j] for j in perm], **kw))
    for row, j in enumerate(perm):
        for k in INT_KEYS:
            assert torch.equal(b[k][row], a[k][j]), (k, row, j)
        for k in FLOAT_KEYS:
            d = float((b[k][row] - a[k][j]).abs().max())
            assert d <= 1e-6, (k, row, j, d)
    # the ids in the OLD order over the permuted images: the class follows the row, and the walks show it
    c = _keep(tr.rollout(ragged.image_env(tr, [imgs[j] for j in perm], [boxes[j] for j in perm]), start_positions=starts[perm],
                         classes=ids, **kw))
    assert any(float((c["logits"][row, 0] - a["logits"][j, 0]).abs().max()) >= ref.MOVE_BAR - 2 * TOL_LOGIT for row, j in enumerate(perm))


# ---- 6. eval_envs_on_images / test_on_images ----------------------------------------------------------------------------
def test_both_walks_of_an_image_run_under_its_class(det):
    det["reset"]()
    product, imgs, boxes, ids = det["product"], det["imgs"], det["boxes"], ref.IMAGE_CLASS_IDS
    n, K = len(imgs), 2
    tr = ja.SupervisedTrainer(_sup_cfg(), product)
    tr.eval_envs_on_images(imgs, boxes, batch_size=2, n_starts=K, class_ids=ids)
    walks = tr.last_eval_rollouts
    assert len(walks) == n * K and tr._eval_runner()._rollouts == n * K
    loop_tr = ja.ReinforceTrainer(ja.CfgNode(max_seq_len=T, entropy_weight=0.0, stop_enabled=True, reward_norm=False, seed=2,
                                             patch_size=P, detection_enabled=True), product)
    starts = ragged.walk_start_positions(loop_tr, 1, range(n), det["grids"], K, "multistart")
    worst = 0.0
    for i in range(n):
        for k in range(K):
            ro = loop_tr.rollout(_own_env(imgs[i], boxes[i], product.engine()), sample_actions=False, keep_patches=False,
                                 start_positions=starts[i, k:k + 1], token_positions="sequence", classes=[ids[i]])
            single = {name: ro[name][0].cpu() for name in ("actions", "positions", "logits")}
            worst = max(worst, _walks_agree(walks[i * K + k], single, (i, k)))
            if ids[i] != 0:                    # ... and not under class 0
                zero = loop_tr.rollout(_own_env(imgs[i], boxes[i], product.engine()), sample_actions=False, keep_patches=False,
                                       start_positions=starts[i, k:k + 1], token_positions="sequence")
                d = float((walks[i * K + k]["logits"][0] - zero["logits"][0, 0].cpu()).abs().max())
                assert d >= ref.MOVE_BAR - 2 * TOL_LOGIT, (i, k, d)
    print(f"eval_envs_on_images: both walks of every image against single rollouts under its class: {worst:.3e}")


def _same_lists(a, b, keys):
    for k in keys:
        assert len(a[k]) == len(b[k]), k
        assert all(x == y or (x != x and y != y) for x, y in zip(a[k], b[k])), (k, a[k], b[k])


def test_test_on_images_hands_its_class_ids_to_the_walks_and_keeps_its_results_without(det):
    """One image per batch (the teacher-forced half stacks the images of a batch, and these differ in size), every image
    padded on its own to whole patches (that half walks whole patches)."""
    product, boxes, ids = det["product"], det["boxes"], ref.IMAGE_CLASS_IDS
    imgs = [ragged_ref.pad_own(im, P) for im in det["imgs"]]
    n = len(imgs)

    def run(how, class_ids):
        det["reset"]()
        tr = ja.SupervisedTrainer(_sup_cfg(), product)
        if how == "envs":
            m = tr.eval_envs_on_images(imgs, boxes, 1, class_ids=class_ids)
        else:
            m = tr.test_on_images(imgs, boxes, 1, class_ids=class_ids, seed=3)
        return m, [w["logits"].clone() for w in tr.last_eval_rollouts]

    envs, envs_logits = run("envs", ids)
    with_ids, with_logits = run("test", ids)
    _same_lists(with_ids, envs, list(envs))                                    # the lists of eval_envs_on_images(class_ids=ids)
    assert all(torch.equal(x, y) for x, y in zip(with_logits, envs_logits))
    assert len(with_ids["supervised_action_loss"]) == n
    none, none_logits = run("test", None)
    zeros, zeros_logits = run("test", [0] * n)
    _same_lists(none, zeros, list(envs) + ["supervised_action_loss", "supervised_action_accuracy", "supervised_episode_length"])
    assert all(torch.equal(x, y) for x, y in zip(none_logits, zeros_logits))   # class_ids=None: the walks under class 0, bit for bit
    for i, c in enumerate(ids):
        for k in range(2):
            assert torch.equal(with_logits[2 * i + k][0], none_logits[2 * i + k][0]) == (c == 0), (i, k, c)


# ---- the REINFORCE loop: zeros unless config.class_tokens ---------------------------------------------------------------
@pytest.mark.parametrize("flag", [None, False, True])
def test_training_step_reads_the_batch_class_ids_only_under_class_tokens(flag):
    class Spy(ja.ReinforceTrainer):
        def rollout(self, env, **kw):
            self.classes_seen = kw.get("classes")
            return super().rollout(env, **kw)

    product = _decision_product("gpt-nano")
    images, bboxes, _, _ = ref.batch()
    kw = {} if flag is None else {"class_tokens": flag}
    tr = Spy(_cfg(learning_rate=1e-3, gradient_accumulation=1, **kw), product)
    ids = torch.tensor([3, 99, 3])
    m = tr.run(0, 1, 0, batches=[{"image": images.to(DEV), "bboxes": bboxes, "class_id": ids}], max_iters=1)
    assert torch.isfinite(m["loss"])
    if flag:
        assert torch.equal(torch.as_tensor(tr.classes_seen), ids)
    else:
        assert tr.classes_seen is None                                         # the reference's zeros (src/reinforce.py:128-129)
