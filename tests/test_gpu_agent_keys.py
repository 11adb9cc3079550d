"""Per-agent random streams (``jn_set_rollout_keys``, ``ReinforceTrainer.rollout(agent_keys=...)``): with every agent's
sampled draws keyed by a stream of its own, a sampled batched rollout is cut back into what each image's own ``B = 1``
rollout returns — the promise the greedy ragged tests hold ``infer_images(batch_size=k)`` to, now for its default
``sample_actions=True``.

Bars.  Two runs of the engine that differ in batch size or in an agent's place in the batch are held to the bars of
tests/test_gpu_ragged_batch.py (logits 2e-4, boxes 2e-3 px: twice what the suite holds one run to against the oracle);
runs that differ in nothing the arithmetic sees are held to their bits.

Two preconditions keep the comparison with the loop honest, both asserted on the loop run, no image excluded: at least
half of the sampled walks differ from the greedy walks (the walks really are sampled), and every draw of the loop lies at
least 1e-4 from a CDF boundary, computed on the host from the loop's logits with the Philox mirror (no coin flip on the
last bit of a logit; the host's choice is also checked against the action the engine took).

TRAINER_SEED was chosen on the CPU with ``tests/agent_keys_ref.find_seed``: the first seed 1, 2, ... on which the
oracle's own per-image walks meet both conditions with a factor 10 to spare on the margin.  Seed 1 leaves a margin of
6.2e-4; seed 2: all 7 walks differ from the greedy ones, smallest margin 2.712e-3."""
import ctypes as C

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, dist, ragged
from jolineedle_amd._lib import JnError
from jolineedle_amd.config import model_config
from oracle import gpt_ref
from tests import agent_keys_ref as ref
from tests import ragged_ref
from tests.helpers import randomize_bn, synth_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, T = ref.P, ref.T
LOGIT_BAR, BOX_BAR = 2e-4, 2e-3
TRAINER_SEED = 2         # see the module docstring
gpt_ref.GPT_ZOO.setdefault("wide-320", (2, 5, 320))
DIMS = {"gpt-nano": (3, 3, 48), "wide-320": (2, 5, 320)}
ROUTE = {"gpt-nano": 0, "wide-320": 1}      # jn_debug_decision_route: per-agent kernel, agents-batched route
INT_KEYS = ("masks", "logit_masks", "positions", "actions")
FLOAT_KEYS = ("rewards", "returns", "logprobs", "entropies", "logits", "final_emb")


def _cfg(seed=TRAINER_SEED, **kw):
    return ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=kw.pop("reward_norm", True), seed=seed, **kw)


def _same_bits(a, b, tag):
    for k in INT_KEYS + FLOAT_KEYS:
        assert a[k].shape == b[k].shape, (tag, k, a[k].shape, b[k].shape)
        assert torch.equal(a[k], b[k]), (tag, k)


def _keep(ro):
    return {k: ro[k].clone() for k in INT_KEYS + FLOAT_KEYS}


def _arm(eng, rows):
    tab = np.ascontiguousarray(np.array(rows, dtype=np.uint64).reshape(-1, 2))
    return eng.lib.jn_set_rollout_keys(eng.handle, tab.ctypes.data_as(C.c_void_p), len(tab))


# ---- 1. identity ------------------------------------------------------------------------------------------------------
def _decision_model(name, max_batch):
    base = dict(patch_size=P, block_size=T, gpt_backbone="yolox-nano", image_processor=None, with_detector=False)
    oracle = gpt_ref.build_gpt_ref(5, model_type=name, **base)
    randomize_bn(oracle, 5)
    n_layer, n_head, n_embd = DIMS[name]
    product = ja.GPT(model_config(**dict(base, model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd)), max_batch=max_batch)
    eng = product.engine()
    assert eng.lib.jn_debug_decision_route(eng.handle) == ROUTE[name]
    product.load_state_dict(oracle.eval().state_dict())
    return product


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", ["gpt-nano", "wide-320"])
def test_keys_seed_and_batch_index_give_the_bits_of_the_rollout_without_keys(name, train):
    """Keys (rollout seed, b) name the streams the engine uses on its own: same integers, same float bits, with the
    random reset drawn too.  Then other keys give other walks, a table of another size is refused before any launch
    (nothing is written), and disarming restores the default."""
    B = 5
    product = _decision_model(name, B + 1)
    product.eval()
    eng = product.engine()
    images, bboxes, _ = synth_batch(B, 3, 4, P, seed=41)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True)

    def run(agent_keys=None, **kw):
        tr = ja.ReinforceTrainer(_cfg(**kw), product)                  # a fresh counter: rollout number 1
        if train:
            tr.train_iteration(env, sample_actions=True, stop_early=False, optimizer_step=False, agent_keys=agent_keys)
            out = _keep(tr._last_train_buffers)
            out["masks"], out["logit_masks"] = out["masks"].bool(), out["logit_masks"].bool()
            return out
        return _keep(tr.rollout(env, sample_actions=True, stop_early=False, keep_patches=False, agent_keys=agent_keys))

    seed = ragged.rollout_seed(ja.ReinforceTrainer(_cfg(), product), 1)
    plain = run()
    assert len({tuple(p) for p in plain["positions"][:, 0].tolist()}) > 1, "every agent starts in one cell: the reset draw is not exercised"
    assert len({tuple(a) for a in plain["actions"].tolist()}) > 1
    _same_bits(run([(seed, b) for b in range(B)]), plain, "keys (seed, b)")
    _same_bits(run(torch.tensor([[seed, b] for b in range(B)])), plain, "keys as a tensor")
    _same_bits(run(agent_streams="global"), plain, "config.agent_streams = 'global' on one rank")
    other = run([(seed, b + 1) for b in range(B)])                     # agent b on agent b + 1's stream
    assert torch.equal(other["positions"][:B - 1, 0], plain["positions"][1:, 0])      # same grid for all: the reset draw moves along
    assert not torch.equal(other["actions"], plain["actions"])
    _same_bits(run(), plain, "after a keyed rollout: the trainer disarmed")
    # armed at the library with another n: refused, and still refused (sticky) until disarmed
    for rows in ([(seed, b) for b in range(B + 1)], [(seed, b) for b in range(B - 1)]):
        try:
            assert _arm(eng, rows) == 0
            for _ in range(2):
                with pytest.raises(JnError, match="agent streams"):
                    run()
        finally:
            assert eng.lib.jn_set_rollout_keys(eng.handle, None, 0) == 0
    with pytest.raises(AssertionError):
        run([(seed, b) for b in range(B - 1)])                         # the trainer checks the shape itself
    with pytest.raises(JnError):
        run([(seed, 1 << 32)] * B)
    _same_bits(run(), plain, "after the refusals")


# ---- the detector model and the seven images of cases 2 - 5 ----------------------------------------------------------
@pytest.fixture(scope="module")
def det():
    oracle, images = ref.build()
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=ref.THR,
                                  max_det_per_patch=128), max_batch=8)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    as_f32 = [im.float().div(255) for im, _ in images]                 # ToTensor's values: the loop and the batch see the same pixels
    return {"product": product, "imgs": as_f32, "boxes": [b for _, b in images]}


def _own_env(img_f32, boxes, engine):
    x = ragged_ref.pad_own(img_f32, P).unsqueeze(0).to(DEV).contiguous()
    return ja.NeedleGeneralEnv(x, boxes.reshape(1, -1, 4), P, T, 1, True, engine=engine)


# ---- 2. permutation ---------------------------------------------------------------------------------------------------
def test_an_agent_keeps_its_walk_when_the_batch_is_permuted(det):
    """Five images in two orders on one canvas, every image with its own key and no start position: the reset and every
    sampled action follow the image.  Nothing but the agent's row in the batch differs between the two runs, and no
    kernel of the eval-mode forward sums across agents: integers exact, floats within 1e-6."""
    product, imgs, boxes = det["product"], det["imgs"][:5], det["boxes"][:5]
    perm = [3, 0, 4, 2, 1]
    tr = ja.ReinforceTrainer(_cfg(), product)
    keys = ragged.loop_agent_keys(tr, 1, range(5))
    kw = dict(sample_actions=True, stop_early=False, keep_patches=False)
    a = _keep(tr.rollout(ragged.image_env(tr, imgs, boxes), agent_keys=keys, **kw))
    b = _keep(tr.rollout(ragged.image_env(tr, [imgs[j] for j in perm], [boxes[j] for j in perm]), agent_keys=keys[perm], **kw))
    assert len({tuple(x) for x in a["actions"].tolist()}) > 1
    for row, j in enumerate(perm):
        for k in INT_KEYS:
            assert torch.equal(b[k][row], a[k][j]), (k, row, j)
        for k in FLOAT_KEYS:
            d = float((b[k][row] - a[k][j]).abs().max())
            assert d <= 1e-6, (k, row, j, d)
    # without keys the walks follow the place in the batch, not the image
    c = _keep(tr.rollout(ragged.image_env(tr, imgs, boxes), **kw))
    tr._rollouts -= 1                                                  # the same rollout number, hence the same seed, again
    d = _keep(tr.rollout(ragged.image_env(tr, [imgs[j] for j in perm], [boxes[j] for j in perm]), **kw))
    assert any(not torch.equal(d["actions"][row], c["actions"][j]) for row, j in enumerate(perm))


# ---- 3. the loop ------------------------------------------------------------------------------------------------------
class _Spy(ja.ReinforceTrainer):
    """Keeps what every rollout returned."""

    def rollout(self, env, **kw):
        ro = super().rollout(env, **kw)
        self.seen = getattr(self, "seen", []) + [{k: v.clone() for k, v in ro.items() if torch.is_tensor(v)}]
        return ro


def _infer(det, bs, sample=True, **kw):
    """infer_images on the seven images; per image the rollout it was cut from (steps, positions, actions, logits)."""
    n = len(det["imgs"])
    tr = _Spy(_cfg(detection_enabled=True, patch_size=P), det["product"])
    res = ja.infer_images(tr, det["imgs"], det["boxes"], sample_actions=sample, do_detection=True, batch_size=bs, **kw)
    walks = [None] * n
    if bs is None:
        assert len(tr.seen) == n
        for i, ro in enumerate(tr.seen):
            walks[i] = ragged.slice_rollout(ro, 0, ro["rewards"].shape[1])
    else:
        chunks = ragged.plan_chunks(det["imgs"], bs, P, 8)
        assert len(tr.seen) == len(chunks)
        for ro, chunk in zip(tr.seen, chunks):
            steps = ragged.own_steps(ro)
            for b, i in enumerate(chunk["indices"]):
                walks[i] = ragged.slice_rollout(ro, b, steps[b])
    return res, walks, tr


@pytest.fixture(scope="module")
def infer_runs(det):
    return {bs: _infer(det, bs) for bs in (None, 4, 7)}


def test_loop_preconditions_sampled_walks_and_no_draw_on_a_cdf_boundary(det, infer_runs):
    _, loop, tr = infer_runs[None]
    _, greedy, _ = _infer(det, 7, sample=False)
    n = len(loop)
    assert [tuple(w["positions"][0, 0].tolist()) for w in loop] == [tuple(w["positions"][0, 0].tolist()) for w in greedy]
    differ = sum(not (torch.equal(s["positions"], g["positions"]) and torch.equal(s["actions"], g["actions"])) for s, g in zip(loop, greedy))
    print(f"{differ} of {n} sampled walks differ from the greedy walk")
    assert 2 * differ >= n, f"precondition: only {differ} of {n} sampled walks differ from their greedy walks"
    keys = ragged.loop_agent_keys(tr, 1, range(n)).tolist()
    worst = float("inf")
    for i, (w, (seed, index)) in enumerate(zip(loop, keys)):
        logits, actions = w["logits"][0].cpu().numpy(), w["actions"][0].tolist()
        for t, act in enumerate(actions):
            want, margin, u = ref.sample_draw(logits[t], seed, index, t)
            assert want == act, (i, t, want, act, u)
            worst = min(worst, margin)
            assert margin >= ref.DRAW_MARGIN, f"precondition: image {i} step {t}: the draw {u} lies {margin} from a CDF boundary"
    print(f"smallest distance of a draw from a CDF boundary: {worst:.3e}")


@pytest.mark.parametrize("bs", [4, 7])
def test_sampled_infer_images_batched_equals_the_loop(det, infer_runs, bs):
    """``infer_images(sample_actions=True)`` with batch_size None, 4 and 7: the same walk per image whatever shares its
    chunk (with 4 the images meet other neighbours, on another canvas, in another row than with 7)."""
    (loop, lw, ltr), (bat, bw, btr) = infer_runs[None], infer_runs[bs]
    n = len(lw)
    assert ltr._rollouts == btr._rollouts == n
    assert bat["steps"] == loop["steps"] == [w["actions"].shape[1] for w in lw]
    n_boxes = 0
    for i in range(n):
        assert torch.equal(bat["positions"][i], loop["positions"][i]), i
        for k in ("positions", "actions", "masks", "rewards", "returns"):
            assert torch.equal(bw[i][k], lw[i][k]), (i, k)
        err = float((bw[i]["logits"] - lw[i]["logits"]).abs().max())
        assert (bat["boxes"][i] is None) == (loop["boxes"][i] is None), i
        berr = 0.0
        if loop["boxes"][i] is not None:
            assert bat["boxes"][i].shape == loop["boxes"][i].shape, i
            berr = float((bat["boxes"][i] - loop["boxes"][i]).abs().max())
            n_boxes += len(loop["boxes"][i])
        print(f"image {i}: steps {loop['steps'][i]} logits differ by {err:.3e}, boxes by {berr:.3e} px")
        assert err <= LOGIT_BAR and berr <= BOX_BAR, (i, err, berr)
    assert n_boxes > 0, "no box anywhere: the comparison of the detections is empty"
    assert list(bat["metrics"]) == list(loop["metrics"])


def test_streams_batch_keeps_the_draws_keyed_by_the_place_in_the_chunk(det, infer_runs):
    """streams="batch": the chunk's seed and the agent's row — agent 0 of the first chunk is rollout 1's agent 0 and walks
    as in the loop, some later agent does not."""
    _, lw, _ = infer_runs[None]
    res, bw, tr = _infer(det, 7, streams="batch")
    assert tr._rollouts == len(lw)
    assert torch.equal(bw[0]["actions"], lw[0]["actions"]) and torch.equal(bw[0]["positions"], lw[0]["positions"])
    assert any(not torch.equal(b["positions"], l["positions"]) for b, l in zip(bw[1:], lw[1:]))
    with pytest.raises(ValueError):
        ja.infer_images(tr, det["imgs"], det["boxes"], streams="batch")
    with pytest.raises(ValueError):
        ja.infer_images(tr, det["imgs"], det["boxes"], batch_size=4, streams="image")


# ---- 4. random reset --------------------------------------------------------------------------------------------------
def test_keyed_random_reset_starts_where_the_loop_starts(det):
    product, imgs, boxes = det["product"], det["imgs"], det["boxes"]
    n = len(imgs)
    tr = ja.ReinforceTrainer(_cfg(), product)
    env = ragged.image_env(tr, imgs, boxes)
    extents = env.grid_extents.tolist()
    assert [tuple(e) for e in extents] == ref.GRIDS
    for first in (1, 50):
        keys = ragged.loop_agent_keys(tr, first, range(n))
        ro = tr.rollout(env, sample_actions=True, keep_patches=False, agent_keys=keys)         # no start_positions
        want = ragged.loop_start_positions(tr, first, range(n), extents)
        assert torch.equal(ro["positions"][:, 0].cpu(), want), (first, ro["positions"][:, 0].tolist(), want.tolist())
    # the loop itself: image i alone is agent 0 of rollout first + i
    loop_tr = ja.ReinforceTrainer(_cfg(), product)
    own = [loop_tr.rollout(_own_env(im, b, product.engine()), sample_actions=True, keep_patches=False)["positions"][0, 0].tolist()
           for im, b in zip(imgs, boxes)]
    assert own == ragged.loop_start_positions(tr, 1, range(n), extents).tolist()
    assert len({tuple(p) for p in own}) > 1


# ---- 5. multistart, "rollouts" mode -----------------------------------------------------------------------------------
def test_rollouts_mode_walks_are_the_three_sampled_rollouts_of_the_loop(det):
    """``eval_envs_on_images(eval_mode="rollouts", sample_actions=True)``, K = 3, two images per chunk (6 agents): walk
    (i, k) is rollout 1 + 3 i + k of the per-image loop — agent 0 of that rollout's seed, from walk 0's start."""
    product, K, n = det["product"], 3, 5
    imgs, boxes = det["imgs"][:n], det["boxes"][:n]
    cfg = dict(patch_size=P, max_seq_len=4, test_max_seq_len=T, stop_enabled=True, seed=TRAINER_SEED, detection_enabled=True)
    tr = ja.SupervisedTrainer(ja.CfgNode(**cfg), product)
    tr.eval_envs_on_images(imgs, boxes, batch_size=2, eval_mode="rollouts", n_starts=K, sample_actions=True)
    walks = tr.last_eval_rollouts
    assert len(walks) == n * K and tr._eval_runner()._rollouts == n * K
    loop_tr = ja.ReinforceTrainer(ja.CfgNode(max_seq_len=T, entropy_weight=0.0, stop_enabled=True, reward_norm=False,
                                             seed=TRAINER_SEED, patch_size=P, detection_enabled=True), product)
    starts = ragged.walk_start_positions(loop_tr, 1, range(n), ref.GRIDS[:n], K, "rollouts")
    worst = float("inf")
    for i in range(n):
        for k in range(K):
            assert loop_tr._rollouts == i * K + k                      # the next rollout is number 1 + i K + k
            ro = loop_tr.rollout(_own_env(imgs[i], boxes[i], product.engine()), sample_actions=True, keep_patches=False,
                                 start_positions=starts[i, k:k + 1], token_positions="sequence")
            w = walks[i * K + k]
            for t, act in enumerate(ro["actions"][0].tolist()):       # (a precondition as in case 3: no draw on a boundary)
                want, margin, u = ref.sample_draw(ro["logits"][0, t].cpu().numpy(), ragged.rollout_seed(loop_tr, 1 + i * K + k), 0, t)
                assert want == act and margin >= ref.DRAW_MARGIN, (i, k, t, want, act, margin, u)
                worst = min(worst, margin)
            assert torch.equal(w["actions"], ro["actions"][0].cpu()), (i, k)
            assert torch.equal(w["positions"], ro["positions"][0].cpu()), (i, k)
            err = float((w["logits"] - ro["logits"][0].cpu()).abs().max())
            assert err <= LOGIT_BAR, (i, k, err)
        assert all(walks[i * K + k]["positions"][0].tolist() == starts[i, 0].tolist() for k in range(K))
    print(f"smallest distance of a draw from a CDF boundary: {worst:.3e}")
    assert any(not torch.equal(walks[i * K]["positions"], walks[i * K + k]["positions"]) for i in range(n) for k in (1, 2)), \
        "every image walks three times the same way: the walks are not sampled from streams of their own"


# ---- 6. shards --------------------------------------------------------------------------------------------------------
def test_two_envs_of_three_with_their_shards_walk_like_one_env_of_six(det):
    """Global keys: the six agents of one rank and three agents on each of two ranks draw the same uniforms, so they walk
    alike (two batch sizes of one engine: integers exact, logits within the bar of the ragged tests)."""
    product = det["product"]
    images, bboxes, _ = synth_batch(6, 3, 4, P, seed=43)
    kw = dict(sample_actions=True, stop_early=False, keep_patches=False)
    tr = ja.ReinforceTrainer(_cfg(agent_streams="global"), product)
    whole = _keep(tr.rollout(ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True), **kw))
    assert len({tuple(a) for a in whole["actions"].tolist()}) > 1
    for rank in range(2):
        part = ja.ReinforceTrainer(_cfg(), product, rank=rank)
        keys = dist.shard_agent_keys(part.seed, 1, rank, 2, 3)
        sl = slice(3 * rank, 3 * rank + 3)
        got = _keep(part.rollout(ja.NeedleGeneralEnv(images[sl].to(DEV), bboxes[sl], P, T, 1, True), agent_keys=keys, **kw))
        for k in INT_KEYS + ("rewards", "returns"):
            assert torch.equal(got[k], whole[k][sl]), (rank, k)
        err = float((got["logits"] - whole["logits"][sl]).abs().max())
        print(f"rank {rank}: logits differ by {err:.3e}")
        assert err <= LOGIT_BAR, (rank, err)
    # without keys both ranks would repeat agents 0..2 of the same seed
    same = [_keep(ja.ReinforceTrainer(_cfg(), product, rank=r).rollout(
        ja.NeedleGeneralEnv(images[:3].to(DEV), bboxes[:3], P, T, 1, True), **kw))["actions"] for r in range(2)]
    assert torch.equal(same[0], same[1])
