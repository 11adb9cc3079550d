"""Rollouts whose tokens sit at their sequence position (``token_positions="sequence"``, jn_set_rollout_positions), the
teacher's action sets computed inside the rollout (jn_set_rollout_teacher) and ``SupervisedTrainer.eval_on_images``.

The yardstick of the position mode is the CPU oracle built with ``no_recurrent_embedding=True``: its rollout forwards the
whole prefix again at every step (src/models/gpt.py:427-428, 331-354), the reference's semantics; the bar is the one of
the recurrent twin ``test_gpu_parity.test_rollout_forced_vs_oracle``.  The teacher's yardstick is the host function
``trajectory.teacher_action_sets`` (pinned to the reference by tests/test_teacher_cpu.py) replayed on the rollout's own
positions."""
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import ragged
from jolineedle_amd._lib import JnError
from jolineedle_amd.config import model_config
from jolineedle_amd.trajectory import simple_env_targets, teacher_action_sets
from tests import ragged_ref
from tests.helpers import make_pair, synth_batch
from tests.ragged_ref import LOGIT_GAP, THR
from tests.test_gpu_parity import TOL_LOGIT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX_BAR = 2e-3          # px: the suite holds the engine's boxes to 1e-3 px of the oracle, so two engine runs to twice that

# three images of unequal size and the seed of weights and images; see test_supervised_eval_on_images
SIZES = [(100, 150), (64, 128), (180, 120)]
SEED = 0


def _cfg(**kw):
    return ja.CfgNode(max_seq_len=kw.pop("T", 6), entropy_weight=0.01, stop_enabled=kw.pop("stop", True),
                      reward_norm=kw.pop("reward_norm", True), seed=1, **kw)


def _tensors(ro):
    return {k: v for k, v in ro.items() if torch.is_tensor(v)}


def _same_rollout(a, b):
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) == set(tb)
    for k in ta:
        assert ta[k].shape == tb[k].shape and torch.equal(ta[k], tb[k]), k


def replay_sets(positions, targets):
    """The host teacher on the states a rollout went through: at step t the agent stands at positions[:, t] and has
    visited positions[:, 0..t]."""
    pos = positions.cpu()
    B, S = pos.shape[0], pos.shape[1] - 1
    tg = targets.cpu().to(torch.uint8)
    visited = torch.zeros_like(tg)
    out = torch.zeros((B, S), dtype=torch.uint8)
    for t in range(S):
        visited[torch.arange(B), pos[:, t, 0], pos[:, t, 1]] = 1
        out[:, t] = teacher_action_sets(pos[:, t], visited, tg)
    return out


# ---- (a) parity with the full-prefix oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("dec_pos_enc", [True, False], ids=["sinusoid", "wpe"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_sequence_rollout_forced_vs_full_prefix_oracle(stop, dec_pos_enc):
    from oracle import env_ref, rollout_ref
    P, B, Tn = 64, 3, 5
    nA = 9 if stop else 8
    product, oracle = make_pair(5, patch_size=P, block_size=Tn, nclasses=nA, image_processor="yolox-nano",
                                no_recurrent_embedding=True, decoder_pos_encoding=dec_pos_enc, pos_emb_size=25)
    assert oracle.cfg.no_recurrent_embedding
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    forced = torch.randint(0, nA, (B, Tn), generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        ref = rollout_ref.rollout(oracle, env_ref.EnvRef(images, bboxes, P, Tn, 1, stop), forced_actions=forced,
                                  start_positions=start, stop_early=True)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, stop)
    tr = ja.ReinforceTrainer(_cfg(T=Tn, stop=stop), product)
    ro = tr.rollout(env, forced_actions=forced, start_positions=start, token_positions="sequence")
    S = ref["rewards"].shape[1]
    assert ro["rewards"].shape[1] == S and S >= 2
    for k in ("masks", "logit_masks", "positions", "actions"):
        assert torch.equal(ro[k].cpu(), ref[k]), k
    assert torch.equal(ro["rewards"].cpu(), ref["rewards"])
    for k in ("returns", "logprobs", "entropies", "logits"):
        err = float((ro[k].cpu() - ref[k]).abs().max())
        print(f"{k}: max |product - oracle| = {err:.3e}")
        assert err < TOL_LOGIT, k
    assert torch.equal(ro["patches"].cpu(), ref["patches"])
    # the switch does something: the same walk with every token at position 0 is far from that oracle after step 0
    rec = tr.rollout(env, forced_actions=forced, start_positions=start, token_positions="recurrent")
    assert torch.equal(rec["positions"].cpu(), ref["positions"])
    gap = float((rec["logits"].cpu()[:, 1:] - ref["logits"][:, 1:]).abs().max())
    print(f"recurrent vs full-prefix oracle, steps >= 1: {gap:.3e}")
    assert gap > 10 * TOL_LOGIT
    assert float((rec["logits"].cpu()[:, 0] - ref["logits"][:, 0]).abs().max()) < TOL_LOGIT      # step 0 IS position 0


# ---- (b) self-consistency with the engine's own full-sequence forward -----------------------------------------------
@pytest.mark.parametrize("dec_pos_enc", [True, False], ids=["sinusoid", "wpe"])
def test_sequence_rollout_is_the_last_row_of_the_full_forward(dec_pos_enc):
    P, B, Tn = 64, 3, 5
    product, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano", decoder_pos_encoding=dec_pos_enc)
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, False)
    ro = ja.ReinforceTrainer(_cfg(T=Tn, stop=False), product).rollout(env, sample_actions=False, start_positions=start,
                                                                       keep_patches=True, token_positions="sequence")
    S = ro["actions"].shape[1]
    assert S >= 2
    actions_in = torch.cat((torch.zeros((B, 1), dtype=torch.long, device=DEV), ro["actions"][:, :S - 1]), 1)
    product.eval()
    with torch.no_grad():
        logits, final_emb = product(ro["patches"][:, :S], actions_in, torch.zeros(B, dtype=torch.long), ro["positions"][:, :S])
    assert float((logits - ro["logits"]).abs().max()) < TOL_LOGIT
    assert float((final_emb - ro["final_emb"]).abs().max()) < TOL_LOGIT


# ---- (c) the default is what it was ---------------------------------------------------------------------------------
def test_recurrent_is_the_default_and_the_config_flag_selects_sequence():
    P, B, Tn = 64, 3, 5
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    product, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano")
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    kw = dict(sample_actions=False, start_positions=start)
    plain = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, **kw)
    named = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, token_positions="recurrent", **kw)
    _same_rollout(plain, named)
    assert "teacher_sets" not in plain
    seq = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, token_positions="sequence", **kw)
    assert not torch.equal(seq["logits"], plain["logits"])
    again = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, **kw)              # the switch did not stick
    _same_rollout(plain, again)
    flagged, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano", no_recurrent_embedding=True)
    envf = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    by_flag = ja.ReinforceTrainer(_cfg(T=Tn), flagged).rollout(envf, **kw)
    by_name = ja.ReinforceTrainer(_cfg(T=Tn), flagged).rollout(envf, token_positions="sequence", **kw)
    _same_rollout(by_flag, by_name)
    _same_rollout(by_flag, seq)                                                     # same weights, same mode
    with pytest.raises(ValueError):
        ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, token_positions="absolute", **kw)


# ---- (d) refusals -----------------------------------------------------------------------------------------------------
def test_sequence_mode_refusals_leave_the_engine_usable():
    P, B, Tn = 64, 2, 5
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    product, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano", decoder_pos_encoding=False,
                           pos_emb_size=3)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    tr = ja.ReinforceTrainer(_cfg(T=Tn), product)
    kw = dict(sample_actions=False, start_positions=start)
    before = tr.rollout(env, **kw)
    product.train()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        tr.rollout(env, token_positions="sequence", **kw)
    product.eval()
    with pytest.raises(JnError, match="pos_emb_size"):                  # wpe has 3 rows, the walk 5 tokens
        tr.rollout(env, token_positions="sequence", **kw)
    after = tr.rollout(env, **kw)                                       # recurrent: row 0 only
    _same_rollout(before, after)
    # the engine's own refusal of a train-mode rollout while the mode is set
    eng = product.engine()
    assert eng.lib.jn_set_rollout_positions(eng.handle, 1) == 0
    try:
        product.train()
        with pytest.raises(JnError, match="BatchNorm"):
            tr.rollout(env, **kw)                                       # model.train() + grad: jn_reinforce_forward
    finally:
        product.eval()
        assert eng.lib.jn_set_rollout_positions(eng.handle, 0) == 0
    _same_rollout(before, tr.rollout(env, **kw))


# ---- (e) the teacher inside the rollout -----------------------------------------------------------------------------
def test_teacher_sets_plain_env_with_early_stop_and_caller_targets():
    P, B, Tn = 64, 3, 6
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    product, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano")
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    tr = ja.ReinforceTrainer(_cfg(T=Tn), product)
    forced = torch.tensor([[1, 8, 0, 0, 0, 0], [3, 7, 8, 0, 0, 0], [8, 2, 5, 0, 0, 0]])      # all stopped after step 3
    ro = tr.rollout(env, forced_actions=forced, start_positions=start, teacher=True)
    S = ro["actions"].shape[1]
    assert S == 3 and ro["teacher_sets"].shape == (B, S) and ro["teacher_sets"].dtype == torch.uint8
    want = replay_sets(ro["positions"], env.bbox_masks)
    assert torch.equal(ro["teacher_sets"].cpu(), want)
    assert int((want != 0).sum()) > 0
    whole = ro["teacher_sets"]._base                                    # the [B, T] buffer the engine wrote
    assert whole.shape == (B, Tn) and not bool(whole[:, S:].any())
    # the same walk in sequence mode: the teacher does not depend on the token positions
    seq = tr.rollout(env, forced_actions=forced, start_positions=start, teacher=True, token_positions="sequence")
    assert torch.equal(seq["teacher_sets"], ro["teacher_sets"])
    # a caller's grid instead of the env's masks
    mine = (torch.rand((B, 3, 4), generator=torch.Generator().manual_seed(4)) < 0.4).to(torch.uint8)
    assert not torch.equal(mine.bool(), env.bbox_masks.cpu())
    free = tr.rollout(env, forced_actions=forced[:, :Tn].clamp(max=7), start_positions=start, teacher=True, teacher_targets=mine)
    assert free["actions"].shape[1] == Tn
    assert torch.equal(free["teacher_sets"].cpu(), replay_sets(free["positions"], mine))
    # disarmed again: a later rollout carries no sets
    assert "teacher_sets" not in tr.rollout(env, forced_actions=forced, start_positions=start)


def test_teacher_sets_ragged_env():
    P, Tn = 64, 6
    images = ragged_ref.image_set(SIZES[:2], SEED)                      # grids 2 x 3 and 1 x 2 on a 2 x 3 canvas
    product, _ = make_pair(5, patch_size=P, block_size=Tn, image_processor="yolox-nano")
    tr = ja.ReinforceTrainer(_cfg(T=Tn, stop=False), product)
    env = ragged.image_env(tr, [im for im, _ in images], [b for _, b in images])
    assert env.grid_extents.tolist() == [[2, 3], [1, 2]]
    forced = torch.tensor([[1, 3, 1, 0, 2, 6], [1, 1, 3, 0, 0, 5]])
    ro = tr.rollout(env, forced_actions=forced, start_positions=torch.zeros((2, 2), dtype=torch.long), teacher=True,
                    stop_early=False)
    assert ro["actions"].shape[1] == Tn
    masks = env.bbox_masks
    assert not bool(masks[1, 1:].any()) and not bool(masks[1, :, 2:].any())         # nothing outside the small image
    want = replay_sets(ro["positions"], masks)
    assert torch.equal(ro["teacher_sets"].cpu(), want)
    assert int((want != 0).sum()) > 0


# ---- (f) SupervisedTrainer.eval_on_images ---------------------------------------------------------------------------
def _detecting_product(P, T, max_batch=8):
    images = ragged_ref.image_set(SIZES, SEED)
    oracle = ragged_ref.build_oracle(SEED, P, T, ragged_ref.calib_patches(images, P))
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=THR,
                                  max_det_per_patch=512), max_batch=max_batch)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product, images


def test_supervised_eval_on_images():
    """Three images of unequal size at batch_size 3 and 1.  Equal integer entries need a stable argmax: the top-2 logit gap
    of every executed step is asserted as a precondition on the per-image run (the bar of test_gpu_ragged_batch.py)."""
    P, T = 64, 6
    product, images = _detecting_product(P, T)
    imgs, boxes = [im for im, _ in images], [b for _, b in images]
    cfg = dict(patch_size=P, max_seq_len=4, test_max_seq_len=T, stop_enabled=True, seed=1, detection_enabled=True)
    runs = {}
    for bs in (3, 1):
        tr = ja.SupervisedTrainer(ja.CfgNode(**cfg), product)
        runs[bs] = (tr.eval_on_images(imgs, boxes, batch_size=bs), tr.last_eval_rollouts)
        assert product.training is False
    for i, walk in enumerate(runs[1][1]):
        top = walk["logits"].topk(2, dim=-1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        print(f"image {i}: steps {walk['actions'].numel()} top-2 logit gap {gap:.3e}")
        assert gap >= LOGIT_GAP, f"precondition: image {i} has a top-2 logit gap of {gap}"
    int_keys = ("episode_length", "prop_patches_found", "teacher_agreement", "stopped_inside_bbox")
    for bs, (res, walks) in runs.items():
        assert set(int_keys) <= set(res) and "map" in res and any(k.startswith("yolo_") for k in res)
        assert not any(k in res for k in ("loss", "action_loss", "entropy_loss", "returns"))
        assert all(len(v) == len(imgs) for v in res.values())
        for i, walk in enumerate(walks):
            h, w = imgs[i].shape[-2:]
            gh, gw = -(-h // P), -(-w // P)
            tg = walk["teacher_targets"]
            assert torch.equal(tg[:gh, :gw], simple_env_targets(boxes[i], gh * P, gw * P, P)) and int(tg.sum()) == int(tg[:gh, :gw].sum())
            S = walk["actions"].numel()
            assert 1 <= S <= T and res["episode_length"][i] == S
            sets = replay_sets(walk["positions"].unsqueeze(0), tg.unsqueeze(0))[0]
            assert torch.equal(walk["teacher_sets"], sets)
            judged = [(int(s), int(a)) for s, a in zip(sets, walk["actions"]) if int(s)]
            agree = sum((s >> a) & 1 for s, a in judged) / len(judged) if judged else 0.0
            assert res["teacher_agreement"][i] == agree
            y, x = walk["positions"][-1].tolist()
            assert res["stopped_inside_bbox"][i] == float(bool(tg[y, x]))
            seen = {tuple(p) for p in walk["positions"].tolist()}
            n_found = sum(1 for c in seen if tg[c[0], c[1]])
            assert res["prop_patches_found"][i] == float(torch.tensor(n_found) / max(int(tg.sum()), 1))
    for k in int_keys:
        assert runs[3][0][k] == runs[1][0][k], k
    for a, b in zip(runs[3][1], runs[1][1]):
        for k in ("actions", "positions", "teacher_sets"):
            assert torch.equal(a[k], b[k]), k


# ---- (g) the detector does not care about the mode --------------------------------------------------------------------
def test_sequence_rollout_with_detection():
    P, T = 64, 6
    product, images = _detecting_product(P, T)
    tr = ja.ReinforceTrainer(_cfg(T=T, stop=False), product)
    env = ragged.image_env(tr, [im for im, _ in images], [b for _, b in images])
    B = len(images)
    start = torch.zeros((B, 2), dtype=torch.long)
    seq = tr.rollout(env, do_detection=True, sample_actions=False, start_positions=start, stop_early=False,
                     token_positions="sequence")
    S = seq["actions"].shape[1]
    assert S == T and int(seq["det_counts"].sum()) > 0
    n = 0
    for t in range(S + 1):
        out, _, _ = product.yolox(seq["patches"][:, t])                 # jn_detect on the patches the agents visited
        for b in range(B):
            got = seq["bboxes"][b][t]
            assert (got is None) == (out[b] is None), (b, t)
            if got is not None:
                assert got.shape == out[b].shape, (b, t)
                assert float((got[:, :4] - out[b][:, :4]).abs().max()) <= BOX_BAR, (b, t)
                assert float((got[:, 4:] - out[b][:, 4:]).abs().max()) <= 1e-5, (b, t)
                n += len(got)
    assert n == int(seq["det_counts"].sum())
    # the same walk with every token at position 0: the detector passes are the same launches on the same patches
    rec = tr.rollout(env, do_detection=True, forced_actions=seq["actions"], start_positions=start, stop_early=False,
                     token_positions="recurrent")
    assert torch.equal(rec["positions"], seq["positions"])
    assert torch.equal(rec["det_counts"], seq["det_counts"]) and torch.equal(rec["det_boxes"], seq["det_boxes"])
