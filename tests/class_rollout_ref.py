"""Oracle side of the class-conditioned rollout tests: ``oracle/rollout_ref.py::rollout`` restated with a ``classes``
argument (that file hard-codes the REINFORCE loop's zeros, src/reinforce.py:128-129; a supervised policy is walked under
``classes=sample["class_id"]``, src/supervised.py:317-331), the test models — whose ``embed_class.weight`` is drawn from
N(0, 1) instead of the init's std 0.02, so that a walk under the wrong row cannot hide inside the logit bar — and the
shapes, ids and images the CPU and the GPU tests share.  Built only from ``oracle/`` and ``tests/``: no device."""
import functools

import torch

from oracle import env_ref, gpt_ref, rollout_ref
from tests import ragged_ref
from tests.helpers import randomize_bn, synth_batch

P, T, B = 64, 4, 3
CLASS_IDS = [3, 99, 0]           # the table's last row, and 0 beside non-zero ids
EMBED_SEED = 11                  # of the N(0, 1) embed_class.weight
MOVE_BAR = 1e-2                  # what two different classes must move a walk's logits by: 100 x the eval logit bar
BASE = dict(patch_size=P, block_size=T, gpt_backbone="yolox-nano", image_processor=None, with_detector=False)
gpt_ref.GPT_ZOO.setdefault("narrow-128", (2, 4, 128))
# gpt-nano runs on the per-agent decision route; narrow-128 is small enough to be sent down the wide one by JN_GPT_WIDE=1
DIMS = {"gpt-nano": (3, 3, 48), "narrow-128": (2, 4, 128)}
# the ragged images of the evaluation / inference tests: sides of 2 - 3 patches, no side a multiple of the patch size
SIZES = [(100, 150), (150, 120), (130, 190), (120, 100)]
IMAGE_CLASS_IDS = [3, 99, 0, 7]
WEIGHT_SEED = 0
THR = 1e-3                       # the detector's confidence threshold: low, so that boxes exist
GAP = 1e-3                       # precondition of "walks equal": the top-2 logit gap of every greedy decision


def embed_class_weight(n_embd: int) -> torch.Tensor:
    return torch.randn((100, n_embd), generator=torch.Generator().manual_seed(EMBED_SEED))


def load_embed_class(model):
    with torch.no_grad():
        model.embed_class.weight.copy_(embed_class_weight(model.embed_class.weight.shape[1]))
    return model


@functools.lru_cache(maxsize=None)
def decision_oracle(name: str, sequence: bool = False):
    """`name` of DIMS with a yolox-nano patch encoder and no detector; sequence: ``no_recurrent_embedding``."""
    o = gpt_ref.build_gpt_ref(5, model_type=name, **dict(BASE, no_recurrent_embedding=sequence))
    randomize_bn(o, 5)
    return load_embed_class(o).eval()


def batch(seed: int = 31):
    """(images, bboxes, start positions, forced actions) of the B = 3, T = 4 rollouts on a 2 x 3 grid of patches."""
    images, bboxes, start = synth_batch(B, 2, 3, P, seed=seed)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(9))
    return images, bboxes, start, forced


def rollout(model, env, classes, sample_actions: bool = True, forced_actions=None, start_positions=None, stop_early: bool = True):
    """``rollout_ref.rollout`` without detection, every sequence behind ``embed_class[classes[b]]``; also returns
    "final_emb" [B, S + 1, C], the embeddings the last forward decoded."""
    Bn = env.batch_size
    actions = torch.zeros((Bn, 1), dtype=torch.long)
    classes = torch.as_tensor(classes, dtype=torch.long)
    assert classes.shape == (Bn,)
    patches, infos = env.reset(start_positions)
    positions = infos["positions"].unsqueeze(1)
    masks = [torch.ones(Bn, dtype=torch.bool)]
    rewards, logprobs, entropies, logits_all = [], [], [], []
    emb = None
    for t in range(env.max_ep_len):
        logits, emb = model(patches, actions, classes, positions, emb)
        forced = None if forced_actions is None else forced_actions[:, t]
        new_actions, lp, ent = rollout_ref.sample_from_logits(logits, not sample_actions, forced)
        new_patches, r, terminated, truncated, infos = env.step(new_actions)
        rewards.append(r); logprobs.append(lp); entropies.append(ent); masks.append(~terminated)
        logits_all.append(logits[:, -1])
        actions = torch.cat((actions, new_actions[:, None]), dim=1)
        patches = torch.cat((patches, new_patches), dim=1)
        positions = torch.cat((positions, infos["positions"][:, None]), dim=1)
        if stop_early and bool(torch.all(terminated | truncated)):
            break
    rewards = torch.stack(rewards, 1)
    masks = torch.stack(masks, 1)
    logit_masks, returns = rollout_ref.discounted_returns(rewards, masks)
    return {"rewards": rewards, "returns": returns, "logprobs": torch.stack(logprobs, 1), "entropies": torch.stack(entropies, 1),
            "masks": masks, "logit_masks": logit_masks, "positions": positions, "patches": patches, "actions": actions[:, 1:],
            "logits": torch.stack(logits_all, 1), "final_emb": emb}


def forced_rollout(model, classes, stop_early: bool = False):
    images, bboxes, start, forced = batch()
    return rollout(model, env_ref.EnvRef(images, bboxes, P, T, 1, True), classes, forced_actions=forced, start_positions=start,
                   stop_early=stop_early)


def reinforce_grads(oracle, classes, mean: float = 0.25, std: float = 1.5, ew: float = 0.01):
    """Train-mode forced rollout under `classes`, the REINFORCE loss of ``rollout_ref.reinforce_metrics``, backward."""
    oracle.train()
    oracle.zero_grad()
    ro = forced_rollout(oracle, classes, stop_early=True)
    norm = rollout_ref.ReturnNormaliser()
    norm.mean, norm.std = mean, std
    m = rollout_ref.reinforce_metrics(ro, ew, norm)
    m["loss"].backward()
    return ro, m


# ---- the detector model and the ragged images of the evaluation / inference tests --------------------------------------
@functools.lru_cache(maxsize=None)
def detector_oracle():
    """(gpt-nano with a yolox-nano encoder and detector, no_recurrent_embedding — a supervised policy —, [(uint8 image,
    boxes)])."""
    images = ragged_ref.image_set(SIZES, WEIGHT_SEED)
    oracle = ragged_ref.build_oracle(WEIGHT_SEED, P, T, ragged_ref.calib_patches(images, P), no_recurrent_embedding=True)
    return load_embed_class(oracle), images


@torch.no_grad()
def greedy_walk(oracle, img_u8, boxes, start, class_id: int):
    """The greedy ``B = 1`` walk of one image under `class_id` on the CPU oracle: actions, positions, logits [S, nA] and
    the smallest top-2 logit gap of its decisions."""
    x = ragged_ref.pad_own(img_u8, P).float().div(255).unsqueeze(0)
    env = env_ref.EnvRef(x, boxes.reshape(1, -1, 4), P, T, 1, True)
    ro = rollout(oracle, env, [class_id], sample_actions=False, start_positions=torch.as_tensor(start, dtype=torch.long).reshape(1, 2))
    top = ro["logits"][0].topk(2, dim=-1).values
    return {"actions": ro["actions"][0], "positions": ro["positions"][0], "logits": ro["logits"][0],
            "gap": float((top[:, 0] - top[:, 1]).min())}
