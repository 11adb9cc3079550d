"""Batched rollouts over images of unequal size that reproduce the per-image loop of the reference's inference and
test (infer.py:87-221, src/reinforce.py:383-392): the images of a chunk become one ``ImageViews`` on the smallest canvas
that holds them, every agent is kept inside its own image (``NeedleGeneralEnv(..., clamp_to_image=True)``), and the one
rollout of the chunk is cut back into what each image's own ``B = 1`` rollout would have returned.

What makes the cut exact: agent b of a batch never reads another agent's state; a ``B = 1`` rollout stops at the first
step after which its agent is terminated or truncated, and in a batch that step is the first t with masks[b, t] == 0
(termination is sticky), or the chunk's own last step; the returns are a suffix sum over rewards * logit_masks, to which
the masked steps after that point add exact zeros.  The env of the batch keeps stepping an agent after its own end (a
stopped agent still moves), so the found-ratios are rebuilt from the positions up to the image's own last step and not
read from the env's final state."""
import time
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from .env import NeedleGeneralEnv
from .views import ImageViews

# a padding row of a stacked box tensor that marks no patch and splits into no piece (x2 < x1); all-zero rows are not
# padding here: the per-image loop gives an image without targets the box (0, 0, 0, 0), which marks patch (0, 0)
INERT_BOX = (0, 0, -1, -1)

_PER_STEP = ("rewards", "returns", "logprobs", "entropies", "logit_masks", "actions", "logits", "teacher_sets", "action_sets")
_PER_TOKEN = ("masks", "positions", "final_emb", "det_counts", "det_boxes", "patches")


def plan_chunks(images: Sequence[Tensor], batch_size: int, patch_size: int, max_batch: Optional[int] = None) -> List[Dict]:
    """The chunks ``infer_images(batch_size=k)`` runs: the images in input order, `k` at a time; the uint8 and the
    floating-point images of such a group go to separate chunks (one env reads one element type); every chunk gets the
    smallest canvas (a multiple of `patch_size`) that holds its images.  Needs only shapes and dtypes (no device)."""
    k, P = int(batch_size), int(patch_size)
    assert k >= 1, "batch_size must be at least 1"
    assert max_batch is None or k <= int(max_batch), f"batch_size {k} exceeds the model's max_batch {max_batch}"
    plan = []
    for start in range(0, len(images), k):
        group = range(start, min(start + k, len(images)))
        parts = [[i for i in group if (images[i].dtype == torch.uint8) == u8] for u8 in (True, False)]
        for sel in sorted((p for p in parts if p), key=lambda p: p[0]):
            canvas = tuple(max(-(-int(images[i].shape[d]) // P) for i in sel) * P for d in (-2, -1))
            plan.append({"indices": sel, "uint8": images[sel[0]].dtype == torch.uint8, "canvas": canvas})
    return plan


def stack_inert(bbox_rows: Sequence[Tensor]) -> Tensor:
    """[B, nb, 4] int64 from per-image [n_i, 4] rows, padded with ``INERT_BOX``."""
    nb = max(1, max(int(r.shape[0]) for r in bbox_rows))
    out = torch.tensor(INERT_BOX, dtype=torch.int64).repeat(len(bbox_rows), nb, 1)
    for i, r in enumerate(bbox_rows):
        out[i, :r.shape[0]] = r.to(torch.int64).reshape(-1, 4)
    return out


def image_env(trainer, images: Sequence[Tensor], bbox_rows: Sequence[Tensor], canvas=None) -> NeedleGeneralEnv:
    """One ragged env over `images` ([3, Hi, Wi], all uint8 — read in place — or all floating point, 0..1) on the
    model's engine; bbox_rows[i]: [n_i, 4] xyxy in image i's own pixels."""
    dev, P = trainer.device, int(trainer.patch_size)
    srcs = [im.to(dev) if im.dtype == torch.uint8 else im.to(dev, torch.float32) for im in images]
    views = ImageViews(srcs, patch_size=P, canvas=canvas)
    return NeedleGeneralEnv(None, stack_inert(bbox_rows), P, trainer.max_ep_len, 1, bool(trainer.stop_enabled),
                            engine=trainer.model.engine(), views=views, clamp_to_image=True)


def _philox4x32(seed: int, c0: int, c1: int, c2: int, c3: int):
    """Philox4x32-10 as the engine computes it (csrc/jn_device.h), on Python integers."""
    k0, k1, m = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def rollout_seed(trainer, number: int) -> int:
    """The seed ``ReinforceTrainer.rollout`` hands to the engine for its rollout number `number`."""
    return (trainer.seed * 1000003 + number) & 0xFFFFFFFFFFFFFFFF


def loop_start_positions(trainer, first_rollout: int, indices: Sequence[int], extents: Sequence[Sequence[int]]) -> Tensor:
    """[n, 2] the start position image indices[j] draws in the per-image loop: there it is agent 0 of rollout number
    `first_rollout` + indices[j] of this trainer, whose reset draws (y, x) = Philox(rollout seed, agent 0) modulo the
    image's own grid (env_reset_kernel).  Handing these to the batched rollout makes it start where the loop starts."""
    out = []
    for i, (gh, gw) in zip(indices, extents):
        seed = rollout_seed(trainer, first_rollout + i)
        r = _philox4x32(seed, 0, 0, 0x52455345, 0)
        out.append([r[0] % gh, r[1] % gw])
    return torch.tensor(out, dtype=torch.int64)


def loop_agent_keys(trainer, first_rollout: int, indices: Sequence[int]):
    """uint64 [n, 2] = (stream seed, stream index) of the random stream image indices[j] draws from in the per-image
    loop: there it is agent 0 of rollout number `first_rollout` + indices[j], so its key is (that rollout's seed, 0).
    Handed to the batched rollout as ``agent_keys`` they make every agent sample the actions the loop samples (and
    draw 0 of the same stream's reset is ``loop_start_positions``)."""
    import numpy as np
    return np.array([[rollout_seed(trainer, first_rollout + i), 0] for i in indices], dtype=np.uint64).reshape(-1, 2)


EVAL_MODES = ("multistart", "corners", "rollouts")


def walk_agent_keys(trainer, first_rollout: int, indices: Sequence[int], n_walks: int):
    """uint64 [n * K, 2] the streams of the K walks of every image of ``walk_start_positions``, in image order then
    walk order: walk (i, k) is rollout number first_rollout + i * K + k of the per-image loop in every mode — under
    "rollouts" too, where it starts at walk 0's position but samples from its own rollout's stream."""
    K = int(n_walks)
    return loop_agent_keys(trainer, first_rollout, [i * K + k for i in indices for k in range(K)])


N_CLASS_ROWS = 100       # rows of embed_class (src/models/gpt.py:227)


def image_classes(class_ids, n_images: int) -> Optional[List[int]]:
    """`class_ids` of an evaluation or inference entry point — None, or one integer per image as a tensor (any device:
    one readback) or a sequence — as a list of Python integers; None stays None (every walk under class 0, no call to
    the engine).  An id outside ``embed_class`` raises what ``GPT.forward`` raises, before anything runs."""
    if class_ids is None:
        return None
    ids = [int(c) for c in (class_ids.detach().reshape(-1).tolist() if torch.is_tensor(class_ids) else class_ids)]
    assert len(ids) == n_images, f"class_ids must name one class per image ({n_images}), got {len(ids)}"
    assert all(0 <= c < N_CLASS_ROWS for c in ids), "class id outside embed_class (100 rows)"
    return ids


def walk_classes(class_ids: Optional[Sequence[int]], indices: Sequence[int], n_walks: int = 1) -> Optional[List[int]]:
    """The ``classes`` of a chunk's rollout: agent j * K + k carries the class of image indices[j], so the K walks of an
    image share its class (test_model_on_env gets the image's ``class_id`` for every start, src/supervised.py:663-687)."""
    if class_ids is None:
        return None
    return [int(class_ids[i]) for i in indices for _ in range(int(n_walks))]


def chunk_walks(trainer, first_rollout: int, indices: Sequence[int], extents: Sequence[Sequence[int]], n_walks: int = 1,
                sample_actions: bool = False, streams: str = "loop", class_ids: Optional[Sequence[int]] = None,
                walk_starts=None) -> Dict:
    """Who walks what in one chunk of ``rollout_chunks``, from numbers alone (no device): the n images `indices`, grid
    extents[j] = (gh, gw), run as n * K agents, agents j * K .. j * K + K - 1 walking image indices[j].  "sel": per agent
    its walk number i * K + k; "image_of": its image; "starts" int64 [n * K, 2]: where rollout first_rollout + i * K + k of
    the per-image loop would start (``loop_start_positions``), or walk_starts(first_rollout, indices, extents) -> [n, K, 2];
    "keys": the stream of that same rollout (``walk_agent_keys``), so that a sampled walk is that rollout's walk — None,
    and then no call to the engine, for greedy walks and for streams="batch" (draws keyed by the chunk's seed and the
    agent's place in the chunk); "classes": ``walk_classes``."""
    K = int(n_walks)
    sel = [i * K + k for i in indices for k in range(K)]
    if walk_starts is not None:
        starts = torch.as_tensor(walk_starts(first_rollout, indices, extents)).reshape(len(sel), 2).to(torch.int64)
    else:
        starts = loop_start_positions(trainer, first_rollout, sel, [e for e in extents for _ in range(K)])
    keys = walk_agent_keys(trainer, first_rollout, indices, K) if sample_actions and streams == "loop" else None
    return {"sel": sel, "image_of": [a // K for a in sel], "starts": starts, "keys": keys,
            "classes": walk_classes(class_ids, indices, K)}


def images_per_chunk(max_batch: Optional[int], n_walks: int) -> Optional[int]:
    """The most images one chunk of K walks each may hold: n * K agents stay within the model's max_batch."""
    return max_batch if max_batch is None or int(n_walks) == 1 else int(max_batch) // int(n_walks)


def rollouts_after(first_rollout: int, n_images: int, n_walks: int = 1) -> int:
    """The rollout counter after the per-image loop has walked `n_images` images K times from `first_rollout` on."""
    return first_rollout - 1 + n_images * int(n_walks)


@torch.no_grad()
def rollout_chunks(trainer, images: Sequence[Tensor], rows: Sequence[Tensor], batch_size: int, walks: int = 1,
                   sample_actions: bool = False, do_detection: bool = False, token_positions: Optional[str] = None,
                   streams: str = "loop", class_ids=None, teacher_targets=None, walk_starts=None, action_mask: Optional[str] = None):
    """The chunked rollouts behind every batched evaluation and inference: `images` ([3, Hi, Wi], rows[i] their [n_i, 4]
    boxes) `batch_size` images at a time (``plan_chunks``), every image walked K = `walks` times as ``chunk_walks`` lays
    out — the same stored image, one view-table row per walk with the same source pointer.  Yields one record per chunk:
    "indices" (its images), "sel", "env", "extents" (per agent), "rollout" (``rollout(bbox_lists=False)``), "steps"
    (``own_steps``), "found" (``found_ratios``), "targets", "rows", "walks" and "seconds" (from the rollout's call to the
    readback of its masks); then leaves the trainer's rollout counter where the per-image loop would.
    teacher_targets: a callable (box rows of the chunk's images, their grid extents, the canvas grid) -> uint8
    [n, Gh, Gw]; the rollouts then carry "teacher_sets", "targets" is that grid per agent on the device (else None), and
    the found-ratios count these cells instead of the env's bbox masks.  class_ids: one class per IMAGE, or None.
    action_mask: handed to every rollout (``RolloutRunner.rollout``); every agent's sets are formed on its own extent."""
    class_ids = image_classes(class_ids, len(images))
    if streams not in ("loop", "batch"):
        raise ValueError(f"streams must be 'loop' or 'batch', got {streams!r}")
    K, dev = int(walks), trainer.device
    assert K >= 1 and len(rows) == len(images)
    first = trainer._rollouts + 1                         # the loop's walk k of image i is this trainer's rollout first + i * K + k
    bound = images_per_chunk(getattr(trainer.model, "max_batch", None), K)
    for chunk in plan_chunks(images, batch_size, int(trainer.patch_size), bound):
        imgs_of = chunk["indices"]
        # one upload per image; its K walks hand the SAME tensor to the env, so their views share one source
        once = {i: images[i].to(dev) if images[i].dtype == torch.uint8 else images[i].to(dev, torch.float32) for i in imgs_of}
        env = image_env(trainer, [once[i] for i in imgs_of for _ in range(K)], [rows[i] for i in imgs_of for _ in range(K)],
                        canvas=chunk["canvas"])
        extents = env.grid_extents.tolist()
        plan = chunk_walks(trainer, first, imgs_of, extents[::K], K, sample_actions, streams, class_ids, walk_starts)
        tg_grid = None
        if teacher_targets is not None:
            tg_grid = teacher_targets([rows[i] for i in imgs_of], extents[::K], (env.n_vertical_patches, env.n_horizontal_patches))
            tg_grid = tg_grid.to(dev)                     # uploaded once per chunk
            if K > 1:
                tg_grid = tg_grid.repeat_interleave(K, 0)
        t0 = time.perf_counter()
        ro = trainer.rollout(env, sample_actions=sample_actions, do_detection=do_detection, bbox_lists=False,
                             start_positions=plan["starts"], token_positions=token_positions, agent_keys=plan["keys"],
                             classes=plan["classes"], teacher=tg_grid is not None, teacher_targets=tg_grid,
                             action_mask=action_mask)
        steps = own_steps(ro)
        seconds = time.perf_counter() - t0
        found = found_ratios(env, ro, steps, masks=None if tg_grid is None else tg_grid.bool())
        yield {"indices": imgs_of, "sel": plan["sel"], "env": env, "extents": extents, "rollout": ro, "steps": steps,
               "found": found, "targets": tg_grid, "rows": rows, "walks": K, "seconds": seconds}
    trainer._rollouts = rollouts_after(first, len(images), K)


def walk_entries(trainer, chunk: Dict):
    """Per agent of a ``rollout_chunks`` record: (its walk number, the entries ``env_metrics`` gives it, its own
    ``B = 1`` rollout — with "teacher_targets" [1, Gh, Gw] when the teacher walked along)."""
    for b, a in enumerate(chunk["sel"]):
        ro_b = slice_rollout(chunk["rollout"], b, chunk["steps"][b])
        if chunk["targets"] is not None:
            ro_b["teacher_targets"] = chunk["targets"][b:b + 1]
        yield a, dict(env_metrics(trainer, chunk["found"], ro_b, b)), ro_b


@torch.no_grad()
def eval_image_chunks(trainer, yolox, chunks, do_detection: bool, merge_bboxes: bool = False, device_metrics: bool = False) -> list:
    """Behind ``ReinforceTrainer.eval_on_images`` and ``SupervisedTrainer.eval_on_images`` (whose rollouts carry the
    teacher): from the records of ``rollout_chunks`` with one walk per image, per image in image order (the metrics that
    do not come from ``compute_metrics`` — the env's entries and, with detection, `map` and the `yolo_*` of the detector
    `yolox` —, the image's own ``B = 1`` rollout).  `trainer`: anything with ``stop_enabled``, ``patch_size``, ``device``."""
    from .detection import (detection_targets, map_50_device, merge_boxes_device, pack_boxes, rollout_boxes_packed,
                            split_bboxes_over_patches, unpack_boxes)
    P = int(trainer.patch_size)
    per_image = {}
    for chunk in chunks:
        sel, env, ro, extents, rows = chunk["sel"], chunk["env"], chunk["rollout"], chunk["extents"], chunk["rows"]
        packed = rollout_boxes_packed(ro, P) if do_detection else None
        if do_detection and device_metrics:
            tg = pack_boxes([detection_targets(rows[i].unsqueeze(0), *extents[b], P)[0] for b, i in enumerate(sel)], 5,
                            trainer.device)
            pr = packed
            if merge_bboxes:
                pr, tg = merge_boxes_device(*pr, target=False), merge_boxes_device(*tg, target=True)
            maps = map_50_device(pr, tg, per_image=True)
        elif do_detection:
            full = unpack_boxes(*packed)
        for b, (i, metrics, ro_b) in enumerate(walk_entries(trainer, chunk)):     # metrics: what follows compute_metrics' own entries
            per_image[i] = (metrics, ro_b)
            if not do_detection:
                continue
            gh, gw = extents[b]
            box = rows[i].unsqueeze(0)
            # env.get_detection_batch(sample_neg=0) of the image's own env: every patch that holds a piece of a box
            local, masks = split_bboxes_over_patches(box, gh, gw, P)
            cells = torch.nonzero(masks.any(-1)[0].cpu())
            patches = env.views.gather(torch.full((len(cells),), b, dtype=torch.int64), cells, P)
            patch_targets = torch.stack([torch.nn.functional.pad(local[0, y, x], (1, 0)) for y, x in cells.tolist()]).to(trainer.device)
            if device_metrics:
                metrics["map"] = torch.tensor([maps[b]], dtype=torch.float32)
                metrics.update(detector_eval_metrics(yolox, patches, patch_targets))
            else:
                metrics.update(detection_eval_metrics(yolox, [full[b]], detection_targets(box, gh, gw, P), patches,
                                                      patch_targets, merge_bboxes))
    return [per_image[i] for i in range(len(per_image))]


def detection_eval_metrics(yolox, preds, targets, patches, patch_targets, merge_bboxes: bool) -> Dict[str, Tensor]:
    """The detection half of ``eval_on_sample`` (src/reinforce.py:455-497), shared by ``eval_on_batch`` and
    ``eval_image_chunks``: mAP-50 of the full-image predictions (optionally merged) and the detector's own mAP and
    losses on the patches that hold a box."""
    from .detection import compute_detection_metrics, merge_boxes_batched
    if merge_bboxes:
        preds = merge_boxes_batched(preds, target=False)
        targets = merge_boxes_batched(targets, target=True)
    metrics = dict(compute_detection_metrics(preds, targets))
    metrics.update(detector_eval_metrics(yolox, patches, patch_targets))
    return metrics


def detector_eval_metrics(yolox, patches, patch_targets) -> Dict[str, Tensor]:
    """The `yolo_*` entries of ``detection_eval_metrics``: the detector `yolox` alone on the patches that hold a box."""
    from .detection import compute_detection_metrics
    metrics = {}
    pred_bboxes, _, yolo_losses = yolox(patches)
    for k, v in compute_detection_metrics(pred_bboxes, list(patch_targets)).items():
        metrics["yolo_" + k] = v
    for k, v in yolo_losses.items():
        metrics["yolo_" + k] = v
    return metrics


def walk_start_positions(trainer, first_rollout: int, indices: Sequence[int], extents: Sequence[Sequence[int]], n_walks: int,
                         eval_mode: str = "multistart") -> Tensor:
    """[n, K, 2] the starts of the K walks of every image in ``eval_envs`` (src/supervised.py:668-690), image
    indices[j] with grid extents[j] = (gh, gw):
    "multistart" — walk (i, k) is rollout number first_rollout + i * K + k of the per-image loop and starts where that
    rollout's random reset would (``loop_start_positions``); "rollouts" — every walk of image i starts where its walk 0
    does under "multistart"; "corners" — the corners of the image's own grid in ``iter_corners`` order
    (src/env/simple_env.py:46-52): (0, 0), (gh - 1, 0), (gh - 1, gw - 1), (0, gw - 1), so K = 4."""
    K = int(n_walks)
    if eval_mode == "multistart":
        walks = [i * K + k for i in indices for k in range(K)]
        return loop_start_positions(trainer, first_rollout, walks, [e for e in extents for _ in range(K)]).reshape(-1, K, 2)
    if eval_mode == "rollouts":
        return loop_start_positions(trainer, first_rollout, [i * K for i in indices], extents).unsqueeze(1).repeat(1, K, 1)
    if eval_mode == "corners":
        assert K == 4, "the corners mode walks every image from its four corners"
        return torch.tensor([[[0, 0], [gh - 1, 0], [gh - 1, gw - 1], [0, gw - 1]] for gh, gw in extents],
                            dtype=torch.int64).reshape(-1, 4, 2)
    raise ValueError(f"eval_mode must be one of {EVAL_MODES}, got {eval_mode!r}")


def own_steps(rollout: Dict) -> List[int]:
    """Per image the step count its own ``B = 1`` rollout reports: the first t >= 1 with masks[b, t] == 0, else all S."""
    masks = rollout["masks"]
    S = masks.shape[1] - 1
    ended = ~masks[:, 1:]
    first = torch.where(ended.any(1), ended.to(torch.int64).argmax(1) + 1, torch.full((masks.shape[0],), S, device=masks.device))
    return [int(v) for v in first.tolist()]


def slice_rollout(rollout: Dict, b: int, steps: int) -> Dict:
    """Image b's part of a batched rollout, cut to its own `steps`: the dict of its ``B = 1`` rollout."""
    out = {}
    for k, v in rollout.items():
        if k in _PER_STEP:
            out[k] = None if v is None else v[b:b + 1, :steps]
        elif k in _PER_TOKEN:
            out[k] = None if v is None else v[b:b + 1, :steps + 1]
        elif k == "bboxes":
            out[k] = [v[b][:steps + 1]] if v and v[b] else [[]]
        else:
            out[k] = v
    return out


@torch.no_grad()
def found_ratios(env: NeedleGeneralEnv, rollout: Dict, steps: Sequence[int], masks: Optional[Tensor] = None) -> Tensor:
    """``env.prop_patches_found`` [B] as it stands after each image's own last step: the patches marked by a box among
    those visited at positions[b, 0..steps[b]] (same integer counts and the same division as the env's property).
    masks: bool [B, Gh, Gw] to count instead of the env's bbox masks."""
    pos = rollout["positions"]
    B, n = pos.shape[0], pos.shape[1]
    Gh, Gw = env.n_vertical_patches, env.n_horizontal_patches
    st = torch.tensor(list(steps), device=pos.device).unsqueeze(1)
    own = torch.arange(n, device=pos.device).unsqueeze(0) <= st                  # [B, S + 1]
    cell = (torch.arange(B, device=pos.device).unsqueeze(1) * Gh + pos[..., 0]) * Gw + pos[..., 1]
    visited = torch.zeros(B * Gh * Gw, dtype=torch.bool, device=pos.device)
    visited[cell[own]] = True
    m = env.bbox_masks if masks is None else masks
    count = (m & visited.view(B, Gh, Gw)).sum(dim=(1, 2))
    tot = m.sum(dim=(1, 2))
    tot[tot == 0] = 1
    return count / tot


def env_metrics(trainer, found: Tensor, rollout_b: Dict, b: int) -> Dict[str, Tensor]:
    """The entries ``compute_metrics(rollout, env)`` reads from a ``B = 1`` env (src/reinforce.py:254-263) for image b."""
    f = found[b]
    m = {"prop_patches_found": f, "prop_bbox_found": (found > 0).to(torch.float32)[b]}
    if trainer.stop_enabled:
        stopped = (rollout_b["actions"][0] == 8).any()       # STOP ends a B = 1 rollout, so it can only be its last action
        m["stop_used"] = stopped.to(torch.float32)
        m["stop_misused"] = (stopped & (f < 1)).to(torch.float32)
    return m
