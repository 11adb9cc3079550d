"""``infer.infer`` of the reference (infer.py:82-221) on the accelerated rollout, without the plotting: per image — scale
to [0, 1], zero-pad to a multiple of the patch size (bottom / right), one sampled (or greedy) rollout with the detector
on every visited patch, boxes moved to full-image coordinates; with targets also the rollout and detection metrics."""
import time
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from .detection import (compute_detection_metrics, detection_targets, map_50_device, pack_boxes, patch_bboxes2full_image,
                        rollout_boxes_packed, rollout_boxes_to_image, unpack_boxes)  # noqa: F401
from .env import NeedleGeneralEnv
from .ragged import env_metrics, image_classes, plan_chunks, rollout_chunks, slice_rollout, walk_classes  # noqa: F401


def load_bboxes(bbox_fname) -> List[List[int]]:
    """One ``cls x1 y1 x2 y2`` line per box (infer.py:71-79)."""
    out = []
    with open(bbox_fname) as f:
        for line in f:
            parts = line.strip().split()
            if len(parts) >= 5:
                out.append([int(v) for v in parts[1:5]])
    return out


def pad_to_patch_multiple(image: torch.Tensor, patch_size: int) -> torch.Tensor:
    """[1, C, H, W] -> zero-padded bottom / right so that H and W are multiples of `patch_size` (infer.py:138-146)."""
    H, W = image.shape[-2:]
    ph = ((H - 1) // patch_size + 1) * patch_size
    pw = ((W - 1) // patch_size + 1) * patch_size
    return F.pad(image, (0, pw - W, 0, ph - H), value=0)


@torch.no_grad()
def infer_images(trainer, images: Sequence[torch.Tensor], targets: Optional[Sequence] = None, sample_actions: bool = True,
                 do_detection: Optional[bool] = None, batch_size: Optional[int] = None, device_metrics: bool = False,
                 token_positions: Optional[str] = None, streams: str = "loop", class_ids=None,
                 action_mask: Optional[str] = None) -> Dict:
    """`images`: [C, H, W] tensors (uint8 0..255 or float 0..1) of any sizes; `targets`: per image an [n, 4] xyxy list /
    tensor or None.  Returns per-image boxes ([n, 7] in full-image pixels or None), positions, step counts, durations
    and — where targets are given — the mean of the reference's metrics.

    batch_size=None: one ``B = 1`` env and rollout per image, the reference's loop.  batch_size=k (at most the model's
    ``max_batch``): the images in input order, k at a time, each chunk as one rollout (``ragged.plan_chunks``): uint8
    images stay bytes and are read in place, the others are fp32, every agent stays inside its own image, the boxes
    are assembled per image on the device.  Same keys, per image and in input order; ``steps[i]`` is what image i's own
    rollout reports; ``duration_ms[i]`` is its chunk's time divided by the chunk's size — a share, not a measurement
    of that image.  Every image starts where the loop's own random reset puts it
    (``ragged.loop_start_positions``) and samples its actions from the stream of its own rollout of the loop
    (``ragged.loop_agent_keys``), so on floating-point images greedy and sampled results equal the loop's up to the
    engine's rounding across batch sizes, whatever `batch_size` is and whichever images share a chunk.  streams="batch"
    keys a sampled action by the chunk's seed and the agent's place in the chunk instead (the draws before per-agent
    streams existed); it is an error without batch_size.
    On uint8 images the two do not see the same pixels: the loop scales on the device (``x.float() / 255``, which torch
    computes as a multiply by the rounded reciprocal, one ulp off b / 255 for some bytes) while the batched path reads
    the bytes as the correctly rounded b / 255 that ToTensor computes; measured on the test detector that moved a box
    by up to 3e-3 px (positions and steps unchanged).

    device_metrics=True (with batch_size): the `map` metric of a chunk's images comes from ``map_50_device`` on the
    chunk's packed boxes, one readback per chunk, instead of one host ``map_50`` per image.

    token_positions: "sequence" / "recurrent" / None, handed to every rollout (``ReinforceTrainer.rollout``): a policy
    trained in supervised mode needs "sequence".

    class_ids: one class per image (a tensor or a sequence): the class token of image i's rollout is row class_ids[i] of
    ``embed_class`` (``ReinforceTrainer.rollout(classes=...)``), in the loop and in every chunk alike — what a
    class-conditioned policy was trained under (src/supervised.py:317-331); None = class 0.

    action_mask: "grid" / "unvisited" / None, handed to every rollout (``RolloutRunner.rollout``): the sampled or greedy
    decisions are then made among the allowed actions only; None = ``config.action_mask``."""
    class_ids = image_classes(class_ids, len(images))
    cfg, dev = trainer.config, trainer.device
    P, T = int(cfg.patch_size), int(cfg.max_seq_len)
    if do_detection is None:
        do_detection = bool(getattr(cfg, "detection_enabled", False)) and trainer.yolox_model() is not None
    if streams not in ("loop", "batch"):
        raise ValueError(f"streams must be 'loop' or 'batch', got {streams!r}")
    if batch_size is not None:
        return _infer_batched(trainer, images, targets, sample_actions, do_detection, int(batch_size), device_metrics,
                              token_positions, streams, class_ids, action_mask)
    if streams != "loop":
        raise ValueError("streams='batch' needs batch_size: the per-image loop has no batch")
    if device_metrics:
        raise ValueError("device_metrics needs batch_size: the per-image loop evaluates one image at a time")
    res = {"boxes": [], "positions": [], "steps": [], "duration_ms": []}
    all_metrics = defaultdict(list)
    for i, img in enumerate(images):
        x = img.to(dev)
        x = (x.float() / 255 if not x.is_floating_point() else x.float()).unsqueeze(0)
        x = pad_to_patch_multiple(x, P).contiguous()
        tg = None if targets is None or i >= len(targets) or targets[i] is None else torch.as_tensor(targets[i]).reshape(1, -1, 4)
        bboxes = tg.to(torch.long) if tg is not None else torch.zeros((1, 1, 4), dtype=torch.long)
        env = NeedleGeneralEnv(x, bboxes, P, T, 1, bool(getattr(cfg, "stop_enabled", False)))
        t0 = time.perf_counter()
        ro = trainer.rollout(env, do_detection=do_detection, sample_actions=sample_actions, token_positions=token_positions,
                             classes=walk_classes(class_ids, [i]), action_mask=action_mask)
        torch.cuda.synchronize(dev)
        res["duration_ms"].append((time.perf_counter() - t0) * 1e3)
        offsets = ro["positions"][:, :, [1, 0]] * P                       # (y, x) grid -> (x, y) pixels
        full = patch_bboxes2full_image(ro["bboxes"], offsets, ro["masks"])
        res["boxes"].append(full[0])
        res["positions"].append(ro["positions"][0][ro["masks"][0]].cpu())
        res["steps"].append(int(ro["rewards"].shape[1]))
        if tg is not None:
            m = trainer.compute_metrics(ro, env)
            if do_detection:
                m.update(compute_detection_metrics(full, env.get_detection_targets()))
            for k, v in m.items():
                all_metrics[k].append(float(v))
    res["metrics"] = {k: sum(v) / len(v) for k, v in all_metrics.items()}
    return res


def _infer_batched(trainer, images, targets, sample_actions, do_detection, batch_size, device_metrics=False,
                   token_positions=None, streams="loop", class_ids=None, action_mask=None) -> Dict:
    dev, P = trainer.device, int(trainer.config.patch_size)
    n = len(images)
    res = {"boxes": [None] * n, "positions": [None] * n, "steps": [0] * n, "duration_ms": [0.0] * n}
    per_image = [None] * n
    has_tg = [not (targets is None or i >= len(targets) or targets[i] is None) for i in range(n)]
    # (an image without targets gets the box (0, 0, 0, 0), as in the loop)
    rows = [torch.as_tensor(targets[i]).reshape(-1, 4).to(torch.long) if h else torch.zeros((1, 4), dtype=torch.long)
            for i, h in enumerate(has_tg)]
    for ch in rollout_chunks(trainer, images, rows, batch_size, sample_actions=sample_actions, do_detection=do_detection,
                             token_positions=token_positions, streams=streams, class_ids=class_ids, action_mask=action_mask):
        sel, ro, steps, extents = ch["indices"], ch["rollout"], ch["steps"], ch["extents"]
        ms = ch["seconds"] * 1e3 / len(sel)                # (the walker read the step counts back: the rollout has ended)
        packed = rollout_boxes_packed(ro, P) if do_detection else None
        full = unpack_boxes(*packed) if do_detection else [None] * len(sel)
        maps = None
        if do_detection and device_metrics and any(has_tg[i] for i in sel):
            tg = pack_boxes([detection_targets(rows[i].unsqueeze(0), *extents[b], P)[0] if has_tg[i] else None
                             for b, i in enumerate(sel)], 5, dev)
            maps = map_50_device(packed, tg, per_image=True)
        pos_cpu, masks_cpu = ro["positions"].cpu(), ro["masks"].cpu()
        for b, i in enumerate(sel):
            res["boxes"][i] = full[b]
            res["positions"][i] = pos_cpu[b, :steps[b] + 1][masks_cpu[b, :steps[b] + 1]]
            res["steps"][i] = steps[b]
            res["duration_ms"][i] = ms
            if has_tg[i]:
                ro_b = slice_rollout(ro, b, steps[b])
                m = dict(env_metrics(trainer, ch["found"], ro_b, b))       # what follows compute_metrics' own entries
                if maps is not None:
                    m["map"] = torch.tensor([maps[b]], dtype=torch.float32)
                elif do_detection:
                    gh, gw = extents[b]
                    m.update(compute_detection_metrics([full[b]], detection_targets(rows[i].unsqueeze(0), gh, gw, P)))
                per_image[i] = (ro_b, m)
    all_metrics = defaultdict(list)
    for entry in per_image:                               # in input order, as the loop accumulates them (and as it
        if entry is not None:                             # feeds the reward-norm window through compute_metrics)
            m = trainer.compute_metrics(entry[0])
            m.update(entry[1])
            for k, v in m.items():
                all_metrics[k].append(float(v))
    res["metrics"] = {k: sum(v) / len(v) for k, v in all_metrics.items()}
    return res
