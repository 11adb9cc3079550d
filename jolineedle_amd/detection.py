"""Detection bookkeeping around the rollout: splitting ground-truth boxes over the patch grid,
patch -> full-image box coordinates, merging of contiguous boxes and mAP-50.  Host-side integer / float logic on small
tensors (a few boxes per image) — nothing here is on the per-glimpse hot path.  The ``*_device`` functions are the same
merge and mAP-50 for a whole batch in a few launches of the engine (csrc/kernels_eval.hip), for evaluations that carry
hundreds of boxes per image; the host functions are their comparands.

Reference: ``NeedleGeneralEnv.parse_bboxes / get_detection_targets`` (src/env/general_env.py:381-573),
``Trainer.patch_bboxes2full_image`` (src/trainer.py:250-280), ``merge_boxes`` (src/utils.py:185-255),
``Trainer.compute_detection_metrics`` (src/trainer.py:188-248; the reference calls torchmetrics' COCO
MeanAveragePrecision, which is not vendored — map_50 is restated here from the published COCO protocol and pinned by
the known answers of the reference's tests/test_map.py: 0, 1 and 0.8)."""
from typing import List, Optional, Tuple

import torch
from torch import Tensor


def split_bboxes_over_patches(bboxes: Tensor, n_vertical: int, n_horizontal: int, patch_size: int) -> Tuple[Tensor, Tensor]:
    """[B, nb, 4] xyxy image boxes -> per-patch local boxes [B, Gy, Gx, nb, 4] + masks [B, Gy, Gx, nb].

    A box that crosses a patch border is cut at the border (inclusive max = patch_size - 1) and continues in the
    neighbouring patch(es), as the reference's recursive placement does (general_env.py:432-490).  Zero-padded rows
    land in patch (0, 0) with an all-zero box (a reference quirk that its callers filter by |box| == 0)."""
    P = patch_size
    bb = bboxes.to(torch.int64).cpu()
    B, nb = bb.shape[0], bb.shape[1]
    out = torch.zeros((B, n_vertical, n_horizontal, nb, 4), dtype=torch.long)
    masks = torch.zeros((B, n_vertical, n_horizontal, nb), dtype=torch.bool)
    for b in range(B):
        for k in range(nb):
            x1, y1, x2, y2 = (int(v) for v in bb[b, k])
            # the recursion of the reference visits exactly the grid cells the box touches; cell p spans
            # [p * P, p * P + P - 1] (inclusive) and the next piece starts at (p + 1) * P
            for py in range(y1 // P, y2 // P + 1):
                for px in range(x1 // P, x2 // P + 1):
                    if not (0 <= py < n_vertical and 0 <= px < n_horizontal):
                        continue
                    out[b, py, px, k] = torch.tensor([max(x1, px * P) - px * P, max(y1, py * P) - py * P,
                                                      min(x2, px * P + P - 1) - px * P, min(y2, py * P + P - 1) - py * P])
                    masks[b, py, px, k] = True
    return out.to(bboxes.device), masks.to(bboxes.device)


def detection_targets(bboxes: Tensor, n_vertical: int, n_horizontal: int, patch_size: int) -> List[Tensor]:
    """Full-image targets [n, 5] = (class 0, x1, y1, x2, y2), one entry per (box, patch) piece, in (y, x, box) order
    (general_env.py:546-573)."""
    local, _ = split_bboxes_over_patches(bboxes, n_vertical, n_horizontal, patch_size)
    res = []
    for b in range(local.shape[0]):
        rows = []
        for y in range(n_vertical):
            for x in range(n_horizontal):
                for k in range(local.shape[3]):
                    box = local[b, y, x, k]
                    if int(box.abs().sum()) == 0:
                        continue
                    off = torch.tensor([x, y, x, y], device=box.device) * patch_size
                    rows.append(torch.cat((torch.zeros(1, dtype=box.dtype, device=box.device), box + off)))
        res.append(torch.stack(rows) if rows else torch.zeros((0, 5), dtype=torch.long, device=bboxes.device))
    return res


def patch_bboxes2full_image(outputs: List[List[Optional[Tensor]]], offsets: Tensor,
                            masks: Optional[Tensor] = None) -> List[Optional[Tensor]]:
    """Per-patch predictions (list over images of lists over glimpse steps) -> one tensor of boxes per image in
    full-image coordinates; offsets[i, j] = (x, y) of patch j of image i (src/trainer.py:250-280)."""
    res = []
    for i, per_image in enumerate(outputs):
        kept = []
        for j, boxes in enumerate(per_image):
            if masks is not None and not bool(masks[i, j]):
                continue
            if boxes is None:
                continue
            moved = boxes.clone()
            moved[:, 0:2] += offsets[i, j].to(moved.dtype)
            moved[:, 2:4] += offsets[i, j].to(moved.dtype)
            kept.append(moved)
        res.append(torch.cat(kept) if kept else None)
    return res


def rollout_boxes_to_image(rollout: dict, patch_size: int) -> List[Optional[Tensor]]:
    """``patch_bboxes2full_image(rollout["bboxes"], positions[:, :, [1, 0]] * P, rollout["masks"])`` for the whole
    batch in one launch of the engine (``jn_rollout_boxes_to_image``), from the rollout's device outputs "det_boxes" /
    "det_counts" / "positions" / "masks" — so it also serves ``rollout(..., bbox_lists=False)``.  Only the per-image totals
    come back to the host; the returned tensors are slices of one device buffer (None where an image has no box)."""
    return unpack_boxes(*rollout_boxes_packed(rollout, patch_size))


def unpack_boxes(boxes: Tensor, counts: Tensor) -> List[Optional[Tensor]]:
    """Packed rows [B, Nmax, W] + counts [B] -> the list form (one readback: the counts)."""
    return [boxes[b, :k] if k > 0 else None for b, k in enumerate(counts.tolist())]


def rollout_boxes_packed(rollout: dict, patch_size: int) -> Tuple[Tensor, Tensor]:
    """``rollout_boxes_to_image`` without the readback: rows [B, (S+1)*K, 7] fp32 and int32 counts [B], both on the
    device — the packed form ``merge_boxes_device`` and ``map_50_device`` take."""
    from . import _lib
    from ._lib import check, ptr
    boxes, counts, pos, masks = rollout["det_boxes"], rollout["det_counts"], rollout["positions"], rollout["masks"]
    if boxes is None or counts is None:
        raise ValueError("rollout_boxes_to_image needs a rollout with do_detection=True")
    dev = boxes.device
    B, n, K = boxes.shape[0], boxes.shape[1], boxes.shape[2]
    S = n - 1
    # the rollout hands out [:, :S + 1] slices of its [B, T + 1, ...] buffers: read them in place where the strides say so
    T1 = counts.stride(0) if B > 1 else n
    in_place = (counts.dtype == torch.int32 and pos.dtype == torch.int64 and boxes.dtype == torch.float32
                and counts.stride(1) == 1 and T1 >= n
                and (B == 1 or (boxes.stride(0) == T1 * K * 7 and pos.stride(0) == T1 * 2))
                and boxes[0].is_contiguous() and pos[0].is_contiguous())
    if not in_place:
        boxes, counts, pos, T1 = boxes.float().contiguous(), counts.to(torch.int32).contiguous(), pos.long().contiguous(), n
    m = torch.zeros((B, T1), device=dev, dtype=torch.uint8)
    m[:, :n] = masks
    out = torch.empty((B, n * K, 7), device=dev, dtype=torch.float32)
    totals = torch.empty((B,), device=dev, dtype=torch.int32)
    check(_lib.load_library().jn_rollout_boxes_to_image(ptr(boxes), ptr(counts), ptr(pos), ptr(m), B, T1 - 1, S, K, int(patch_size),
                                                        ptr(out), ptr(totals), _lib.current_stream(dev)),
          "jn_rollout_boxes_to_image")
    return out, totals


def merge_boxes(boxes: Tensor, threshold: int = 2, target: bool = False) -> Tensor:
    """Union of boxes whose edges are within `threshold` px of each other (src/utils.py:198-255): box i opens a group
    (or takes the lowest-numbered group that already contains it) and pulls every later box j with min edge distance
    <= threshold into that group.  Predictions (x1, y1, x2, y2, obj, cls, ...) keep the best obj * cls of the group;
    targets are (cls, x1, y1, x2, y2)."""
    off = 1 if target else 0
    n = len(boxes)
    group_of = [-1] * n                          # the lowest-numbered group that contains box i so far
    groups: List[List[int]] = []
    for i in range(n):
        if group_of[i] < 0:
            group_of[i] = len(groups)
            groups.append([i])
        gi = group_of[i]
        a = boxes[i]
        for j in range(i + 1, n):
            b = boxes[j]
            d = min(abs(float(b[off + 2] - a[off + 0])), abs(float(a[off + 2] - b[off + 0])),
                    abs(float(b[off + 3] - a[off + 1])), abs(float(a[off + 3] - b[off + 1])))
            if d <= threshold:
                groups[gi].append(j)             # (the reference appends duplicates too; min / max ignore them)
                if group_of[j] < 0 or gi < group_of[j]:
                    group_of[j] = gi
    merged = []
    for grp in groups:
        sel = boxes[sorted(set(grp))]
        row = [sel[:, off + 0].min(), sel[:, off + 1].min(), sel[:, off + 2].max(), sel[:, off + 3].max()]
        if target:
            row = [torch.zeros((), dtype=boxes.dtype, device=boxes.device)] + row
        elif boxes.shape[1] > 5:
            row += [(sel[:, 4] * sel[:, 5]).max(), torch.ones((), dtype=boxes.dtype, device=boxes.device)]
        merged.append(torch.stack([torch.as_tensor(v, dtype=boxes.dtype, device=boxes.device) for v in row]))
    return torch.stack(merged)


def merge_boxes_batched(batch: List[Optional[Tensor]], threshold: int = 2, target: bool = False) -> List[Optional[Tensor]]:
    return [None if b is None else merge_boxes(b, threshold, target) for b in batch]


def _iou_matrix(a: Tensor, b: Tensor) -> Tensor:
    lt = torch.maximum(a[:, None, :2], b[None, :, :2])
    rb = torch.minimum(a[:, None, 2:4], b[None, :, 2:4])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area_a[:, None] + area_b[None, :] - inter).clamp(min=1e-12)


def map_50(outputs: List[Optional[Tensor]], targets: List[Tensor], max_det: int = 100) -> float:
    """COCO-protocol AP at IoU 0.5 for the single needle class: per image the `max_det` best predictions are matched
    greedily in score order to the not-yet-matched target of highest IoU (>= 0.5); precision is made monotone and
    sampled at the 101 recall points 0, 0.01, ..., 1."""
    n_gt = sum(len(t) for t in targets)
    if n_gt == 0:
        return 0.0                               # src/trainer.py:205-208
    scores, hits = [], []
    for out, tgt in zip(outputs, targets):
        if out is None or len(out) == 0:
            continue
        out = out.detach().to("cpu", torch.float64)              # host-side bookkeeping on a handful of boxes
        order = torch.argsort(out[:, 4], descending=True, stable=True)[:max_det]
        boxes, sc = out[order, :4], out[order, 4]
        gt = tgt[:, 1:5].detach().to("cpu", torch.float64)
        taken = torch.zeros(len(gt), dtype=torch.bool)
        iou = _iou_matrix(boxes, gt) if len(gt) else torch.zeros((len(boxes), 0), dtype=torch.float64)
        for p in range(len(boxes)):
            best, best_j = 0.5, -1
            for j in range(len(gt)):
                if taken[j]:
                    continue
                if iou[p, j] >= best:
                    best, best_j = float(iou[p, j]), j
            if best_j >= 0:
                taken[best_j] = True
            scores.append(float(sc[p]))
            hits.append(best_j >= 0)
    if not scores:
        return 0.0
    order = sorted(range(len(scores)), key=lambda i: -scores[i])
    tp = torch.tensor([1.0 if hits[i] else 0.0 for i in order], dtype=torch.float64).cumsum(0)
    fp = torch.tensor([0.0 if hits[i] else 1.0 for i in order], dtype=torch.float64).cumsum(0)
    recall = tp / n_gt
    precision = tp / (tp + fp)
    for i in range(len(precision) - 2, -1, -1):
        precision[i] = max(precision[i], precision[i + 1])
    ap = 0.0
    for r in torch.linspace(0, 1, 101, dtype=torch.float64):
        idx = int(torch.searchsorted(recall, r, right=False))
        ap += float(precision[idx]) if idx < len(precision) else 0.0
    return ap / 101.0


def compute_detection_metrics(outputs: List[Optional[Tensor]], targets: List[Tensor]) -> dict:
    """``Trainer.compute_detection_metrics`` (src/trainer.py:188-248): {"map": mAP-50 over the batch}."""
    dev = targets[0].device if len(targets) else torch.device("cpu")
    return {"map": torch.tensor([map_50(outputs, targets)], dtype=torch.float32, device=dev)}


# ---- the same evaluation on the device (csrc/kernels_eval.hip) ---------------------------------------------------------
MAX_EVAL_BOXES = 4096            # JN_EVAL_MAX_BOXES: boxes (or targets) per image the kernels hold in LDS
MAX_EVAL_ENTRIES = 8192          # JN_EVAL_MAX_ENTRIES: (score, hit) slots per average-precision segment
_THRESHOLDS = {}


def _recall_thresholds(device) -> Tensor:
    """The 101 recall points of ``map_50``, computed where the host computes them (torch's CPU linspace is not i * 0.01
    in its upper half) and kept on the device."""
    key = str(device)
    if key not in _THRESHOLDS:
        _THRESHOLDS[key] = torch.linspace(0, 1, 101, dtype=torch.float64).to(device)
    return _THRESHOLDS[key]


def pack_boxes(batch: List[Optional[Tensor]], width: int, device=None) -> Tuple[Tensor, Tensor]:
    """List form (None / [n_i, width]) -> packed fp32 rows [B, max(1, Nmax), width] + int32 counts [B] on the device.
    Integer rows (targets) must stay below 2**24 to be exact in fp32."""
    if device is None:
        device = next((b.device for b in batch if b is not None), torch.device("cpu"))
    dtype = next((b.dtype for b in batch if b is not None), torch.float32)
    rows = [torch.zeros((0, width), device=device, dtype=dtype) if b is None else b.to(device) for b in batch]
    assert all(r.shape[1] == width and r.dtype == dtype for r in rows), [(tuple(r.shape), r.dtype) for r in rows]
    counts = torch.tensor([len(r) for r in rows], dtype=torch.int32).to(device)
    # (one more row of length 1 keeps Nmax >= 1)
    packed = torch.nn.utils.rnn.pad_sequence(rows + [torch.zeros((1, width), device=device, dtype=dtype)], batch_first=True)[:-1]
    if not packed.is_floating_point():
        assert bool((packed.abs() < (1 << 24)).all()), "integer boxes beyond 2**24 are not exact in fp32"
    return packed.to(torch.float32).contiguous(), counts


def merge_boxes_device(boxes: Tensor, counts: Tensor, threshold: float = 2, target: bool = False,
                       return_rounds: bool = False):
    """``merge_boxes`` of every image of a batch in one launch (``jn_merge_boxes``): packed fp32 rows [B, Nmax, W] with
    int32 counts [B] on the device — what ``rollout_boxes_packed`` returns — to merged rows [B, Nmax, Wout] in the
    reference's group order and their counts, without a readback.  W = 7 or 6 (predictions, 6 columns out) or, with
    target, 5 (5 out).  Beyond ``MAX_EVAL_BOXES`` rows per image the kernel does not apply and the images are merged
    by the host function.  return_rounds: also the int32 [B] relaxation rounds the kernel took."""
    from . import _lib
    from ._lib import check, ptr
    assert boxes.dim() == 3 and boxes.dtype == torch.float32 and counts.dtype == torch.int32 and boxes.is_cuda
    boxes, counts = boxes.contiguous(), counts.contiguous()
    B, N, W = boxes.shape
    Wout = 5 if target else 6
    if N > MAX_EVAL_BOXES:
        assert not return_rounds
        return _merge_boxes_host_packed(boxes, counts, threshold, target, Wout)
    out = torch.empty((B, N, Wout), device=boxes.device, dtype=torch.float32)
    out_counts = torch.empty((B,), device=boxes.device, dtype=torch.int32)
    rounds = torch.empty((B,), device=boxes.device, dtype=torch.int32) if return_rounds else None
    check(_lib.load_library().jn_merge_boxes(ptr(boxes), ptr(counts), B, N, W, int(bool(target)), float(threshold), ptr(out),
                                             ptr(out_counts), ptr(rounds), _lib.current_stream(boxes.device)), "jn_merge_boxes")
    return (out, out_counts, rounds) if return_rounds else (out, out_counts)


def _merge_boxes_host_packed(boxes, counts, threshold, target, Wout):
    merged = [merge_boxes(boxes[b, :k], threshold, target) if k > 0 else None for b, k in enumerate(counts.tolist())]
    out = torch.zeros((boxes.shape[0], boxes.shape[1], Wout), device=boxes.device, dtype=torch.float32)
    for b, m in enumerate(merged):
        if m is not None:
            out[b, :len(m)] = m
    return out, torch.tensor([0 if m is None else len(m) for m in merged], dtype=torch.int32).to(boxes.device)


def merge_boxes_batched_device(batch: List[Optional[Tensor]], threshold: float = 2, target: bool = False) -> List[Optional[Tensor]]:
    """``merge_boxes_batched`` through ``merge_boxes_device``: list in, list out, None stays None; integer targets go
    over as fp32 (asserted below 2**24) and come back in their own dtype.  One readback: the merged counts."""
    present = [b for b in batch if b is not None]
    if not present:
        return [None] * len(batch)
    width, dtype = present[0].shape[1], present[0].dtype
    packed, counts = pack_boxes(batch, width)
    out, out_counts = merge_boxes_device(packed, counts, threshold, target)
    if not dtype.is_floating_point:
        out = out.to(dtype)
    return [None if b is None else out[i, :k] for i, (b, k) in enumerate(zip(batch, out_counts.tolist()))]


def _as_packed(x, width: int, device=None) -> Tuple[Tensor, Tensor]:
    return (x[0].contiguous(), x[1].contiguous()) if isinstance(x, tuple) else pack_boxes(list(x), width, device)


def match_detections_device(outputs, targets, max_det: int = 100) -> dict:
    """The per-image half of ``map_50`` (``jn_match_detections``): `outputs` / `targets` in list form or packed
    (rows, counts).  Device tensors: scores f64, hits and sel int32 [B, max_det], n_pred and n_gt int32 [B]."""
    from . import _lib
    from ._lib import check, ptr
    if isinstance(outputs, tuple):
        preds, pcounts = outputs[0].contiguous(), outputs[1].contiguous()
    else:
        outputs = list(outputs)
        width = next((o.shape[1] for o in outputs if o is not None), 7)
        dev = next((o.device for o in outputs if o is not None), None)
        if dev is None:
            dev = targets[1].device if isinstance(targets, tuple) else next(iter(targets)).device
        preds, pcounts = pack_boxes(outputs, width, dev)
    dev = preds.device
    tg, tcounts = _as_packed(targets, 5, dev)
    tg = tg.to(dev)
    B, N, W = preds.shape
    M = tg.shape[1]
    assert tg.shape[0] == B and tg.shape[2] == 5 and preds.dtype == tg.dtype == torch.float32
    res = {"scores": torch.zeros((B, max_det), device=dev, dtype=torch.float64),
           "hits": torch.zeros((B, max_det), device=dev, dtype=torch.int32),
           "sel": torch.zeros((B, max_det), device=dev, dtype=torch.int32),
           "n_pred": torch.zeros((B,), device=dev, dtype=torch.int32), "n_gt": torch.zeros((B,), device=dev, dtype=torch.int32)}
    check(_lib.load_library().jn_match_detections(ptr(preds), ptr(pcounts), B, N, W, ptr(tg), ptr(tcounts.to(dev)), M, int(max_det),
                                                  ptr(res["scores"]), ptr(res["hits"]), ptr(res["sel"]), ptr(res["n_pred"]),
                                                  ptr(res["n_gt"]), _lib.current_stream(dev)), "jn_match_detections")
    return res


def average_precision_device(match: dict, pooled: bool) -> Tensor:
    """``jn_average_precision`` over ``match_detections_device``'s result: f64 [B] (one AP per image) or [1] (pooled)."""
    from . import _lib
    from ._lib import check, ptr
    B, max_det = match["scores"].shape
    dev = match["scores"].device
    thr = _recall_thresholds(dev)
    out = torch.zeros((1 if pooled else B,), device=dev, dtype=torch.float64)
    check(_lib.load_library().jn_average_precision(ptr(match["scores"]), ptr(match["hits"]), ptr(match["n_pred"]), ptr(match["n_gt"]),
                                                   B, max_det, int(bool(pooled)), ptr(thr), thr.numel(), ptr(out),
                                                   _lib.current_stream(dev)), "jn_average_precision")
    return out


def map_50_device(outputs, targets, max_det: int = 100, per_image: bool = False):
    """``map_50`` on the device: one workgroup per image selects and matches, one per segment forms the average precision.
    `outputs` / `targets`: list form as for ``map_50``, or packed (fp32 rows [B, N, W], int32 counts [B]).  Returns the
    pooled value (a float) or, per_image, the list of every image's own ``map_50([out], [tgt])``.  One readback per
    call.  Shapes beyond the kernels' limits (``MAX_EVAL_BOXES`` rows per image, ``MAX_EVAL_ENTRIES`` pooled slots) are
    evaluated by the host function."""
    n_rows = outputs[0].shape[1] if isinstance(outputs, tuple) else max([0] + [len(o) for o in outputs if o is not None])
    n_tgts = targets[0].shape[1] if isinstance(targets, tuple) else max([0] + [len(t) for t in targets])
    B = outputs[0].shape[0] if isinstance(outputs, tuple) else len(outputs)
    if B == 0:
        return [] if per_image else 0.0
    if n_rows > MAX_EVAL_BOXES or n_tgts > MAX_EVAL_BOXES or (not per_image and B * max_det > MAX_EVAL_ENTRIES):
        outs = unpack_boxes(*outputs) if isinstance(outputs, tuple) else list(outputs)
        tgts = [t if t is not None else targets[0][:0, 0] for t in unpack_boxes(*targets)] if isinstance(targets, tuple) else list(targets)
        tgts = [t.reshape(-1, 5) for t in tgts]
        return [map_50([o], [t], max_det) for o, t in zip(outs, tgts)] if per_image else map_50(outs, tgts, max_det)
    ap = average_precision_device(match_detections_device(outputs, targets, max_det), pooled=not per_image)
    return ap.tolist() if per_image else float(ap)


def compute_detection_metrics_device(outputs, targets) -> dict:
    """``compute_detection_metrics`` through ``map_50_device``."""
    dev = targets[1].device if isinstance(targets, tuple) else (targets[0].device if len(targets) else torch.device("cpu"))
    return {"map": torch.tensor([map_50_device(outputs, targets)], dtype=torch.float32, device=dev)}
