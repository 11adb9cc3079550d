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
from typing import List, Optional, Sequence, Tuple

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


MAX_DETECTION_CELLS = 4096       # JN_DETCELLS_MAX_CELLS: cells per image the select kernel lists in LDS
_NEG_TAG = 0x4E454753            # third Philox counter word of the negative draws


def detection_cells(bboxes: Tensor, gh: int, gw: int, P: int, sample_neg: int, seed: int,
                    extents=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The cells and targets of ``NeedleGeneralEnv.get_detection_batch`` (src/env/general_env.py:506-546) for a whole
    batch, on the host in numpy — the statement of the rule ``jn_detection_cells`` computes (include/jnroll.h) and the
    comparand of ``detection_cells_device``.  bboxes [B, nb, 4] xyxy (zero rows = padding) on a grid of gh x gw cells
    of P px; extents [B, 2] = (gh_i, gw_i): image i owns the top-left gh_i x gw_i cells only.

    Per image, in index order: the cells that hold a piece of a box (``split_bboxes_over_patches``' masks) in
    row-major order, then min(sample_neg, n_empty) of its empty cells by a partial Fisher-Yates shuffle of their
    row-major list E: draw j swaps E[j] with E[j + r mod (n_empty - j)], r = Philox4x32-10(seed; image, j, 0x4e454753,
    0).x, and emits E[j] — a function of (seed, image index) alone.  (The reference draws with ``torch.randperm``.)

    Returns on the CPU: cells int64 [n, 3] = (image, y, x), targets int64 [n, nb, 5] = (0, x1, y1, x2, y2) patch-local
    (zero rows for the boxes that do not touch the cell), offsets int32 [B + 1] (row offsets[i] is image i's first,
    offsets[B] = n) and n_pos int32 [B]."""
    import numpy as np
    from .ragged import _philox4x32
    gh, gw, P, sample_neg = int(gh), int(gw), int(P), int(sample_neg)
    bb = np.asarray(bboxes.detach().cpu() if isinstance(bboxes, Tensor) else bboxes, dtype=np.int64)
    assert bb.ndim == 3 and bb.shape[2] == 4 and bb.shape[1] >= 1 and P >= 1 and sample_neg >= 0 and gh >= 1 and gw >= 1
    B, nb = bb.shape[0], bb.shape[1]
    if extents is None:
        ext = np.tile(np.array([[gh, gw]], np.int64), (B, 1))
    else:
        ext = np.asarray(extents.cpu() if isinstance(extents, Tensor) else extents, dtype=np.int64).reshape(B, 2)
        assert ((ext >= 1) & (ext <= np.array([gh, gw]))).all(), "an extent outside the grid"
    x1, y1, x2, y2 = (bb[:, :, k, None] for k in range(4))                               # [B, nb, 1]
    ys, xs = np.arange(gh, dtype=np.int64)[None, None, :], np.arange(gw, dtype=np.int64)[None, None, :]
    in_y = (y1 // P <= ys) & (ys <= y2 // P) & (ys < ext[:, None, 0:1])                  # [B, nb, gh] (numpy's // floors)
    in_x = (x1 // P <= xs) & (xs <= x2 // P) & (xs < ext[:, None, 1:2])                  # [B, nb, gw]
    touch = (in_y[:, :, :, None] & in_x[:, :, None, :]).transpose(0, 2, 3, 1)            # [B, gh, gw, nb]
    ly1, ly2 = np.maximum(y1, ys * P) - ys * P, np.minimum(y2, ys * P + P - 1) - ys * P  # [B, nb, gh]
    lx1, lx2 = np.maximum(x1, xs * P) - xs * P, np.minimum(x2, xs * P + P - 1) - xs * P  # [B, nb, gw]
    local = np.zeros((B, gh, gw, nb, 5), np.int64)
    local[..., 1] = lx1.transpose(0, 2, 1)[:, None, :, :]
    local[..., 2] = ly1.transpose(0, 2, 1)[:, :, None, :]
    local[..., 3] = lx2.transpose(0, 2, 1)[:, None, :, :]
    local[..., 4] = ly2.transpose(0, 2, 1)[:, :, None, :]
    local *= touch[..., None]
    positive = touch.any(-1)                                                             # [B, gh, gw]
    exists = (np.arange(gh)[None, :, None] < ext[:, 0, None, None]) & (np.arange(gw)[None, None, :] < ext[:, 1, None, None])
    cells, offsets, n_pos = [], [0], []
    for i in range(B):
        pos = np.argwhere(positive[i])                                                   # row-major
        E = [tuple(c) for c in np.argwhere(exists[i] & ~positive[i])]
        k = min(sample_neg, len(E))
        for j in range(k):
            o = j + _philox4x32(int(seed), i, j, _NEG_TAG, 0)[0] % (len(E) - j)
            E[j], E[o] = E[o], E[j]
        rows = np.concatenate((pos, np.array(E[:k], np.int64).reshape(-1, 2)))
        cells.append(np.concatenate((np.full((len(rows), 1), i, np.int64), rows), 1))
        n_pos.append(len(pos))
        offsets.append(offsets[-1] + len(rows))
    cells = np.concatenate(cells) if cells else np.zeros((0, 3), np.int64)
    targets = local[cells[:, 0], cells[:, 1], cells[:, 2]]
    return (torch.from_numpy(cells), torch.from_numpy(targets), torch.tensor(offsets, dtype=torch.int32),
            torch.tensor(n_pos, dtype=torch.int32))


def detection_cells_device(bboxes: Tensor, gh: int, gw: int, P: int, sample_neg: int, seed: int,
                           extents=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``detection_cells`` on the device (``jn_detection_cells``: three launches, no Python loop): bboxes [B, nb, 4] on
    the GPU; returns (cells, targets, offsets, n_pos) as the host function does, with cells, targets and n_pos on the
    device.  The buffers hold B * gh * gw rows, which always suffices; the B + 1 offsets are read back once — the one
    synchronisation, for n (with `extents` the entry point checks them on the host first, a second one).  A grid beyond
    ``MAX_DETECTION_CELLS`` cells is refused by the entry point."""
    from . import _lib
    from ._lib import check, ptr
    if not bboxes.is_cuda:
        raise RuntimeError("detection_cells_device needs the boxes on the GPU (detection_cells is the host function)")
    dev = bboxes.device
    bb = bboxes.to(torch.int64).contiguous()
    assert bb.dim() == 3 and bb.shape[2] == 4, "bboxes are [B, nb, 4]"
    B, nb = int(bb.shape[0]), int(bb.shape[1])
    gh, gw = int(gh), int(gw)
    ext = None if extents is None else torch.as_tensor(extents).to(dev, torch.int32).reshape(B, 2).contiguous()
    cap = B * gh * gw
    cells = torch.empty((cap, 3), device=dev, dtype=torch.int64)
    targets = torch.empty((cap, max(nb, 1), 5), device=dev, dtype=torch.int64)
    offsets = torch.empty((B + 1,), device=dev, dtype=torch.int32)
    n_pos = torch.empty((B,), device=dev, dtype=torch.int32)
    check(_lib.load_library().jn_detection_cells(ptr(bb), ptr(ext), B, nb, gh, gw, int(P), int(sample_neg),
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, cap, ptr(cells), ptr(targets), ptr(offsets),
                                                 ptr(n_pos), _lib.current_stream(dev)), "jn_detection_cells")
    offsets = offsets.cpu()
    n = int(offsets[B])
    return cells[:n], targets[:n], offsets, n_pos


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


# ---- the multistart evaluation (src/supervised.py:485-636): pool the walks' detections per cell, NMS, mAP per image ------
def nms_pool(boxes: Tensor) -> List[int]:
    """Greedy NMS at IoU 0.5 over one pool [n, >= 5] (``nms(bboxes[:, :4], score, 0.5)``, src/supervised.py:552, 624):
    the rows in (column 4 descending, index ascending) order, a row suppressed when its IoU with a kept row is > 0.5.
    The IoU is fp32, every operation rounded once: w = max(min(x2) - max(x1), 0), likewise h, inter = w * h,
    iou = inter / ((area_a + area_b) - inter); a NaN (two zero-area boxes) suppresses nothing.  Returns the kept row
    indices in that order."""
    n = len(boxes)
    if n == 0:
        return []
    b = boxes.detach().to("cpu", torch.float32)
    order = torch.argsort(b[:, 4], descending=True, stable=True)
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = torch.zeros(n, dtype=torch.bool)
    keep = []
    for p in range(n):
        if dead[p]:
            continue
        keep.append(int(order[p]))
        if p + 1 < n:
            w = (torch.minimum(b[p, 2], b[p + 1:, 2]) - torch.maximum(b[p, 0], b[p + 1:, 0])).clamp(min=0)
            h = (torch.minimum(b[p, 3], b[p + 1:, 3]) - torch.maximum(b[p, 1], b[p + 1:, 1])).clamp(min=0)
            inter = w * h
            dead[p + 1:] |= inter / ((area[p] + area[p + 1:]) - inter) > 0.5
    return keep


def pool_walk_detections(det_boxes: Tensor, det_counts: Tensor, positions: Tensor, walk_tokens: Sequence[int],
                         walk_first: Sequence[int], walk_count: Sequence[int], grid: Tuple[int, int],
                         max_per_cell: int) -> dict:
    """The pooling of ``metrics_from_multiple_samples`` / ``eval_missing_patches`` (src/supervised.py:573-625) on the
    host, and the statement of the rule ``jn_pool_walk_detections`` computes.  det_boxes [A, S + 1, K, 7], det_counts
    [A, S + 1], positions [A, S + 1, 2] (y, x) of A walks; walk a owns its first walk_tokens[a] tokens; image i uses the
    walks walk_first[i] .. walk_first[i] + walk_count[i] - 1.  A cell of the `grid` = (Gh, Gw) is visited when such a
    token stands on it; its pool is the boxes of all those tokens in (walk, token, stored) order — a walk that returns
    to a cell contributes its boxes again — de-duplicated by ``nms_pool`` (score = column 4; DESIGN.md §6 on the
    reference's column) and cut to the first `max_per_cell` survivors.

    Returns {"boxes": per image a list over the Gh * Gw cells of None (not visited) or the survivors [n, 7] fp32 on
    the CPU, "visited": bool [NI, Gh * Gw], "stats": int32 [NI, Gh * Gw, 2] = (pool size, survivors before the cut)}."""
    Gh, Gw = int(grid[0]), int(grid[1])
    boxes, counts, pos = det_boxes.detach().cpu().float(), det_counts.detach().cpu().tolist(), positions.detach().cpu().tolist()
    tokens = [int(v) for v in (walk_tokens.tolist() if isinstance(walk_tokens, Tensor) else walk_tokens)]
    first = [int(v) for v in (walk_first.tolist() if isinstance(walk_first, Tensor) else walk_first)]
    count = [int(v) for v in (walk_count.tolist() if isinstance(walk_count, Tensor) else walk_count)]
    A, n_tok, M = boxes.shape[0], boxes.shape[1], int(max_per_cell)
    assert M >= 1 and len(first) == len(count) >= 1
    out = {"boxes": [], "visited": torch.zeros((len(first), Gh * Gw), dtype=torch.bool),
           "stats": torch.zeros((len(first), Gh * Gw, 2), dtype=torch.int32)}
    for i, (w0, nw) in enumerate(zip(first, count)):
        pools: dict = {}
        for a in range(max(w0, 0), min(w0 + nw, A)):
            for t in range(min(tokens[a], n_tok)):
                y, x = pos[a][t]
                if 0 <= y < Gh and 0 <= x < Gw:
                    pools.setdefault(y * Gw + x, []).append(boxes[a, t, :max(0, min(counts[a][t], boxes.shape[2]))])
        cells: List[Optional[Tensor]] = [None] * (Gh * Gw)
        for c, parts in pools.items():
            pool = torch.cat(parts)
            kept = pool[nms_pool(pool)] if len(pool) else pool
            out["visited"][i, c] = True
            out["stats"][i, c] = torch.tensor([len(pool), len(kept)], dtype=torch.int32)
            cells[c] = kept[:M]
        out["boxes"].append(cells)
    return out


def pool_walk_detections_device(det_boxes: Tensor, det_counts: Tensor, positions: Tensor, walk_tokens: Tensor,
                                walk_first: Tensor, walk_count: Tensor, max_walks: int, grid: Tuple[int, int],
                                max_per_cell: int, stats: bool = True) -> dict:
    """``pool_walk_detections`` of every (image, cell) in one launch (``jn_pool_walk_detections``), without a readback.
    The first three arguments are a rollout's "det_boxes" / "det_counts" / "positions" (read in place where they are
    [:, :S + 1] slices of [A, T + 1, ...] buffers); walk_tokens / walk_first / walk_count int32 on the device; `max_walks`
    is the host's bound on walk_count.  Returns device tensors {"boxes": fp32 [NI, Gh * Gw, M, 7] (rows beyond a count
    are not written), "counts": int32 [NI, Gh * Gw], "stats": int32 [NI, Gh * Gw, 2] or None, "visited": bool
    [NI, Gh * Gw]}.  Beyond ``MAX_EVAL_BOXES`` boxes per pool (max_walks * (S + 1) * K) the kernel does not apply and
    the host function pools."""
    from . import _lib
    from ._lib import check, ptr
    dev = det_boxes.device
    A, n, K = det_boxes.shape[0], det_boxes.shape[1], det_boxes.shape[2]
    S, Gh, Gw, M = n - 1, int(grid[0]), int(grid[1]), int(max_per_cell)
    NI = int(walk_first.numel())
    if int(max_walks) * n * K > MAX_EVAL_BOXES:
        host = pool_walk_detections(det_boxes, det_counts, positions, walk_tokens, walk_first, walk_count, grid, M)
        boxes = torch.zeros((NI, Gh * Gw, M, 7), dtype=torch.float32)
        cnt = torch.zeros((NI, Gh * Gw), dtype=torch.int32)
        for i, cells in enumerate(host["boxes"]):
            for c, rows in enumerate(cells):
                if rows is not None and len(rows):
                    boxes[i, c, :len(rows)], cnt[i, c] = rows, len(rows)
        return {"boxes": boxes.to(dev), "counts": cnt.to(dev), "stats": host["stats"].to(dev) if stats else None,
                "visited": host["visited"].to(dev)}
    T1 = det_counts.stride(0) if A > 1 else n
    in_place = (det_counts.dtype == torch.int32 and positions.dtype == torch.int64 and det_boxes.dtype == torch.float32
                and det_counts.stride(1) == 1 and T1 >= n
                and (A == 1 or (det_boxes.stride(0) == T1 * K * 7 and positions.stride(0) == T1 * 2))
                and det_boxes[0].is_contiguous() and positions[0].is_contiguous())
    if not in_place:
        det_boxes, det_counts, positions, T1 = (det_boxes.float().contiguous(), det_counts.to(torch.int32).contiguous(),
                                                positions.long().contiguous(), n)
    i32 = lambda t: t.to(dev, torch.int32).contiguous()
    walk_tokens, walk_first, walk_count = i32(walk_tokens), i32(walk_first), i32(walk_count)
    assert walk_tokens.numel() == A and walk_count.numel() == NI
    out = {"boxes": torch.empty((NI, Gh * Gw, M, 7), device=dev, dtype=torch.float32),
           "counts": torch.empty((NI, Gh * Gw), device=dev, dtype=torch.int32),
           "stats": torch.empty((NI, Gh * Gw, 2), device=dev, dtype=torch.int32) if stats else None}
    vis = torch.empty((NI, Gh * Gw), device=dev, dtype=torch.uint8)
    check(_lib.load_library().jn_pool_walk_detections(ptr(det_boxes), ptr(det_counts), ptr(positions), ptr(walk_tokens),
                                                      ptr(walk_first), ptr(walk_count), A, T1 - 1, S, K, NI, int(max_walks), Gh, Gw,
                                                      M, ptr(out["boxes"]), ptr(out["counts"]), ptr(out["stats"]), ptr(vis),
                                                      _lib.current_stream(dev)), "jn_pool_walk_detections")
    out["visited"] = vis.bool()
    return out


def cell_targets(bbox_rows: Sequence[Tensor], extents: Sequence[Sequence[int]], canvas_grid: Tuple[int, int],
                 patch_size: int, device=None) -> Tuple[Tensor, Tensor]:
    """Per image and per cell of the canvas grid the targets a patch-level mAP scores against: the rows
    (0, x1, y1, x2, y2) of ``NeedleSimpleEnv.local_bboxes`` (trajectory.py; the part of every box inside the cell,
    patch-local, kept where it is more than a line: strict <) with the objectness-0 rows dropped, in box order.
    bbox_rows[i]: [n_i, 4] xyxy in image i's pixels; extents[i] = (gh, gw), cells outside hold nothing.  Returns fp32
    [NI, Gh * Gw, nb, 5] and int32 counts [NI, Gh * Gw] (torch ops on `device`, once per chunk, without a readback)."""
    Gh, Gw, P = int(canvas_grid[0]), int(canvas_grid[1]), int(patch_size)
    NI = len(bbox_rows)
    nb = max([1] + [int(r.shape[0]) for r in bbox_rows])
    rows = torch.zeros((NI, nb, 4), dtype=torch.int64)
    real = torch.zeros((NI, nb), dtype=torch.bool)
    for i, r in enumerate(bbox_rows):
        rows[i, :r.shape[0]], real[i, :r.shape[0]] = r.to(torch.int64).reshape(-1, 4), True
    ext = torch.as_tensor([[int(e[0]), int(e[1])] for e in extents], dtype=torch.int64).reshape(NI, 2)
    # every coordinate kept below lies in 0 .. P (the part of a box inside its cell), so P bounds what fp32 must hold
    assert P < (1 << 24), "integer boxes beyond 2**24 are not exact in fp32"
    rows, real, ext = rows.to(device), real.to(device), ext.to(device)
    ys = torch.arange(Gh, device=rows.device).repeat_interleave(Gw)                     # cell c = y * Gw + x
    xs = torch.arange(Gw, device=rows.device).repeat(Gh)
    px, py = (xs * P)[None, :, None], (ys * P)[None, :, None]                           # [1, cells, 1]
    x1, y1, x2, y2 = (rows[:, None, :, k] for k in range(4))                             # [NI, 1, nb]
    cx1, cy1 = torch.maximum(px, x1), torch.maximum(py, y1)
    cx2, cy2 = torch.minimum(px + P, x2), torch.minimum(py + P, y2)
    inside = (ys[None, :] < ext[:, None, 0]) & (xs[None, :] < ext[:, None, 1])          # [NI, cells]
    valid = (cx1 < cx2) & (cy1 < cy2) & real[:, None, :] & inside[:, :, None]
    local = torch.stack((torch.zeros_like(cx1), cx1 - px, cy1 - py, cx2 - px, cy2 - py), -1)      # [NI, cells, nb, 5]
    order = torch.argsort((~valid).to(torch.int8), dim=-1, stable=True)                 # the valid rows first, in box order
    local = torch.gather(local, 2, order[..., None].expand(-1, -1, -1, 5))
    counts = valid.sum(-1).to(torch.int32)
    local = local * (torch.arange(nb, device=rows.device)[None, None, :] < counts[..., None])[..., None]
    return local.to(torch.float32).contiguous(), counts.contiguous()


def average_precision_segments_device(match: dict, seg_offsets: Tensor, max_units: int) -> Tensor:
    """``jn_average_precision_segments`` over ``match_detections_device``'s result: f64 [NS], segment s = the units
    seg_offsets[s] .. seg_offsets[s + 1] - 1 (int32 on the device); `max_units` is the host's bound on their number."""
    from . import _lib
    from ._lib import check, ptr
    U, max_det = match["scores"].shape
    dev = match["scores"].device
    thr = _recall_thresholds(dev)
    seg = seg_offsets.to(dev, torch.int32).contiguous()
    NS = seg.numel() - 1
    out = torch.zeros((NS,), device=dev, dtype=torch.float64)
    check(_lib.load_library().jn_average_precision_segments(ptr(match["scores"]), ptr(match["hits"]), ptr(match["n_pred"]),
                                                            ptr(match["n_gt"]), U, max_det, ptr(seg), NS, int(max_units), ptr(thr),
                                                            thr.numel(), ptr(out), _lib.current_stream(dev)),
          "jn_average_precision_segments")
    return out


def map_50_segments(outputs: List[Optional[Tensor]], targets: List[Tensor], seg_offsets: Sequence[int],
                    max_det: int = 100) -> List[float]:
    """Per segment ``map_50`` over the units seg_offsets[s] .. seg_offsets[s + 1] - 1 of the two lists (host)."""
    return [map_50(outputs[a:b], targets[a:b], max_det) for a, b in zip(seg_offsets[:-1], seg_offsets[1:])]


def map_50_segments_device(outputs, targets, seg_offsets: Sequence[int], max_det: int = 100, readback: bool = True):
    """``map_50_segments`` on the device: ``jn_match_detections`` over all units, then ``jn_average_precision_segments``;
    `outputs` / `targets` in list form or packed (fp32 rows [U, N, W] / [U, Mmax, 5] with int32 counts [U]);
    `seg_offsets` host integers.  One readback (none with readback=False: the f64 [NS] device tensor is returned).
    A unit never offers more than its N rows, so min(max_det, N) slots per unit hold every selected prediction; beyond
    ``MAX_EVAL_ENTRIES`` slots per segment or ``MAX_EVAL_BOXES`` rows per unit the host function evaluates."""
    seg = [int(v) for v in seg_offsets]
    n_rows = outputs[0].shape[1] if isinstance(outputs, tuple) else max([0] + [len(o) for o in outputs if o is not None])
    n_tgts = targets[0].shape[1] if isinstance(targets, tuple) else max([0] + [len(t) for t in targets])
    U = outputs[0].shape[0] if isinstance(outputs, tuple) else len(outputs)
    max_units = max([1] + [b - a for a, b in zip(seg[:-1], seg[1:])])
    det = max(1, min(int(max_det), n_rows))
    if len(seg) < 2:
        return [] if readback else torch.zeros((0,), dtype=torch.float64)
    if U == 0 or n_rows > MAX_EVAL_BOXES or n_tgts > MAX_EVAL_BOXES or max_units * det > MAX_EVAL_ENTRIES:
        outs = unpack_boxes(*outputs) if isinstance(outputs, tuple) else list(outputs)
        tgts = ([t if t is not None else targets[0][:0, 0] for t in unpack_boxes(*targets)] if isinstance(targets, tuple)
                else list(targets))
        res = map_50_segments(outs, [t.reshape(-1, 5) for t in tgts], seg, max_det)
        return res if readback else torch.tensor(res, dtype=torch.float64)
    ap = average_precision_segments_device(match_detections_device(outputs, targets, det), torch.tensor(seg, dtype=torch.int32),
                                           max_units)
    return ap.tolist() if readback else ap


def walk_cell_maps(pool: dict, targets: Tensor, target_counts: Tensor, target_cells: Tensor, max_det: int = 100) -> List[List[float]]:
    """The two per-image mAP-50 values of the multistart evaluation from ``pool_walk_detections``' result, on the host:
    [map_traj, map], each a list over the images.  map_traj (``metrics_from_multiple_samples``): one ``map_50`` over the
    image's visited cells, each a unit with its survivors as predictions and its ``cell_targets`` as targets.  map
    (``eval_missing_patches``): the target cells (`target_cells` bool [NI, cells]) that were not visited come first as
    units without predictions.  Cells in row-major order."""
    tg, tc = targets.detach().cpu(), target_counts.detach().cpu().tolist()
    vis, tcell = pool["visited"].cpu().tolist(), target_cells.cpu().tolist()
    traj, full = [], []
    for i, cells in enumerate(pool["boxes"]):
        seen = [c for c in range(len(cells)) if vis[i][c]]
        missed = [c for c in range(len(cells)) if tcell[i][c] and not vis[i][c]]
        outs = [cells[c] if cells[c] is not None and len(cells[c]) else None for c in seen]
        tgts = [tg[i, c, :tc[i][c]] for c in seen]
        traj.append(map_50(outs, tgts, max_det))
        full.append(map_50([None] * len(missed) + outs, [tg[i, c, :tc[i][c]] for c in missed] + tgts, max_det))
    return [traj, full]


def walk_cell_maps_device(pool: dict, targets: Tensor, target_counts: Tensor, target_cells: Tensor, max_det: int = 100) -> Tensor:
    """``walk_cell_maps`` on the device from ``pool_walk_detections_device``'s result: f64 [2, NI] without a readback.
    Per variant one ``jn_match_detections`` over all NI * cells units and one ``jn_average_precision_segments`` with one
    segment per image; a cell that is not counted has its target count zeroed (and, unvisited, holds no prediction), so
    it adds nothing to either side."""
    NI, cells, M, W = pool["boxes"].shape
    dev = pool["boxes"].device
    preds = (pool["boxes"].view(NI * cells, M, W), pool["counts"].view(NI * cells))
    tg = targets.to(dev).view(NI * cells, -1, 5)
    tcounts, vis = target_counts.to(dev), pool["visited"]
    seg = [i * cells for i in range(NI + 1)]
    res = []
    for counted in (vis, vis | target_cells.to(dev)):
        tc = (tcounts * counted.to(torch.int32)).view(NI * cells).contiguous()
        res.append(map_50_segments_device(preds, (tg, tc), seg, max_det, readback=False).to(dev))
    return torch.stack(res)
