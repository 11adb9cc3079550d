"""The multistart evaluation restated loop by loop from the reference (``metrics_from_multiple_samples`` and
``eval_missing_patches``, src/supervised.py:485-636) with sets, dicts and Python lists as it is written there, and the
small cases that the CPU and the GPU tests hold ``jolineedle_amd.detection`` and ``jn_pool_walk_detections`` to.

What is restated here is independent of the code under test except for ``detection.map_50`` (the package's statement of
torchmetrics' mAP-50, pinned by tests/test_detection_eval_cpu.py and the reference's known answers) and
``NeedleSimpleEnv`` (pinned to the reference by tests/golden/g8_trajectories.npz).  The NMS is torchvision's rule
(greedy in score order, suppress at IoU > threshold) in scalar numpy fp32 arithmetic, one rounding per operation, with
the score in column 4 and ties to the lower pool index (DESIGN.md §6 on the reference's column).

A *problem* is what one launch sees: A walks (det_boxes [A, S + 1, K, 7], det_counts, positions, walk_tokens), NI
images (walk_first, walk_count, box rows, grid extents) on one canvas grid, and the cap M."""
import numpy as np
import torch

from jolineedle_amd import detection
from jolineedle_amd.trajectory import NeedleSimpleEnv

P = 64


def ref_nms(boxes: torch.Tensor) -> list:
    """Kept row indices of one pool in score order: scalar fp32, one operation at a time."""
    b = boxes.numpy().astype(np.float32)
    order = sorted(range(len(b)), key=lambda i: (-float(b[i, 4]), i))
    dead, keep = set(), []
    f = np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, i in enumerate(order):
            if i in dead:
                continue
            keep.append(i)
            area_i = f(f(b[i, 2] - b[i, 0]) * f(b[i, 3] - b[i, 1]))
            for j in order[n + 1:]:
                if j in dead:
                    continue
                w = max(f(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])), f(0))
                h = max(f(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1])), f(0))
                inter = f(w * h)
                area_j = f(f(b[j, 2] - b[j, 0]) * f(b[j, 3] - b[j, 1]))
                iou = f(inter / f(f(area_i + area_j) - inter))
                if iou > f(0.5):                           # a NaN compares false
                    dead.add(j)
    return keep


def ref_image(pr: dict, i: int, n_starts: int = None) -> dict:
    """One image of a problem as the reference evaluates it: `samples` are its used walks, a sample's valid tokens
    (``masks == 1``) are its first walk_tokens; visited is a SET of positions, predicted a dict of lists."""
    Gh, Gw = pr["grid"]
    w0 = pr["walk_first"][i]
    nw = pr["walk_count"][i] if n_starts is None else n_starts
    A = pr["det_boxes"].shape[0]
    walks = [a for a in range(w0, w0 + nw) if 0 <= a < A]
    visited, predicted = set(), {}
    for a in walks:
        for t in range(pr["walk_tokens"][a]):
            pos = tuple(int(v) for v in pr["positions"][a, t])
            visited.add(pos)
            n = int(pr["det_counts"][a, t])
            if n == 0:
                continue                                   # the rollout's bboxes entry is None
            predicted.setdefault(pos, []).append(pr["det_boxes"][a, t, :n])
    cells = {}
    stats = {}
    for pos in visited:
        if pos not in predicted:
            cells[pos], stats[pos] = torch.zeros((0, 7)), (0, 0)
            continue
        pool = torch.cat(predicted[pos], dim=0)
        kept = pool[ref_nms(pool)]
        cells[pos], stats[pos] = kept[:pr["M"]], (len(pool), len(kept))
    gh, gw = pr["extents"][i]
    env = NeedleSimpleEnv(None, P, pr["rows"][i], height=gh * P, width=gw * P)

    def targets(pos):
        loc = torch.from_numpy(env.local_bboxes(pos))
        return loc[loc[:, -1] == 1][:, :5]
    order = sorted(visited)                                # (the reference iterates a set; any order scores the same)
    outs = [cells[p] if len(cells[p]) else None for p in order]
    tgts = [targets(p) for p in order]
    missed = sorted(env.bbox_patches - visited)
    return {"visited": visited, "cells": cells, "stats": stats,
            "map_traj": detection.map_50(outs, tgts),
            "map": detection.map_50([None] * len(missed) + outs, [targets(p) for p in missed] + tgts),
            "prop_patches_found_traj": len(visited & env.bbox_patches) / len(env.bbox_patches) if env.bbox_patches else 0.0,
            "bbox_patches": env.bbox_patches}


# ---- building problems ------------------------------------------------------------------------------------------------
def box(x1, y1, x2, y2, score, cls=1.0):
    return [float(x1), float(y1), float(x2), float(y2), float(score), float(cls), 0.0]


def make_problem(walks, images, grid, M, S=None, K=None):
    """walks: list of {"tokens": [((y, x), [box rows]) ...], "own": n tokens the walk owns (default all)};
    images: list of {"first", "count", "rows" [n, 4], "extent" (gh, gw)}.  Rows past a count are NaN."""
    S1 = max(len(w["tokens"]) for w in walks) if S is None else S + 1
    Kd = max([1] + [len(b) for w in walks for _, b in w["tokens"]]) if K is None else K
    A = len(walks)
    det = torch.full((A, S1, Kd, 7), float("nan"))
    cnt = torch.zeros((A, S1), dtype=torch.int32)
    pos = torch.zeros((A, S1, 2), dtype=torch.int64)
    for a, w in enumerate(walks):
        for t, (p, rows) in enumerate(w["tokens"]):
            pos[a, t] = torch.tensor(p)
            cnt[a, t] = len(rows)
            if rows:
                det[a, t, :len(rows)] = torch.tensor(rows, dtype=torch.float32)
        pos[a, len(w["tokens"]):] = pos[a, len(w["tokens"]) - 1]
    return {"det_boxes": det, "det_counts": cnt, "positions": pos,
            "walk_tokens": [w.get("own", len(w["tokens"])) for w in walks],
            "walk_first": [im["first"] for im in images], "walk_count": [im["count"] for im in images],
            "rows": [torch.tensor(im["rows"], dtype=torch.long).reshape(-1, 4) for im in images],
            "extents": [tuple(im["extent"]) for im in images], "grid": tuple(grid), "M": int(M)}


def cases() -> dict:
    """name -> problem; every problem is tiny (grids <= 4 x 5, K <= 4 walks, S <= 6, K_det <= 8)."""
    c = {}
    A4, A3, A2 = (0, 0, 4, 4), (0, 0, 4, 3), (0, 0, 4, 2)        # IoU(A4, A3) = 12 / 16 = 3/4, IoU(A4, A2) = 8 / 16 = 1/2 exactly
    far = (20, 20, 30, 31)
    c["one_walk_once"] = make_problem(
        [{"tokens": [((0, 0), [box(*far, 0.9), box(1, 1, 9, 9, 0.4)]), ((0, 1), []), ((1, 1), [box(5, 5, 25, 25, 0.7)])]}],
        [{"first": 0, "count": 1, "rows": [[70, 70, 90, 90]], "extent": (2, 3)}], (2, 3), 8)
    c["two_walks_one_cell"] = make_problem(
        [{"tokens": [((0, 0), []), ((1, 1), [box(5, 5, 25, 25, 0.7)])]},
         {"tokens": [((1, 2), []), ((1, 1), [box(6, 5, 25, 25, 0.8), box(40, 40, 50, 50, 0.6)])]}],
        [{"first": 0, "count": 2, "rows": [[70, 70, 90, 90]], "extent": (2, 3)}], (2, 3), 8)
    # the walk returns to (0, 1): its boxes enter the pool twice, IoU 1 with themselves, the lower pool index survives;
    # column 5 tells the two copies apart
    c["same_walk_returns"] = make_problem(
        [{"tokens": [((0, 1), [box(*far, 0.9, cls=0.25), box(2, 2, 12, 12, 0.5, cls=0.25)]), ((0, 0), []),
                     ((0, 1), [box(*far, 0.9, cls=0.75), box(2, 2, 12, 12, 0.5, cls=0.75)])]}],
        [{"first": 0, "count": 1, "rows": [[80, 10, 100, 30]], "extent": (1, 2)}], (1, 2), 8)
    c["equal_scores_overlap"] = make_problem(
        [{"tokens": [((0, 0), [box(0, 0, 10, 10, 0.5, cls=0.1), box(1, 0, 10, 10, 0.5, cls=0.2), box(0, 0, 10, 9, 0.5, cls=0.3),
                               box(30, 30, 40, 40, 0.5, cls=0.4)])]}],
        [{"first": 0, "count": 1, "rows": [[0, 0, 10, 10]], "extent": (1, 1)}], (1, 1), 8)
    c["iou_half_and_three_quarters"] = make_problem(
        [{"tokens": [((0, 0), [box(*A4, 0.9), box(*A2, 0.8)]),                            # 1/2: both kept
                     ((0, 1), [box(*A4, 0.9), box(*A3, 0.8)]),                            # 3/4: one kept
                     ((1, 0), [box(*A2, 0.9), box(*A4, 0.8)])]}],                         # 1/2 the other way round
        [{"first": 0, "count": 1, "rows": [[0, 0, 4, 4]], "extent": (2, 2)}], (2, 2), 8)
    c["zero_area_twins"] = make_problem(
        [{"tokens": [((0, 0), [box(5, 5, 5, 5, 0.9), box(5, 5, 5, 5, 0.8), box(5, 5, 5, 9, 0.7)])]}],
        [{"first": 0, "count": 1, "rows": [[1, 1, 9, 9]], "extent": (1, 1)}], (1, 1), 8)
    # token 2 of walk 0 lies beyond the walk's own tokens, walk 1 belongs to no image: their boxes and cells are ignored
    c["ignored_token_and_walk"] = make_problem(
        [{"tokens": [((0, 0), [box(0, 0, 10, 10, 0.9)]), ((0, 1), []), ((1, 1), [box(0, 0, 10, 10, 0.95)])], "own": 2},
         {"tokens": [((0, 0), [box(0, 0, 10, 10, 0.99)]), ((1, 0), [box(3, 3, 9, 9, 0.5)]), ((1, 0), [])]}],
        [{"first": 0, "count": 1, "rows": [[0, 0, 10, 10], [70, 70, 100, 100]], "extent": (2, 2)}], (2, 2), 8)
    c["visited_without_boxes"] = make_problem(
        [{"tokens": [((0, 0), []), ((0, 1), []), ((0, 0), [])]}],
        [{"first": 0, "count": 1, "rows": [[10, 10, 30, 30]], "extent": (1, 2)}], (1, 2), 8)
    c["cap_below_survivors"] = make_problem(
        [{"tokens": [((0, 0), [box(10 * k, 0, 10 * k + 8, 8, 0.1 * (k + 1)) for k in range(6)] + [box(0, 0, 8, 7, 0.05)])]}],
        [{"first": 0, "count": 1, "rows": [[0, 0, 8, 8]], "extent": (1, 1)}], (1, 1), 4)
    c["image_without_boxes"] = make_problem(
        [{"tokens": [((0, 0), [box(0, 0, 10, 10, 0.9)]), ((1, 0), [])]}],
        [{"first": 0, "count": 1, "rows": [], "extent": (2, 1)}], (2, 1), 8)
    # two target cells, (0, 0) visited with a perfect prediction, (0, 2) never reached: map_traj = 1, map = 51 / 101
    c["unvisited_target_cell"] = make_problem(
        [{"tokens": [((0, 0), [box(10, 10, 40, 40, 0.9)]), ((0, 1), [])]}],
        [{"first": 0, "count": 1, "rows": [[10, 10, 40, 40], [140, 10, 180, 50]], "extent": (1, 3)}], (1, 3), 8)
    # two images of unequal extent on one canvas, K = 2 walks each, one walk shared cells with the other
    c["two_images_two_walks"] = make_problem(
        [{"tokens": [((0, 0), [box(1, 1, 30, 30, 0.9)]), ((1, 1), [box(6, 6, 26, 26, 0.6)]), ((2, 2), [])]},
         {"tokens": [((3, 4), []), ((2, 3), [box(0, 0, 5, 5, 0.3)]), ((1, 1), [box(5, 5, 25, 25, 0.7), box(6, 6, 26, 26, 0.65)])]},
         {"tokens": [((0, 0), [box(2, 2, 20, 20, 0.8)]), ((0, 1), [box(0, 0, 64, 64, 0.2)])]},
         {"tokens": [((1, 1), [box(3, 3, 33, 33, 0.5)]), ((0, 1), [box(0, 0, 63, 63, 0.4)]), ((0, 0), [box(2, 2, 20, 21, 0.85)])]}],
        [{"first": 0, "count": 2, "rows": [[65, 65, 100, 100], [0, 0, 31, 31], [200, 150, 300, 250]], "extent": (4, 5)},
         {"first": 2, "count": 2, "rows": [[2, 2, 20, 20], [60, 0, 128, 64]], "extent": (2, 2)}], (4, 5), 8)
    return c


def combine(problems: list) -> dict:
    """Several problems side by side as ONE: the walks concatenated, the images with shifted walk_first, one canvas grid
    (the largest), the smallest cap; rows past a count stay NaN."""
    S1 = max(p["det_boxes"].shape[1] for p in problems)
    Kd = max(p["det_boxes"].shape[2] for p in problems)
    out = {"det_boxes": [], "det_counts": [], "positions": [], "walk_tokens": [], "walk_first": [], "walk_count": [], "rows": [],
           "extents": [], "grid": (max(p["grid"][0] for p in problems), max(p["grid"][1] for p in problems)),
           "M": min(p["M"] for p in problems)}
    base = 0
    for p in problems:
        A, s1, kd = p["det_boxes"].shape[:3]
        det = torch.full((A, S1, Kd, 7), float("nan"))
        det[:, :s1, :kd] = p["det_boxes"]
        cnt = torch.zeros((A, S1), dtype=torch.int32)
        cnt[:, :s1] = p["det_counts"]
        pos = torch.zeros((A, S1, 2), dtype=torch.int64)
        pos[:, :s1] = p["positions"]
        out["det_boxes"].append(det), out["det_counts"].append(cnt), out["positions"].append(pos)
        out["walk_tokens"] += p["walk_tokens"]
        out["walk_first"] += [f + base for f in p["walk_first"]]
        out["walk_count"] += p["walk_count"]
        out["rows"] += p["rows"]
        out["extents"] += p["extents"]
        base += A
    for k in ("det_boxes", "det_counts", "positions"):
        out[k] = torch.cat(out[k])
    return out


def assert_pool_equals_reference(pr: dict, pool: dict, n_starts: int = None):
    """`pool` in ``detection.pool_walk_detections``' list form against ``ref_image`` of every image of the problem."""
    Gh, Gw = pr["grid"]
    for i in range(len(pr["walk_first"])):
        ref = ref_image(pr, i, n_starts)
        vis = {(c // Gw, c % Gw) for c in range(Gh * Gw) if bool(pool["visited"][i, c])}
        assert vis == ref["visited"], (i, vis, ref["visited"])
        for c in range(Gh * Gw):
            pos = (c // Gw, c % Gw)
            got = pool["boxes"][i][c]
            if pos not in ref["visited"]:
                assert got is None and pool["stats"][i, c].tolist() == [0, 0], (i, pos)
                continue
            assert got is not None and got.shape == ref["cells"][pos].shape, (i, pos, got, ref["cells"][pos])
            assert torch.equal(got, ref["cells"][pos]), (i, pos, got, ref["cells"][pos])
            assert tuple(pool["stats"][i, c].tolist()) == ref["stats"][pos], (i, pos)


def unpack_device_pool(pool: dict) -> dict:
    """``pool_walk_detections_device``'s tensors in the host function's list form (unvisited: None)."""
    boxes, counts, vis = pool["boxes"].cpu(), pool["counts"].cpu(), pool["visited"].cpu()
    cells = [[boxes[i, c, :int(counts[i, c])] if bool(vis[i, c]) else None for c in range(boxes.shape[1])]
             for i in range(boxes.shape[0])]
    return {"boxes": cells, "visited": vis, "stats": pool["stats"].cpu(), "counts": counts}
