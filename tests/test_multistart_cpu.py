"""The host side of the multistart evaluation (``detection.pool_walk_detections``, ``cell_targets``, ``walk_cell_maps``,
``ragged.walk_start_positions``) against the loop-by-loop restatement of the reference in tests/multistart_cases.py.
Boxes compare with ``torch.equal`` (the rule rounds nothing but the fp32 IoU, which decides and is not stored); mAP
values to 1e-12 (both sides call the same fp64 ``map_50``; only the order of the units may differ)."""
from types import SimpleNamespace

import pytest
import torch

from jolineedle_amd import _lib, detection, ragged
from jolineedle_amd.trajectory import NeedleSimpleEnv
from tests import multistart_cases as mc

MAP_BAR = 1e-12
CASES = mc.cases()


def host_pool(pr, n_starts=None):
    count = pr["walk_count"] if n_starts is None else [n_starts] * len(pr["walk_count"])
    return detection.pool_walk_detections(pr["det_boxes"], pr["det_counts"], pr["positions"], pr["walk_tokens"], pr["walk_first"],
                                          count, pr["grid"], pr["M"])


def host_maps(pr, pool):
    tg, tc = detection.cell_targets(pr["rows"], pr["extents"], pr["grid"], mc.P)
    Gh, Gw = pr["grid"]
    cells = torch.zeros((len(pr["rows"]), Gh * Gw), dtype=torch.bool)
    for i, (rows, (gh, gw)) in enumerate(zip(pr["rows"], pr["extents"])):
        for y, x in NeedleSimpleEnv(None, mc.P, rows, height=gh * mc.P, width=gw * mc.P).bbox_patches:
            cells[i, y * Gw + x] = True
    return detection.walk_cell_maps(pool, tg, tc, cells), cells


@pytest.mark.parametrize("name", list(CASES))
def test_host_pool_and_maps_equal_the_reference_loops(name):
    pr = CASES[name]
    pool = host_pool(pr)
    mc.assert_pool_equals_reference(pr, pool)
    (traj, full), cells = host_maps(pr, pool)
    for i in range(len(pr["rows"])):
        ref = mc.ref_image(pr, i)
        print(name, i, "map_traj", ref["map_traj"], traj[i], "map", ref["map"], full[i])
        assert abs(traj[i] - ref["map_traj"]) <= MAP_BAR and abs(full[i] - ref["map"]) <= MAP_BAR
        Gw = pr["grid"][1]
        assert {(c // Gw, c % Gw) for c in cells[i].nonzero().flatten().tolist()} == ref["bbox_patches"]


def test_all_cases_side_by_side_equal_the_reference_loops():
    pr = mc.combine(list(CASES.values()))
    assert pr["grid"] == (4, 5) and len(pr["rows"]) == len(CASES) + 1
    mc.assert_pool_equals_reference(pr, host_pool(pr))


def test_the_cases_decide_what_they_are_meant_to_decide():
    pool = {n: host_pool(p) for n, p in CASES.items()}
    b = pool["same_walk_returns"]
    assert b["stats"][0, 1].tolist() == [4, 2] and b["boxes"][0][1][:, 5].tolist() == [0.25, 0.25]      # the first copies
    b = pool["equal_scores_overlap"]
    assert b["stats"][0, 0].tolist() == [4, 2] and b["boxes"][0][0][:, 5].tolist() == [pytest.approx(0.1), pytest.approx(0.4)]
    b = pool["iou_half_and_three_quarters"]
    assert [b["stats"][0, c].tolist() for c in range(3)] == [[2, 2], [2, 1], [2, 2]]
    b = pool["zero_area_twins"]
    assert b["stats"][0, 0].tolist() == [3, 3]                                                         # NaN suppresses nothing
    b = pool["ignored_token_and_walk"]
    assert b["visited"][0].tolist() == [True, True, False, False] and b["stats"][0, 0].tolist() == [1, 1]
    assert float(b["boxes"][0][0][0, 4]) == pytest.approx(0.9)
    b = pool["visited_without_boxes"]
    assert b["visited"][0].tolist() == [True, True] and len(b["boxes"][0][0]) == 0 and b["stats"][0].tolist() == [[0, 0], [0, 0]]
    b = pool["cap_below_survivors"]
    assert b["stats"][0, 0].tolist() == [7, 6] and len(b["boxes"][0][0]) == 4
    assert b["boxes"][0][0][:, 4].tolist() == [pytest.approx(0.6), pytest.approx(0.5), pytest.approx(0.4), pytest.approx(0.3)]
    b = pool["two_walks_one_cell"]
    assert b["stats"][0, 4].tolist() == [3, 2]                                                         # cell (1, 1) of a 2 x 3 grid
    assert pool["image_without_boxes"]["visited"][0].tolist() == [True, True]


def test_unvisited_target_cell_by_hand():
    """Two target cells, each with one target; the visited one holds one prediction that equals its target, the other was
    never reached.  map_traj: one unit, one target, one true positive: precision 1 at every recall point -> 1.
    map: two targets, one true positive -> the only (recall, precision) point is (1/2, 1); the 101-point rule takes,
    for every recall point r of linspace(0, 1, 101), the precision at the first index with recall >= r, else 0: that is 1
    for r = 0, 0.01, ..., 0.50 — 51 points, r = 0.5 included, because 1/2 >= linspace[50] = 1 - 50 * 0.01 = 0.5 exactly —
    and 0 for the 50 points above.  map = 51 / 101."""
    pr = CASES["unvisited_target_cell"]
    (traj, full), cells = host_maps(pr, host_pool(pr))
    assert cells[0].tolist() == [True, False, True]
    assert traj[0] == 1.0
    assert abs(full[0] - 51 / 101) <= MAP_BAR and full[0] < traj[0]
    ref = mc.ref_image(pr, 0)
    assert ref["map_traj"] == 1.0 and abs(ref["map"] - 51 / 101) <= MAP_BAR and ref["prop_patches_found_traj"] == 0.5


def test_prefix_of_a_two_walk_run_equals_the_one_walk_run():
    pr = CASES["two_images_two_walks"]
    two_k1, one = host_pool(pr, n_starts=1), dict(pr)
    # the K = 1 run: only walk 0 of every image exists at all
    keep = pr["walk_first"]
    one.update(det_boxes=pr["det_boxes"][keep], det_counts=pr["det_counts"][keep], positions=pr["positions"][keep],
               walk_tokens=[pr["walk_tokens"][a] for a in keep], walk_first=list(range(len(keep))), walk_count=[1] * len(keep))
    solo = host_pool(one)
    assert torch.equal(two_k1["visited"], solo["visited"]) and torch.equal(two_k1["stats"], solo["stats"])
    for a, b in zip(two_k1["boxes"], solo["boxes"]):
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))
    mc.assert_pool_equals_reference(pr, two_k1, n_starts=1)
    assert not torch.equal(host_pool(pr)["visited"], two_k1["visited"])               # the second walk adds cells
    assert host_maps(pr, two_k1)[0] == host_maps(one, solo)[0]


def test_cell_targets_equal_local_bboxes_on_random_boxes():
    """200 boxes over 25 images of unequal extent on a 4 x 5 canvas, slivers included: a cell that holds a piece of a box
    below the 5 % area rule (and not its centre) has targets without being a target cell."""
    g = torch.Generator().manual_seed(7)
    rows, extents = [], []
    for i in range(25):
        gh, gw = int(torch.randint(1, 5, (1,), generator=g)), int(torch.randint(1, 6, (1,), generator=g))
        H, W = gh * mc.P, gw * mc.P
        r = []
        for k in range(8):
            x1, y1 = int(torch.randint(0, W - 1, (1,), generator=g)), int(torch.randint(0, H - 1, (1,), generator=g))
            if k % 3 == 0 and x1 // mc.P + 1 < gw:          # a sliver: 1 - 3 px into the next column of cells
                x1 = (x1 // mc.P + 1) * mc.P - int(torch.randint(10, 40, (1,), generator=g))
                x2 = (x1 // mc.P + 1) * mc.P + int(torch.randint(1, 4, (1,), generator=g))
            else:
                x2 = int(torch.randint(x1 + 1, min(W, x1 + 150) + 1, (1,), generator=g))
            y2 = int(torch.randint(y1 + 1, min(H, y1 + 150) + 1, (1,), generator=g))
            r.append([x1, y1, x2, y2])
        rows.append(torch.tensor(r)), extents.append((gh, gw))
    tg, tc = detection.cell_targets(rows, extents, (4, 5), mc.P)
    assert tg.shape == (25, 20, 8, 5) and tg.dtype == torch.float32 and tc.dtype == torch.int32
    slivers = total = 0
    for i, (r, (gh, gw)) in enumerate(zip(rows, extents)):
        env = NeedleSimpleEnv(None, mc.P, r, height=gh * mc.P, width=gw * mc.P)
        for y in range(4):
            for x in range(5):
                c, n = y * 5 + x, int(tc[i, y * 5 + x])
                if y >= gh or x >= gw:
                    assert n == 0
                    continue
                loc = torch.from_numpy(env.local_bboxes((y, x)))
                want = loc[loc[:, -1] == 1][:, :5]
                assert n == len(want) and torch.equal(tg[i, c, :n], want), (i, y, x)
                assert not bool(tg[i, c, n:].any())
                total += n
                slivers += n > 0 and (y, x) not in env.bbox_patches
    print("pieces", total, "cells with targets that are no target cells", slivers)
    assert total > 250 and slivers > 10
    assert detection.cell_targets([torch.zeros((0, 4), dtype=torch.long)], [(1, 1)], (2, 2), mc.P)[1].tolist() == [[0, 0, 0, 0]]


def test_walk_start_positions_of_the_three_modes():
    tr = SimpleNamespace(seed=3)
    extents, indices, first, K = [(2, 3), (4, 5), (1, 1)], [4, 5, 6], 11, 3
    multi = ragged.walk_start_positions(tr, first, indices, extents, K, "multistart")
    assert multi.shape == (3, K, 2) and multi.dtype == torch.int64
    for j, (i, e) in enumerate(zip(indices, extents)):
        for k in range(K):             # walk (i, k) is rollout number first + i * K + k of the per-image loop
            assert torch.equal(multi[j, k], ragged.loop_start_positions(tr, first, [i * K + k], [e])[0])
            assert torch.equal(multi[j, k], ragged.loop_start_positions(tr, first + i * K + k, [0], [e])[0])
    assert len({tuple(p) for p in multi[1].tolist()}) > 1                       # the walks of an image differ
    roll = ragged.walk_start_positions(tr, first, indices, extents, K, "rollouts")
    assert torch.equal(roll, multi[:, :1].repeat(1, K, 1))
    corners = ragged.walk_start_positions(tr, first, indices, extents, 4, "corners")
    assert corners.tolist() == [[[0, 0], [1, 0], [1, 2], [0, 2]], [[0, 0], [3, 0], [3, 4], [0, 4]], [[0, 0]] * 4]
    with pytest.raises(AssertionError):
        ragged.walk_start_positions(tr, first, indices, extents, 2, "corners")
    with pytest.raises(ValueError):
        ragged.walk_start_positions(tr, first, indices, extents, 2, "spiral")
    # the last walk of n images is rollout first - 1 + n * K: where the trainer's counter ends
    n = 7
    last = ragged.walk_start_positions(tr, first, list(range(n)), [(4, 5)] * n, K, "multistart")[-1, -1]
    assert torch.equal(last, ragged.loop_start_positions(tr, first - 1 + n * K, [0], [(4, 5)])[0])


def test_nms_pool_equals_the_scalar_rule_on_random_pools():
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 17, 64):
        xy = torch.rand((n, 2), generator=g) * 40
        wh = torch.rand((n, 2), generator=g) * 30
        score = torch.randint(1, 6, (n, 1), generator=g).float() / 5                 # many ties
        pool = torch.cat((xy, xy + wh, score, torch.ones((n, 1)), torch.zeros((n, 1))), 1)
        assert detection.nms_pool(pool) == mc.ref_nms(pool), n


def test_new_entry_points_refuse_bad_shapes_before_any_launch():
    lib = _lib.load_library()
    p = _lib.ptr(torch.zeros(8))
    args = lambda **kw: [kw.get(k, d) for k, d in (("A", 1), ("T", 0), ("S", 0), ("K", 8), ("NI", 1), ("W", 1), ("Gh", 1), ("Gw", 1), ("M", 4))]
    call = lambda ptrs=p, **kw: lib.jn_pool_walk_detections(*([ptrs] * 6), *args(**kw), p if ptrs else None, p if ptrs else None, None,
                                                            p if ptrs else None, None)
    assert call(ptrs=None) == -1 and b"jn_pool_walk_detections" in lib.jn_last_error()
    assert call(M=0) == -1 and call(NI=0) == -1
    assert call(K=4097) == -1
    msg = lib.jn_last_error()
    assert b"jn_pool_walk_detections" in msg and b"4097" in msg and b"4096" in msg
    assert call(W=2, S=7, T=7, K=257) == -1 and b"4112" in lib.jn_last_error()                       # 2 x 8 x 257
    seg = lambda U=4, det=100, NS=1, units=4, thr=101: lib.jn_average_precision_segments(p, p, p, p, U, det, p, NS, units, p, thr, p, None)
    assert lib.jn_average_precision_segments(None, None, None, None, 4, 100, None, 1, 4, None, 101, None, None) == -1
    assert b"jn_average_precision_segments" in lib.jn_last_error()
    assert seg(units=83) == -1 and b"8300" in lib.jn_last_error()                                  # 83 x 100 slots > 8192
    assert seg(thr=257) == -1 and seg(NS=0) == -1
    assert lib.jn_average_precision(p, p, p, p, 83, 100, 1, p, 101, p, None) == -1 and b"8300" in lib.jn_last_error()   # as before
