"""Inputs shared by tests/test_teacher_walks_cpu.py and tests/test_gpu_teacher_walks.py (``trajectory.teacher_walks`` and its
device twin ``jn_teacher_walks``).  Every case is small; ``CASES`` maps a name to the arguments of ``teacher_walks``."""
import torch

# boxes of tests/golden/make_golden_trajectories.py (P = 4)
TWO_BOXES = [[13, 2, 18, 9], [25, 25, 31, 31]]
TIE_BOXES = [[0, 12, 3, 15], [24, 12, 27, 15], [12, 0, 15, 3], [12, 24, 15, 27]]       # four cells at distance 3 of (3, 3)
CORNERS = [[0, 0, 3, 3], [28, 28, 31, 31], [0, 28, 3, 31]]


def _case(boxes, gh, gw, P, T, kmin=0, kmax=0, binomial=False, seed=0, starts=None):
    """boxes: one list of xyxy rows per image (padded here with zero rows to the longest), or a ready [B, nb, 4] tensor."""
    if not isinstance(boxes, torch.Tensor):
        nb = max((len(b) for b in boxes), default=0)
        t = torch.zeros((len(boxes), nb, 4), dtype=torch.int64)
        for i, rows in enumerate(boxes):
            for j, r in enumerate(rows):
                t[i, j] = torch.tensor(r)
        boxes = t
    return dict(bboxes=boxes, gh=gh, gw=gw, P=P, T=T, min_keypoints=kmin, max_keypoints=kmax, binomial_keypoints=binomial,
                seed=seed, start_positions=None if starts is None else torch.tensor(starts, dtype=torch.int64).reshape(-1, 2))


Z = [0, 0, 0, 0]
CASES = {
    # no empty cell (no negative); the one keypoint is the agent's own cell: the STOP replacement is drawn
    "grid_1x1": _case([[[1, 1, 3, 3]]], 1, 1, 4, 4, seed=3),
    "grid_1x1_no_box": _case(torch.zeros((2, 0, 4), dtype=torch.int64), 1, 1, 4, 3, kmax=2, seed=4),
    "grid_1x5": _case([[[9, 0, 18, 3]], [[17, 1, 19, 2]]], 1, 5, 4, 9, kmax=1, seed=5),
    "grid_5x1": _case([[[0, 9, 3, 18]], [[1, 1, 2, 2]]], 5, 1, 4, 9, kmax=1, seed=6),
    "grid_8x8": _case([TWO_BOXES, CORNERS], 8, 8, 4, 40, kmin=1, kmax=3, seed=7),
    "grid_8x8_binomial": _case([TWO_BOXES, CORNERS], 8, 8, 4, 40, kmin=1, kmax=3, binomial=True, seed=8),
    # 40 columns: two draws per binomial in x, one in y
    "grid_3x40_binomial": _case([[[30, 2, 61, 9], [140, 5, 150, 11]], [[80, 0, 83, 3]]], 3, 40, 4, 64, kmin=2, kmax=4,
                                binomial=True, seed=9),
    "boxes_outside": _case([[[12, 12, 19, 18]], [[100, 100, 120, 120]], [[-6, -3, 5, 6]], [[-20, -20, -10, -10]],
                            [[-9, 5, 40, 6]]], 4, 4, 4, 10, kmax=1, seed=10),
    # P = 20: cell (0, 0) holds 4 x 5 = 20 px of image 0's box, exactly 1 / 20 of a patch: no target; 7 x 3 = 21 px is one
    "area_exactly_a_twentieth": _case([[[16, 0, 60, 5]], [[13, 0, 60, 3]]], 2, 4, 20, 8, seed=11),
    "zero_area": _case([[[5, 5, 5, 5]], [[9, 2, 9, 14]]], 4, 4, 4, 8, kmax=1, seed=12),
    "no_boxes": _case(torch.zeros((2, 0, 4), dtype=torch.int64), 4, 4, 4, 8, kmax=2, seed=13),
    "zero_row_padding": _case([[Z, [1, 1, 7, 3], Z, [18, 14, 27, 23], Z], [[1, 1, 7, 3], [18, 14, 27, 23], Z, Z, Z]],
                              6, 7, 4, 24, kmax=2, seed=14),
    "ties_8x8": _case([TIE_BOXES, TIE_BOXES], 8, 8, 4, 40, seed=15, starts=[[3, 3], [3, 3]]),
    "T_1": _case([CORNERS], 8, 8, 4, 1, kmax=1, seed=16),
    "ring_wrap": _case([CORNERS, TWO_BOXES], 8, 8, 4, 6, kmax=1, seed=17, starts=[[4, 4], [7, 0]]),
    "zero_tail": _case([[[9, 5, 14, 11]]], 5, 6, 4, 30, seed=18, starts=[[0, 0]]),
    "no_detours": _case([TWO_BOXES], 8, 8, 4, 40, kmin=0, kmax=0, seed=19),
    # three detours; with this seed one of them lands on a keypoint still to come (asserted by the CPU test)
    "three_detours": _case([[[4, 4, 19, 19]]], 6, 6, 4, 64, kmin=3, kmax=3, seed=20),
    "start_inside_a_box": _case([[[10, 9, 30, 20]]], 4, 5, 8, 16, kmax=1, seed=21, starts=[[1, 2]]),
    "start_outside_a_box": _case([[[10, 9, 30, 20]]], 4, 5, 8, 16, kmax=1, seed=22, starts=[[3, 0]]),
    "three_images": _case([[[1, 1, 7, 3], [18, 14, 27, 23]], [Z, Z], [Z, [9, 5, 14, 11]]], 6, 7, 4, 12, kmax=2, seed=23),
    # the largest grid the kernel takes: 4096 cells
    "grid_64x64": _case([[[40, 70, 47, 75]]], 64, 64, 2, 8, kmax=1, seed=24),
}
