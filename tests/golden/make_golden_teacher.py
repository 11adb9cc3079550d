"""Generate tests/golden/g11_teacher_sets.npz: the teacher's action SET of seeded states, recorded from the REFERENCE's
NeedleSimpleEnv (src/env/simple_env.py, imported read-only from the reference tree, ``make_golden.REF``) on CPU.

Run in the build container only:  python tests/golden/make_golden_teacher.py

Per state: `reset(position, visited)`, then `build_keypoints_trajectory()` with the module's `random.choice` replaced by
a recorder that keeps the candidate list of its FIRST call — the nearest remaining target cells N — and the set is
`move_towards(position, q)` over N, one bit per action.  The fixture holds inputs (grid, boxes, position, target and
visited cells) and the sets — no source.
"""
import random
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True

from make_golden import install_stubs, REF  # noqa: E402

P, GMAX, N_RANDOM = 4, 9, 200
TIES = (7, 7, [[0, 12, 3, 15], [24, 12, 27, 15], [12, 0, 15, 3], [12, 24, 15, 27]], (3, 3))      # G8's `ties` layout


def random_state(rng, k):
    h, w = int(rng.integers(1, GMAX + 1)), int(rng.integers(1, GMAX + 1))
    if k % 13 == 0:
        h = 1
    elif k % 13 == 1:
        w = 1
    boxes = []
    for _ in range(int(rng.integers(0, 5))):
        x1, y1 = int(rng.integers(0, w * P)), int(rng.integers(0, h * P))
        boxes.append([x1, y1, x1 + int(rng.integers(0, 3 * P)), y1 + int(rng.integers(0, 3 * P))])
    return h, w, boxes, (int(rng.integers(0, h)), int(rng.integers(0, w)))


def main():
    install_stubs()
    sys.path.insert(0, str(REF))
    from src.env import simple_env as se
    from src.utils import BBox, Position

    rng = np.random.default_rng(11)
    states = [TIES] + [random_state(rng, k) for k in range(N_RANDOM)]
    n = len(states)
    out = {"patch_size": np.int64(P), "hw": np.zeros((n, 2), np.int64), "position": np.zeros((n, 2), np.int64),
           "boxes": np.zeros((n, 4, 4), np.int64), "n_boxes": np.zeros(n, np.int64),
           "targets": np.zeros((n, GMAX, GMAX), np.uint8), "visited": np.zeros((n, GMAX, GMAX), np.uint8),
           "n_nearest": np.zeros(n, np.int64), "sets": np.zeros(n, np.uint8)}
    real_random = se.random
    for i, (h, w, boxes, pos) in enumerate(states):
        bbs = [BBox(up_left=Position(y=b[1], x=b[0]), bottom_right=Position(y=b[3], x=b[2])) for b in boxes]
        env = se.NeedleSimpleEnv(torch.zeros(3, h * P, w * P), P, bbs, seed=i)
        cells = sorted(env.bbox_patches)
        if i == 0:
            seen = set()
        elif i % 10 == 0:
            seen = set(cells)                                     # nothing left to visit
        else:
            seen = {c for c in cells if rng.random() < 0.4}
        env.reset(Position(*pos), set(seen))
        handed = []

        def recorder(candidates):
            handed.append(list(candidates))
            return real_random.choice(candidates)

        se.random = types.SimpleNamespace(choice=recorder)
        try:
            random.seed(i)
            env.build_keypoints_trajectory()
        finally:
            se.random = real_random
        nearest = handed[0] if handed else []
        bits = 0
        for q in nearest:
            a = se.move_towards(env.position, q)
            assert a is not se.Action.STOP
            bits |= 1 << a.value
        out["hw"][i], out["position"][i] = (h, w), pos
        out["boxes"][i, :len(boxes)] = np.array(boxes, np.int64).reshape(-1, 4)
        out["n_boxes"][i] = len(boxes)
        for c in cells:
            out["targets"][i, c.y, c.x] = 1
        for c in env.visited_bbox_patches:                        # reset() adds the start cell when it is a target
            out["visited"][i, c.y, c.x] = 1
        out["n_nearest"][i], out["sets"][i] = len(nearest), bits
    popcount = np.array([bin(int(s)).count("1") for s in out["sets"]])
    assert int(((out["n_nearest"] >= 2) & (popcount >= 2)).sum()) >= 20, "too few tied states with different actions"
    assert int((out["n_nearest"] == 0).sum()) >= 10, "too few states with nothing left"
    assert int((out["hw"].min(axis=1) == 1).sum()) >= 5, "too few one-row / one-column grids"
    assert out["n_nearest"][0] == 4 and popcount[0] == 4, "the ties layout must give four nearest cells"
    np.savez_compressed(HERE / "g11_teacher_sets.npz", **out)
    print("g11_teacher_sets.npz", (HERE / "g11_teacher_sets.npz").stat().st_size, "states", n,
          "tied", int(((out["n_nearest"] >= 2) & (popcount >= 2)).sum()), "empty", int((out["n_nearest"] == 0).sum()),
          "thin", int((out["hw"].min(axis=1) == 1).sum()))


if __name__ == "__main__":
    main()
