"""Generate tests/golden/g9_image_views.npz by running the REFERENCE's NeedleDataset.rotate / translate
(src/dataset.py:95-226, imported read-only from the reference tree, `REF` of make_golden.py) on CPU for a set of seeded cases.

Run in the build container only:  python tests/golden/make_golden_views.py
torchvision is absent there, so ``F.affine`` is replaced by a recorder that stores the (tx, ty) the reference asks for
and returns the image unchanged: the fixture pins the reference's draws and box arithmetic, the shift itself stays a
restatement.  The fixture holds inputs and recorded results — no source.  Images are the integer ramp
`case_image()` so that the tests can rebuild them.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True

from make_golden import install_stubs, REF  # noqa: E402

# (name, Hs, Ws, boxes xyxy, numpy seed, rotations, translations).  With rng.choice(np.arange(4), (1,)) the seeds
# 0, 1, 4 and 11 of np.random.default_rng draw 270, 90, 180 and 0 degrees.
CASES = [
    ("square_270", 32, 32, [[4, 6, 12, 15]], 0, True, True),
    ("square_90", 32, 32, [[4, 6, 12, 15], [20, 2, 27, 9]], 1, True, True),
    ("square_180", 32, 32, [[10, 10, 20, 21]], 4, True, True),
    ("square_0", 32, 32, [[8, 9, 17, 18]], 11, True, True),
    ("wide_270", 24, 48, [[5, 3, 30, 14], [33, 10, 41, 20]], 0, True, True),
    ("wide_90", 24, 48, [[12, 4, 25, 19]], 1, True, True),
    ("tall_180", 48, 24, [[3, 20, 11, 40], [14, 2, 20, 9], [6, 10, 9, 13]], 4, True, True),
    ("tall_0", 48, 24, [[2, 5, 20, 41]], 11, True, True),
    ("edge_left_top", 32, 48, [[0, 0, 9, 7]], 11, True, True),             # both up-left margins are 0
    ("edge_full_width", 32, 48, [[0, 10, 48, 20]], 11, True, True),         # no draw for x at all
    ("rotate_only", 32, 48, [[7, 8, 19, 22]], 1, True, False),
    ("translate_only", 32, 48, [[7, 8, 19, 22], [30, 1, 40, 12]], 3, False, True),
    ("edge_after_rotation", 24, 48, [[0, 0, 10, 24]], 0, True, True),
]


def case_image(Hs, Ws):
    return torch.arange(3 * Hs * Ws, dtype=torch.float32).reshape(3, Hs, Ws)


def main():
    install_stubs()
    sys.path.insert(0, str(REF))
    import src.dataset as ds
    from src.utils import BBox, Position

    calls = []

    def affine(image, angle, translate, scale, shear, fill):
        assert angle == 0 and scale == 1.0 and shear == 0.0 and fill == 0.0
        calls.append((int(translate[0]), int(translate[1])))
        return image

    ds.F.affine = affine
    dataset = ds.NeedleDataset.__new__(ds.NeedleDataset)        # rotate / translate read no attribute of self

    def to_rows(bbs):
        return np.array([[b.up_left.x, b.up_left.y, b.bottom_right.x, b.bottom_right.y] for b in bbs], np.int64).reshape(-1, 4)

    out = {"names": np.array([c[0] for c in CASES])}
    for name, Hs, Ws, boxes, seed, rotations, translations in CASES:
        image = case_image(Hs, Ws)
        bbs = [BBox(up_left=Position(y=b[1], x=b[0]), bottom_right=Position(y=b[3], x=b[2])) for b in boxes]
        rng = np.random.default_rng(seed)
        rotated, rot_boxes = image, bbs
        if rotations:                                            # the order of transform, src/dataset.py:274-278
            rotated, rot_boxes = dataset.rotate(image, bbs, rng)
        final_boxes, t = rot_boxes, (0, 0)
        if translations:
            del calls[:]
            _, final_boxes = dataset.translate(rotated, rot_boxes, rng)
            (t,) = calls
        out[f"{name}.args"] = np.array([Hs, Ws, seed, int(rotations), int(translations)], np.int64)
        out[f"{name}.boxes"] = np.array(boxes, np.int64).reshape(-1, 4)
        out[f"{name}.rotated"] = rotated.numpy().astype(np.int16)       # the ramp stays below 2^15
        out[f"{name}.rotated_boxes"] = to_rows(rot_boxes)
        out[f"{name}.final_boxes"] = to_rows(final_boxes)
        out[f"{name}.translate_xy"] = np.array(t, np.int64)
        out[f"{name}.rng_after"] = np.array(rng.integers(0, 1 << 30, (1,)), np.int64)   # the stream position afterwards
    np.savez_compressed(HERE / "g9_image_views.npz", **out)
    print("g9_image_views.npz", (HERE / "g9_image_views.npz").stat().st_size)


if __name__ == "__main__":
    main()
