"""Inputs and independent restatements shared by tests/test_detection_cells_cpu.py and tests/test_gpu_detection_cells.py
(``detection.detection_cells`` and its device twin ``jn_detection_cells``).

The boxes are built from named kinds, each the smallest box that takes one branch of the rule: a box inside one cell,
across one border, across a corner (four pieces), over three cells, ending on the last pixel of a cell (x2 = P - 1)
and on the first of the next (x2 = P), a zero padding row, a box beyond the right / bottom of the grid, a box with a
negative coordinate, x2 < x1 within one cell, a box left of and above the grid, a box with y2 // P < y1 // P, and a box
over the whole grid (an image without an empty cell)."""
import numpy as np
import torch

P = 8
GRIDS = [(1, 1), (2, 2), (3, 5), (12, 25)]       # 12 x 25 = 300 cells: more than one pass of a 256-thread workgroup
BATCHES = [1, 3, 65]
NBS = [1, 3]
NEG_TAG = 0x4E454753

KINDS = ["inside", "border", "corner", "three", "x2_last", "x2_next", "zero", "beyond", "negative", "reversed", "outside",
         "y_reversed", "whole"]


def make_box(kind: str, cy: int, cx: int, gh: int, gw: int):
    """One xyxy box of `kind`; the relative kinds sit at cell (cy, cx)."""
    ox, oy = cx * P, cy * P
    rel = {"inside": (1, 2, 5, 6), "border": (3, 1, P + 2, 4), "corner": (P - 3, P - 2, P + 1, P + 3),
           "three": (2, 3, 2 * P + 4, 5), "x2_last": (2, 2, P - 1, 5), "x2_next": (2, 2, P, 5), "reversed": (6, 2, 3, 5),
           "y_reversed": (2, 2 * P + 4, 5, 3)}
    if kind in rel:
        b = rel[kind]
        return [b[0] + ox, b[1] + oy, b[2] + ox, b[3] + oy]
    return {"zero": [0, 0, 0, 0], "beyond": [gw * P - 3, gh * P - 2, gw * P + 10, gh * P + 9], "negative": [-5, -3, 4, 4],
            "outside": [-20, -19, -10, -9], "whole": [0, 0, gw * P - 1, gh * P - 1]}[kind]


def make_boxes(gh: int, gw: int, B: int, nb: int, shift: int = 0) -> torch.Tensor:
    """[B, nb, 4] int64: slot (i, k) takes kind (i * nb + k + shift) mod 13 at a cell that moves with i."""
    out = torch.zeros((B, nb, 4), dtype=torch.int64)
    for i in range(B):
        for k in range(nb):
            kind = KINDS[(i * nb + k + shift) % len(KINDS)]
            out[i, k] = torch.tensor(make_box(kind, (i + k) % gh, (i // gh + 2 * k) % gw, gh, gw))
    return out


def make_extents(gh: int, gw: int, B: int) -> torch.Tensor:
    """int32 [B, 2]: every third image keeps the whole grid, the others a smaller one (boxes then reach past it)."""
    return torch.tensor([[gh, gw] if i % 3 == 0 else [1 + (i * 5) % gh, 1 + (i * 3) % gw] for i in range(B)], dtype=torch.int32)


def sample_negs(gh: int, gw: int):
    """0, 1, 2 and gh * gw = n_empty + 1 of an image with one positive cell (more than any image has empty cells)."""
    return [0, 1, 2, gh * gw]


def all_cases():
    """(gh, gw, B, nb, bboxes, extents or None): every grid x batch x nb, each without and (beyond 1 x 1) with extents."""
    for gh, gw in GRIDS:
        for B in BATCHES:
            for nb in NBS:
                bb = make_boxes(gh, gw, B, nb, shift=gh + B + nb)
                yield gh, gw, B, nb, bb, None
                if gh * gw > 1:
                    yield gh, gw, B, nb, bb, make_extents(gh, gw, B)


def host_path_rows(bboxes: torch.Tensor, gh: int, gw: int, extents=None):
    """The positive rows as the host ``get_detection_batch`` forms them: ``split_bboxes_over_patches`` +
    ``masks.any(-1)`` + ``nonzero`` + ``F.pad``; with extents the cells outside an image's extent are dropped (the
    pieces there, and the cells themselves).  Returns per image (cells [n, 2], targets [n, nb, 5])."""
    from jolineedle_amd.detection import split_bboxes_over_patches
    boxes, masks = split_bboxes_over_patches(bboxes, gh, gw, P)
    out = []
    for i in range(bboxes.shape[0]):
        any_box = masks[i].any(-1)
        if extents is not None:
            eh, ew = (int(v) for v in extents[i])
            any_box[eh:, :] = False
            any_box[:, ew:] = False
        pos = torch.nonzero(any_box)
        tg = [torch.nn.functional.pad(boxes[i, y, x], (1, 0)) for y, x in pos.tolist()]
        out.append((pos, torch.stack(tg) if tg else torch.zeros((0, bboxes.shape[1], 5), dtype=torch.int64)))
    return out


def draw_negatives(positive: np.ndarray, eh: int, ew: int, image: int, sample_neg: int, seed: int):
    """The negatives of one image, draw by draw, with the oracle's Philox: `positive` bool [gh, gw]; the image's cells
    are the top-left eh x ew."""
    from oracle.dropout_ref import philox4x32
    E = [(y, x) for y in range(eh) for x in range(ew) if not positive[y, x]]
    out = []
    for j in range(min(sample_neg, len(E))):
        r = philox4x32(seed, *[np.array([c], dtype=np.uint32) for c in (image, j, NEG_TAG, 0)])[0]
        o = j + int(r[0]) % (len(E) - j)
        E[j], E[o] = E[o], E[j]
        out.append(E[j])
    return out
