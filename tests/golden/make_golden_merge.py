"""Generate tests/golden/g10_merge_boxes.npz by running the REFERENCE's merge_boxes (src/utils.py:198-255, imported
read-only from the reference tree, `REF` of make_golden.py) on CPU.

Run in the build container only:  python tests/golden/make_golden_merge.py
The fixture holds inputs and the reference's outputs — no source.  Every case has a prediction form ([n, 7] fp32:
x1, y1, x2, y2, obj, cls, class id -> [g, 6]) and a target form ([n, 5] int64: 0, x1, y1, x2, y2 -> [g, 5]); the target
geometry is the prediction geometry rounded down.

The script also runs the rule this repository's host ``merge_boxes`` followed before it was corrected (box i keeps the
group of the FIRST box that claimed it; the reference puts it into the LOWEST-numbered group that contains it) and
prints on how many of the kept cases that rule differs from the reference.
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True

from make_golden import install_stubs, REF  # noqa: E402

THRESHOLD = 2
N_RANDOM, N_DIVERGENT, N_AGREEING = 3000, 24, 8


def first_claim_merge(boxes, threshold=2, target=False):
    """The repository's former restatement: group_of[j] is set by the first box that pulls j in and never lowered."""
    off = 1 if target else 0
    n = len(boxes)
    group_of, groups = [-1] * n, []
    for i in range(n):
        if group_of[i] < 0:
            group_of[i] = len(groups)
            groups.append([i])
        a = boxes[i]
        for j in range(i + 1, n):
            b = boxes[j]
            d = min(abs(float(b[off + 2] - a[off + 0])), abs(float(a[off + 2] - b[off + 0])),
                    abs(float(b[off + 3] - a[off + 1])), abs(float(a[off + 3] - b[off + 1])))
            if d <= threshold:
                groups[group_of[i]].append(j)
                if group_of[j] < 0:
                    group_of[j] = group_of[i]
    rows = []
    for grp in groups:
        sel = boxes[sorted(set(grp))]
        row = [sel[:, off + 0].min(), sel[:, off + 1].min(), sel[:, off + 2].max(), sel[:, off + 3].max()]
        if target:
            row = [torch.zeros((), dtype=boxes.dtype)] + row
        else:
            row += [(sel[:, 4] * sel[:, 5]).max(), torch.ones((), dtype=boxes.dtype)]
        rows.append(torch.stack([torch.as_tensor(v, dtype=boxes.dtype) for v in row]))
    return torch.stack(rows)


def with_scores(xyxy, gen):
    """[n, 4] -> prediction rows [n, 7] with random obj / cls confidences."""
    n = len(xyxy)
    return torch.cat((xyxy.float(), torch.rand((n, 2), generator=gen), torch.zeros((n, 1))), 1)


def sparse_boxes(n, gen, n_links):
    """n boxes of which no two are within the threshold on any edge pair (every edge coordinate is unique by >= 12 px
    on both axes), then n_links boxes moved next to another one so that some groups form."""
    xs = torch.randperm(n, generator=gen) * 40
    ys = torch.randperm(n, generator=gen) * 40
    wh = torch.randint(5, 20, (n, 2), generator=gen)
    b = torch.stack((xs, ys, xs + wh[:, 0], ys + wh[:, 1]), 1)
    for _ in range(min(n_links, n // 2)):
        i, j = (int(v) for v in torch.randperm(n, generator=gen)[:2])
        gap = int(torch.randint(0, 3, (1,), generator=gen))
        b[j] = torch.stack((b[i, 2] + gap, b[i, 1] + 1, b[i, 2] + gap + 9, b[i, 3] + 3))       # right of i, `gap` px apart
    return b


def staircase(n):
    k = torch.arange(n) * 20
    return torch.stack((k, k, k + 18, k + 18), 1)          # step k ends 2 px before step k + 1 begins, on both axes


def main():
    install_stubs()
    sys.path.insert(0, str(REF))
    from src.utils import merge_boxes as ref_merge

    gen = torch.Generator().manual_seed(0)
    cases = []                                              # (name, [n, 7] fp32)
    divergent, agreeing = [], []
    for trial in range(N_RANDOM):
        xy = torch.randint(0, 60, (6, 2), generator=gen)
        wh = torch.randint(3, 15, (6, 2), generator=gen)
        pred = with_scores(torch.cat((xy, xy + wh), 1), gen)
        differs = not torch.equal(ref_merge(pred, THRESHOLD), first_claim_merge(pred, THRESHOLD))
        (divergent if differs else agreeing).append((f"random{trial:04d}", pred))
    print(f"random family: the former host rule differs from the reference on {len(divergent)} of {N_RANDOM} cases")
    cases += divergent[:N_DIVERGENT] + agreeing[:N_AGREEING]

    cases.append(("staircase64", with_scores(staircase(64), gen)))
    cases.append(("staircase64_reversed", with_scores(staircase(64).flip(0), gen)))
    # pairs at distance exactly threshold and threshold + 1 (on x, on y; every other edge pair far apart)
    cases.append(("pair_at_threshold", with_scores(torch.tensor([[0, 0, 10, 10], [12, 100, 30, 130], [200, 300, 220, 320],
                                                                 [500, 322, 520, 340]]), gen)))
    cases.append(("pair_past_threshold", with_scores(torch.tensor([[0, 0, 10, 10], [13, 100, 30, 130], [200, 300, 220, 320],
                                                                   [500, 323, 520, 340]]), gen)))
    dup = torch.tensor([[5, 5, 20, 20], [100, 100, 140, 130], [5, 5, 20, 20], [100, 100, 140, 130], [300, 400, 310, 410],
                        [5, 5, 20, 20]])
    cases.append(("duplicates", with_scores(dup, gen)))
    neg = torch.tensor([[-50, -40, -30, -20], [-28, -100, -10, -70], [-300, -18, -250, 5], [40, 60, 50, 70], [-7, 200, 3, 230],
                        [5, 400, 60, 450]])
    cases.append(("negative", with_scores(neg, gen)))
    frac = torch.rand((40, 2), generator=gen) * 300 - 50
    cases.append(("fractional", with_scores(torch.cat((frac, frac + 3 + torch.rand((40, 2), generator=gen) * 20), 1), gen)))
    for n in (1, 255, 256, 257, 600):
        cases.append((f"sparse{n}", with_scores(sparse_boxes(n, gen, n // 8), gen)))

    out = {"names": np.array([c[0] for c in cases]), "threshold": np.array(THRESHOLD, np.int64)}
    fails_pred = fails_tgt = 0
    for name, pred in cases:
        tgt = torch.cat((torch.zeros((len(pred), 1), dtype=torch.long), pred[:, :4].floor().long()), 1)
        pred_out = ref_merge(pred, THRESHOLD)
        tgt_out = ref_merge(tgt, THRESHOLD, target=True)
        assert pred_out.dtype == torch.float32 and tgt_out.dtype == torch.long
        out[f"{name}.pred"], out[f"{name}.pred_out"] = pred.numpy(), pred_out.numpy()
        out[f"{name}.tgt"], out[f"{name}.tgt_out"] = tgt.numpy(), tgt_out.numpy()
        if name.startswith("random"):
            fails_pred += not torch.equal(first_claim_merge(pred, THRESHOLD), pred_out)
            fails_tgt += not torch.equal(first_claim_merge(tgt, THRESHOLD, target=True), tgt_out)
    print(f"kept {len(cases)} cases; the former host rule fails {fails_pred} of them in prediction form, "
          f"{fails_tgt} in target form")
    assert fails_pred >= 20
    np.savez_compressed(HERE / "g10_merge_boxes.npz", **out)
    print("g10_merge_boxes.npz", (HERE / "g10_merge_boxes.npz").stat().st_size)


if __name__ == "__main__":
    main()
