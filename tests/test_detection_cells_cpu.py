"""``detection.detection_cells`` — the host statement of the rule ``jn_detection_cells`` computes — against the existing
host path of ``NeedleGeneralEnv.get_detection_batch`` (positives and targets), the reference's own answer (G7), and a
draw-by-draw restatement of the negatives with the oracle's Philox; and the uniformity of those draws."""
import numpy as np
import torch

from jolineedle_amd import detection
from tests import detection_cells_cases as dc

P = dc.P


def _positive_grid(cells, n_pos, offsets, i, gh, gw):
    g = np.zeros((gh, gw), bool)
    for _, y, x in cells[int(offsets[i]):int(offsets[i]) + int(n_pos[i])].tolist():
        g[y, x] = True
    return g


def test_positives_and_targets_match_the_existing_host_path():
    n_cases = 0
    for gh, gw, B, nb, bb, ext in dc.all_cases():
        cells, targets, offsets, n_pos = detection.detection_cells(bb, gh, gw, P, 0, 0, extents=ext)
        assert cells.dtype == targets.dtype == torch.int64 and offsets.dtype == n_pos.dtype == torch.int32
        assert cells.shape == (int(offsets[B]), 3) and targets.shape == (int(offsets[B]), nb, 5)
        assert offsets[0] == 0 and torch.equal(offsets[1:] - offsets[:-1], n_pos)           # sample_neg = 0: positives only
        for i, (pos, tg) in enumerate(dc.host_path_rows(bb, gh, gw, ext)):
            a, b = int(offsets[i]), int(offsets[i + 1])
            assert bool((cells[a:b, 0] == i).all()), (gh, gw, B, nb, i)
            assert torch.equal(cells[a:b, 1:], pos), (gh, gw, B, nb, i)
            assert torch.equal(targets[a:b], tg), (gh, gw, B, nb, i)
        n_cases += 1
    assert n_cases == 42                                                                     # 4 x 3 x 2, 18 of them with extents too


def test_every_box_kind_takes_its_branch():
    gh, gw = 3, 5
    want = {"inside": [(1, 1)], "border": [(1, 1), (1, 2)], "corner": [(1, 1), (1, 2), (2, 1), (2, 2)],
            "three": [(1, 1), (1, 2), (1, 3)], "x2_last": [(1, 1)], "x2_next": [(1, 1), (1, 2)], "zero": [(0, 0)],
            "beyond": [(2, 4)], "negative": [(0, 0)], "reversed": [(1, 1)], "outside": [], "y_reversed": [],
            "whole": [(y, x) for y in range(gh) for x in range(gw)]}
    assert sorted(want) == sorted(dc.KINDS)
    for kind, cells_want in want.items():
        bb = torch.tensor([[dc.make_box(kind, 1, 1, gh, gw)]])
        cells, targets, offsets, n_pos = detection.detection_cells(bb, gh, gw, P, 0, 0)
        assert [tuple(c[1:]) for c in cells.tolist()] == cells_want, kind
    _, t, _, _ = detection.detection_cells(torch.tensor([[dc.make_box("reversed", 1, 1, gh, gw)]]), gh, gw, P, 0, 0)
    assert t.tolist() == [[[0, 6, 2, 3, 5]]]
    _, t, _, _ = detection.detection_cells(torch.tensor([[dc.make_box("negative", 0, 0, gh, gw)]]), gh, gw, P, 0, 0)
    assert t.tolist() == [[[0, 0, 0, 4, 4]]]
    _, t, _, _ = detection.detection_cells(torch.zeros((1, 2, 4), dtype=torch.int64), gh, gw, P, 0, 0)
    assert t.tolist() == [[[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]]                             # the padding quirk: cell (0, 0), zero boxes


def test_reference_known_answer_g7(golden):
    """Box [410, 410, 500, 500] at P = 448 (the reference's tests/test_map.py): its four pieces, and the second box's one,
    moved back to image pixels, are the reference's ``get_detection_targets``."""
    g = golden("g7_known_answers.npz")
    bb = torch.from_numpy(g["targets_bboxes"])
    cells, targets, offsets, n_pos = detection.detection_cells(bb, 1792 // 448, 2240 // 448, 448, 0, 0)
    assert n_pos.tolist() == [5] and offsets.tolist() == [0, 5]
    rows = []
    for (_, y, x), tg in zip(cells.tolist(), targets):
        for k in range(tg.shape[0]):
            if int(tg[k].abs().sum()):
                rows.append((tg[k] + torch.tensor([0, x, y, x, y]) * 448).tolist())
    assert rows == g["targets_expected"].tolist()
    assert cells[:, 1:].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [3, 3]]


def test_negatives_are_well_formed_and_follow_the_stated_draws():
    seed = 0x1234_5678_9ABC_DEF1
    for gh, gw, B, nb, bb, ext in dc.all_cases():
        for sn in dc.sample_negs(gh, gw):
            if B == 65 and sn > 2:
                continue                                         # (thousands of single Philox calls of the oracle; B = 3 draws them all)
            cells, targets, offsets, n_pos = detection.detection_cells(bb, gh, gw, P, sn, seed, extents=ext)
            for i in range(B):
                eh, ew = (gh, gw) if ext is None else (int(ext[i, 0]), int(ext[i, 1]))
                positive = _positive_grid(cells, n_pos, offsets, i, gh, gw)
                n_empty = eh * ew - int(n_pos[i])
                neg = cells[int(offsets[i]) + int(n_pos[i]):int(offsets[i + 1])]
                assert len(neg) == min(sn, n_empty), (gh, gw, B, nb, sn, i)
                got = [(y, x) for _, y, x in neg.tolist()]
                assert len(set(got)) == len(got)                                               # distinct
                assert all(0 <= y < eh and 0 <= x < ew and not positive[y, x] for y, x in got)  # inside the extent, empty
                assert bool((neg[:, 0] == i).all())
                assert not bool(targets[int(offsets[i]) + int(n_pos[i]):int(offsets[i + 1])].any())
                assert got == dc.draw_negatives(positive, eh, ew, i, sn, seed), (gh, gw, B, nb, sn, i)


def test_negatives_depend_on_seed_and_image_index_only():
    gh, gw = 3, 5
    bb = dc.make_boxes(gh, gw, 7, 3, shift=2)
    big = detection.detection_cells(bb, gh, gw, P, 2, 99)
    for B in (1, 2, 5):
        small = detection.detection_cells(bb[:B], gh, gw, P, 2, 99)
        n = int(small[2][B])
        assert torch.equal(small[0], big[0][:n]) and torch.equal(small[1], big[1][:n])
        assert torch.equal(small[2], big[2][:B + 1]) and torch.equal(small[3], big[3][:B])
    other = detection.detection_cells(bb, gh, gw, P, 2, 100)
    assert torch.equal(other[3], big[3]) and not torch.equal(other[0], big[0])                # another seed: other negatives


SEEDS = range(3000)


def test_negative_draws_are_uniform():
    """4 x 4 grid, one positive cell, one negative per seed over the committed range of 3000 seeds: chi-square over the
    15 empty cells (200 expected in each) below the 1 - 1e-6 quantile of chi2(14), which a uniform draw passes with
    that probability."""
    from scipy.stats import chi2
    bb = torch.tensor([[dc.make_box("inside", 1, 2, 4, 4)]])
    counts = np.zeros((4, 4), np.int64)
    for seed in SEEDS:
        cells, _, offsets, n_pos = detection.detection_cells(bb, 4, 4, P, 1, seed)
        assert n_pos.tolist() == [1] and offsets.tolist() == [0, 2] and cells[0].tolist() == [0, 1, 2]
        counts[cells[1, 1], cells[1, 2]] += 1
    assert counts[1, 2] == 0 and counts.sum() == len(SEEDS)
    obs = np.delete(counts.reshape(-1), 1 * 4 + 2)
    expect = len(SEEDS) / 15
    stat = float(((obs - expect) ** 2 / expect).sum())
    print(f"chi-square {stat:.3f} over {obs.tolist()}")
    assert stat < chi2.ppf(1 - 1e-6, 14), stat


def test_detbatch_ab_help():
    import subprocess
    import sys
    from pathlib import Path
    tool = Path(__file__).resolve().parent.parent / "tools" / "detbatch_ab.py"
    r = subprocess.run([sys.executable, str(tool), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--sample-neg" in r.stdout and "--step-timeout" in r.stdout
