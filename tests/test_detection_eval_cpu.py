"""merge_boxes against the reference's own outputs (tests/golden/g10_merge_boxes.npz, written by
tests/golden/make_golden_merge.py from src/utils.py:198-255): the host function, and the parallel statement of the same
rule that the device kernel (csrc/kernels_eval.hip) implements.  Everything here compares with ``torch.equal``: the rule
rounds nothing but one fp32 multiply per prediction."""
from pathlib import Path

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "g10_merge_boxes.npz"


@pytest.fixture(scope="module")
def g10():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def g10_cases(g10):
    for name in g10["names"].tolist():
        for form in ("pred", "tgt"):
            yield name, form, torch.from_numpy(g10[f"{name}.{form}"]), torch.from_numpy(g10[f"{name}.{form}_out"])


def parallel_merge(boxes, threshold, target):
    """The rule in the form the kernel computes it.  adj(i, j): the smallest of the four edge distances is within the
    threshold.  r(j) = j where no i < j is adjacent, else min r(i) over those i, reached by relaxing from r(j) = j.  The
    groups are the distinct labels in ascending order; group g holds every i with r(i) = g and every j > i adjacent to
    such an i.  Returns (rows, relaxation rounds)."""
    off = 1 if target else 0
    c = boxes[:, off:off + 4]
    n = len(c)
    d = torch.stack(((c[None, :, 2] - c[:, None, 0]).abs(), (c[:, None, 2] - c[None, :, 0]).abs(),
                     (c[None, :, 3] - c[:, None, 1]).abs(), (c[:, None, 3] - c[None, :, 1]).abs())).amin(0)
    idx = torch.arange(n)
    pulls = (d <= threshold) & (idx[:, None] < idx[None, :])          # pulls[i, j]: box i pulls the later box j
    r, rounds = idx.clone(), 0
    while True:
        new = torch.minimum(idx, torch.where(pulls, r[:, None], n).amin(0))
        rounds += 1
        if torch.equal(new, r):
            break
        r = new
    # (group, member) pairs: every box with its own label, every pulled box with the label of the box that pulls it
    gi, gj = pulls.nonzero(as_tuple=True)
    labels = torch.unique(r)                                          # ascending: the order the reference opens them
    slot, member = torch.searchsorted(labels, torch.cat((r, r[gi]))), torch.cat((idx, gj))

    def over_members(col, how):
        return torch.zeros(len(labels), dtype=col.dtype).scatter_reduce(0, slot, col[member], how, include_self=False)
    cols = [over_members(boxes[:, off + 0], "amin"), over_members(boxes[:, off + 1], "amin"),
            over_members(boxes[:, off + 2], "amax"), over_members(boxes[:, off + 3], "amax")]
    if target:
        cols = [torch.zeros_like(cols[0])] + cols
    else:
        cols += [over_members(boxes[:, 4] * boxes[:, 5], "amax"), torch.ones_like(cols[0])]
    rows = torch.stack(cols, 1)
    return rows, rounds


def test_fixture_covers_the_cases_the_kernel_can_get_wrong(g10):
    names = g10["names"].tolist()
    assert int(g10["threshold"]) == 2
    assert sum(n.startswith("random") for n in names) >= 28
    for n in ("staircase64", "staircase64_reversed", "pair_at_threshold", "pair_past_threshold", "duplicates", "negative",
              "sparse1", "sparse255", "sparse256", "sparse257", "sparse600"):
        assert n in names
    assert len(g10["pair_at_threshold.pred_out"]) == 2 and len(g10["pair_past_threshold.pred_out"]) == 4
    assert len(g10["staircase64.tgt_out"]) == 1 and (g10["negative.pred"][:, :4] < 0).any()


def test_host_merge_boxes_equals_the_reference_on_every_case(g10):
    """Fails with the former rule (a box kept the group of the first box that claimed it) on the divergent random cases."""
    wrong = []
    for name, form, boxes, want in g10_cases(g10):
        got = ja.merge_boxes(boxes, threshold=2, target=form == "tgt")
        if not (got.dtype == want.dtype and torch.equal(got, want)):
            wrong.append((name, form))
    assert not wrong, wrong


def test_parallel_rule_equals_the_reference_on_every_case(g10):
    most = 0
    for name, form, boxes, want in g10_cases(g10):
        got, rounds = parallel_merge(boxes, 2, form == "tgt")
        assert got.dtype == want.dtype and torch.equal(got, want), (name, form)
        if name == "staircase64":
            assert rounds == 64                                      # 63 rounds that lower a label and the one that finds none
        most = max(most, rounds)
    assert most == 64


def test_eval_entry_points_refuse_bad_shapes_before_any_launch():
    lib = _lib.load_library()
    one = torch.zeros(8)
    p = _lib.ptr(one)
    assert lib.jn_merge_boxes(None, None, 1, 4, 7, 0, 2.0, None, None, None, None) == -1
    assert b"jn_merge_boxes" in lib.jn_last_error()
    assert lib.jn_merge_boxes(p, p, 1, 4097, 7, 0, 2.0, p, p, None, None) == -1           # JN_EINVAL, nothing launched
    assert b"4097" in lib.jn_last_error() and b"4096" in lib.jn_last_error()
    assert lib.jn_merge_boxes(p, p, 1, 4, 5, 0, 2.0, p, p, None, None) == -1              # predictions have 6 or 7 columns
    assert lib.jn_merge_boxes(p, p, 1, 4, 7, 1, 2.0, p, p, None, None) == -1              # targets have 5
    assert lib.jn_match_detections(None, None, 1, 4, 7, None, None, 0, 100, None, None, None, None, None, None) == -1
    assert b"jn_match_detections" in lib.jn_last_error()
    assert lib.jn_match_detections(p, p, 1, 4097, 7, p, p, 1, 100, p, p, p, p, p, None) == -1
    assert lib.jn_average_precision(None, None, None, None, 1, 100, 0, None, 101, None, None) == -1
    assert b"jn_average_precision" in lib.jn_last_error()
    assert lib.jn_average_precision(p, p, p, p, 83, 100, 1, p, 101, p, None) == -1        # 8300 pooled slots > 8192
    assert b"8300" in lib.jn_last_error()
    assert lib.jn_average_precision(p, p, p, p, 1, 100, 0, p, 257, p, None) == -1
