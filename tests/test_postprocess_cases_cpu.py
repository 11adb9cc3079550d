"""CPU only, reference only: the committed postprocess cases (tests/postprocess_cases.py) mean something before any kernel
sees them.  The NumPy reference equals the oracle (oracle/yolox_ref.py::postprocess + clamp) bit for bit, every case keeps
its IoU comparisons away from the threshold by 16 x the fp32 IoU's own error, and every case reaches the branch it is
named after: a deliberately wrong reference (`run(..., conf_strict / iou_ge / tie_high_index / dead_suppress /
clamp_first)`) gives another answer on it."""
import numpy as np
import torch

from oracle import yolox_ref
from tests import postprocess_cases as pc

F = np.float32


def _oracle(raw, case):
    if raw.shape[0] == 1:                          # the oracle's squeeze() needs two anchors; the second one does not pass
        raw = np.concatenate((raw, np.array([[5, 5, 4, 4, min(case.conf, 0.0) - 1.0, 1.0]], F)))
    out = yolox_ref.postprocess(torch.from_numpy(np.array(raw))[None], 1, case.conf, case.nms, class_agnostic=True)[0]
    if out is None:
        return torch.zeros((0, 7))
    out[:, :4].clamp_(0, case.P - 1)
    return out


def _mutant(case, **flag):
    return pc.run(pc.build(case), case.conf, case.nms, case.P, case.max_out, **flag)


def _same(x, y):
    return x[1] == y[1] and x[2] == y[2] and np.array_equal(x[0], y[0], equal_nan=False)


def test_reference_equals_the_oracle():
    """torch.equal on every case.  Where a cap is reached the oracle, which has none, sees what the caps leave: the first
    2048 passing anchors, and the first max_out rows of its answer."""
    reached = dict(cap=0, max_out=0)
    for case in pc.CASES:
        rows, count, (n_pass, n_keep) = pc.reference(case)
        raw = np.array(pc.build(case))
        if n_pass > pc.DET_CAP:
            score = raw[:, 4] * raw[:, 5]
            late = np.nonzero(score >= F(case.conf))[0][pc.DET_CAP:]
            assert len(late) == n_pass - pc.DET_CAP
            raw[late, 4] = F(min(case.conf, 0.0) - 1.0)            # no longer passes
            reached["cap"] += 1
        want = _oracle(raw, case)
        assert want.shape[0] == n_keep, case.name
        reached["max_out"] += n_keep > case.max_out
        want = want[:case.max_out]
        assert count == want.shape[0] == min(n_keep, case.max_out), case.name
        assert torch.equal(torch.from_numpy(np.array(rows)).reshape(-1, 7), want), case.name
        assert rows.dtype == F and bool((rows[:, 6] == 0).all())
    assert reached == dict(cap=2, max_out=2), reached


def test_every_case_is_admissible_and_the_bar_is_the_measured_one(capsys):
    worst_b, least_a, lines = 0.0, float("inf"), []
    for case in pc.CASES:
        m = pc.margins(case)
        worst_b, least_a = max(worst_b, m["b"]), min(least_a, m["a"])
        lines.append(f"  {case.name:18s} pairs {m['pairs']:8d}  exactly on the threshold {m['exact']:4d}  NaN {m['nan']:2d}  "
                     f"(a) {m['a']:.3e}  (b) {m['b']:.3e}")
    with capsys.disabled():
        print("\npostprocess cases: (a) least |iou64 - thr| off the exact ties, (b) largest |iou32 - iou64|")
        print("\n".join(lines))
        print(f"  largest (b) {worst_b:.3e}  ->  16 x = {16 * worst_b:.3e} (MARGIN_BAR {pc.MARGIN_BAR:.3e});  least (a) {least_a:.3e}")
    for case in pc.CASES:
        assert pc.margins(case)["a"] > pc.MARGIN_BAR, (case.name, pc.margins(case))
    assert abs(pc.MARGIN_BAR - 16 * worst_b) <= 0.005 * pc.MARGIN_BAR, (pc.MARGIN_BAR, 16 * worst_b)   # written to three digits
    assert f"{worst_b:.2e}" in pc.__doc__ and f"{pc.MARGIN_BAR:.2e}" in pc.__doc__ and f"{least_a:.2e}" in pc.__doc__
    # random boxes stay small; the large cases are lattices whose IoUs are exact in fp32
    for case in pc.CASES:
        if case.kind == "clusters":
            assert 20 <= pc.reference(case)[2][0] <= 300
        if case.kind in ("lattice", "copies", "max-out", "iou-exact"):
            assert pc.margins(case)["b"] == 0.0, case.name
    assert len({c.name for c in pc.CASES}) == len(pc.CASES)


def test_the_case_list_covers_the_shapes_and_thresholds():
    As = {c.A for c in pc.CASES}
    assert As >= {84, 189, 525, 4116, 1, 63, 65, 255, 257}
    assert {c.conf for c in pc.CASES} >= {0.25, 0.3} and {c.nms for c in pc.CASES} == {0.45, 0.5}
    assert float(F(0.45)) != 0.45 and float(F(0.5)) == 0.5 and float(F(0.3)) != 0.3
    sizes = [len(cs) for *_, cs in pc.launches()]
    assert 1 in sizes and 7 in sizes and max(sizes) == 7 and sum(sizes) == len(pc.CASES)
    for conf, nms, P, max_out, cs in pc.launches():
        raw = pc.stack(cs)
        assert raw.shape == (len(cs), max(c.A for c in cs), 6)
        for n, c in enumerate(cs):                                 # the padding does not pass: same answer at the larger A
            got = pc.run(raw[n], conf, nms, P, max_out)
            assert _same(got, pc.reference(c)), c.name


def test_every_case_reaches_its_branch():
    seen = set()
    for case in pc.CASES:
        raw = pc.build(case)
        ref = pc.reference(case)
        rows, count, (n_pass, n_keep) = ref
        score = raw[:, 4] * raw[:, 5]
        kind = case.kind
        seen.add(kind)
        if kind == "empty":
            assert (count, n_pass, n_keep) == (0, 0, 0)
        elif kind == "last":
            assert n_pass == 1 and score[case.A - 1] >= F(case.conf) and case.A % 256 != 0 and count == 1
        elif kind == "conf-exact":
            on = np.nonzero(score == F(case.conf))[0]
            below = np.nonzero(score == np.nextafter(F(case.conf), F(-1)))[0]
            assert len(on) == 1 and len(below) >= 1 and n_pass == 2
            assert _mutant(case, conf_strict=True)[1] == count - 1
            if case.conf == 0.25:
                assert raw[on[0], 4] == 0.5 and raw[on[0], 5] == 0.5
        elif kind == "clusters":
            assert 20 <= n_pass <= 300 and 2 <= n_keep < n_pass
            chunks = {int(a) // 256 for a in np.nonzero(score >= F(case.conf))[0]}
            assert len(chunks) == (case.A + 255) // 256            # candidates in every chunk of 256 anchors
            # the index order is not the score order
            cand = np.nonzero(score >= F(case.conf))[0]
            assert (np.diff(score[cand]) > 0).any() and (np.diff(score[cand]) < 0).any()
        elif kind == "ties":
            for a0, cnt, _, _ in pc.TIE_GROUPS:
                s = score[a0:a0 + cnt]
                assert bool((s == s[0]).all()) and bool((score == s[0]).sum() == cnt)
                assert a0 < 64 * ((a0 + cnt - 1) // 64) <= a0 + cnt - 1         # a multiple of 64 strictly inside the group
            assert pc.TIE_GROUPS[1][0] < 256 <= pc.TIE_GROUPS[1][0] + pc.TIE_GROUPS[1][1] - 1
            other = _mutant(case, tie_high_index=True)
            assert other[1] == count and not _same(other, ref)     # as many survivors, other boxes
            kept = {tuple(r[:4]) for r in rows}
            for a0, cnt, _, _ in pc.TIE_GROUPS:                    # the lowest index of each group survives, nobody else
                e = pc.xyxy(raw)
                assert tuple(e[a0]) in kept and not any(tuple(e[a0 + t]) in kept for t in range(1, cnt))
            assert score[400] == score[401] and float(raw[400, 4]) * float(raw[400, 5]) < float(raw[401, 4]) * float(raw[401, 5])
            assert tuple(pc.xyxy(raw)[400]) in kept and tuple(pc.xyxy(raw)[401]) not in kept
        elif kind == "iou-exact":
            m = pc.margins(case)
            if case.nms == 0.5:
                assert m["exact"] == 1 and count == 5              # 1/2 and 1/4 kept, 3/4 suppressed
                assert _mutant(case, iou_ge=True)[1] == 4
            else:
                assert m["exact"] == 0 and count == 4              # the same 1/2 is above 0.45
        elif kind == "chain":
            e = pc.xyxy(raw)
            x, y, z = (i for i in np.argsort(-score)[:3])
            iou = lambda p, q: float(pc._iou_row(e, p, np.array([q]), F)[0])
            assert iou(x, y) > case.nms and iou(y, z) > case.nms and iou(x, z) <= case.nms
            assert count == 2 and np.array_equal(rows[:, :4], e[[x, z]])
            assert _mutant(case, dead_suppress=True)[1] == 1       # a dead Y that still suppressed would take Z along
        elif kind == "degenerate":
            m = pc.margins(case)
            assert m["nan"] >= 1 and count == n_pass == 5
            assert int(((rows[:, 2] - rows[:, 0]) * (rows[:, 3] - rows[:, 1]) == 0).sum()) == 4
            assert np.array_equal(rows[0], rows[1]) is False and np.array_equal(rows[0, :4], rows[1, :4])
        elif kind == "clamp":
            e = pc.xyxy(raw)[score >= F(case.conf)]
            assert e[:, 0].min() < 0 and e[:, 1].min() < 0 and e[:, 2].max() > case.P - 1 and e[:, 3].max() > case.P - 1
            assert count == n_pass == 9 and rows[:, :4].min() == 0 and rows[:, :4].max() == case.P - 1
            assert _mutant(case, clamp_first=True)[1] == 7         # either pair collapses to one box when clamped first
            assert len({tuple(r[:4]) for r in rows}) == 7          # both of a pair are written, as the same clamped box
        elif kind == "max-out":
            assert n_pass == n_keep == 100 and count == case.max_out < 100
            assert bool((np.diff(rows[:, 4] * rows[:, 5]) < 0).all())
        elif kind == "lattice":
            n, shadows, _ = case.args
            assert n_pass == n
            if shadows and n >= 3:
                assert n_keep < min(n, pc.DET_CAP)
            if not shadows:
                assert n_keep == n == pc.DET_CAP
            if n > pc.DET_CAP:                                     # the best score of the patch is beyond the cap: dropped
                best = int(np.argmax(score))
                assert best == np.nonzero(score >= F(case.conf))[0][-1]
                assert not bool(((rows[:, 4] == raw[best, 4]) & (rows[:, 5] == raw[best, 5])).any())
        elif kind == "copies":
            assert n_pass == pc.DET_CAP and count == n_keep == 1 and rows[0, 4] * rows[0, 5] == score.max()
        elif kind == "negative":
            assert n_pass == case.A and int((score < 0).sum()) >= 2 and count == case.A
            assert case.A & (case.A - 1) != 0                      # not a power of two: the sort pads
            # a pad of score 0 (for -inf) would outrank them: it lands among the first n_pass slots, as a box that does not exist
            pads = [(0.0, 0x7fffffff)] * ((1 << int(case.A).bit_length()) - case.A)
            order = sorted([(float(s), a) for a, s in enumerate(score)] + pads, key=lambda t: (-t[0], t[1]))
            assert any(a == 0x7fffffff for _, a in order[:n_pass])
    assert seen == {c.kind for c in pc.CASES} and len(seen) == 13
    counts = sorted(c.args[0] for c in pc.CASES if c.kind == "lattice" and c.args[1])
    assert counts == [1, 2, 3, 255, 256, 257, 1023, 1025, 2047, 2048, 2049, 3000]
