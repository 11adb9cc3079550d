"""``trajectory.teacher_walks`` — the host statement of the rule ``jn_teacher_walks`` computes, written on plain integers —
against ``NeedleSimpleEnv.generate_sample_indices`` (pinned to the reference by golden G8) drawing from ``PhiloxDraws`` of the
same (seed, image).  Inputs: tests/teacher_walk_cases.py."""
import numpy as np
import pytest
import torch

from jolineedle_amd import trajectory as tj
from tests import teacher_walk_cases as tw

WALK_KEYS = ("positions", "current_actions", "next_actions", "labels", "masks", "local_bboxes")


def _env_walk(case, b, T, record=None):
    """Image b of `case` walked by the env with both random sources replaced; `record` collects (keypoints, detours)."""
    bb = case["bboxes"][b]
    real = bb[(bb != 0).any(dim=-1)] if bb.numel() else bb.reshape(0, 4)
    P = case["P"]
    env = tj.NeedleSimpleEnv(None, P, real, height=case["gh"] * P, width=case["gw"] * P,
                             py_random=tj.PhiloxDraws(case["seed"], b, tj.WALK_TAG_Y))
    env.rng = tj.PhiloxDraws(case["seed"], b, tj.WALK_TAG_R)
    if record is not None:
        build, uniform, binomial = env.build_keypoints_trajectory, env.generate_keypoints, env.generate_binomial_keypoints

        def keypoints():
            record["keypoints"] = build()
            record["random"] = not (env.bbox_patches - env.visited_bbox_patches) and len(record["keypoints"]) == 1
            return record["keypoints"]

        def detours(*a):
            pts = (binomial if len(a) == 2 else uniform)(*a)
            if "keypoints" in record:                    # (the keypoint drawn inside build_keypoints_trajectory is not a detour)
                record.setdefault("detours", []).extend(pts)
            return pts

        env.build_keypoints_trajectory, env.generate_keypoints, env.generate_binomial_keypoints = keypoints, detours, detours
    start = None if case["start_positions"] is None else tuple(int(v) for v in case["start_positions"][b])
    return env.generate_sample_indices(T, case["min_keypoints"], case["max_keypoints"], case["binomial_keypoints"], start), real


@pytest.mark.parametrize("name", list(tw.CASES))
def test_teacher_walks_equal_the_env_on_philox_draws(name):
    case = tw.CASES[name]
    got = tj.teacher_walks(**case)
    B, nb = case["bboxes"].shape[:2]
    gh, gw, P, T = case["gh"], case["gw"], case["P"], case["T"]
    assert got["offsets"].dtype == torch.int32 and got["n_steps"].dtype == torch.int32 and got["targets"].dtype == torch.uint8
    assert got["cells_yolox"].shape == (int(got["offsets"][B]), 3) and got["bboxes_yolox"].shape == (int(got["offsets"][B]), nb, 6)
    for b in range(B):
        want, real = _env_walk(case, b, T)
        n_real = real.shape[0]
        for k in WALK_KEYS:
            g = got[k][b].numpy()
            if k == "local_bboxes":
                assert not g[:, n_real:].any(), (name, b, "columns past the real boxes")
                g = g[:, :n_real]
            assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (name, b, k)
        # the untruncated length: the same walk with room for every step
        long, _ = _env_walk(case, b, (gh * gw + case["max_keypoints"] + 1) * max(gh, gw) + 1)
        assert int(got["n_steps"][b]) == int(long["masks"].sum()), (name, b)
        assert np.array_equal(got["masks"][b].numpy(), (np.arange(T) < min(int(got["n_steps"][b]), T)).astype(np.float32))
        assert torch.equal(got["targets"][b], tj.simple_env_targets(real, gh * P, gw * P, P)), (name, b)
        # detector rows, as a mapping cell -> boxes (the env lists a Python set)
        lo, hi = int(got["offsets"][b]), int(got["offsets"][b + 1])
        cells = got["cells_yolox"][lo:hi]
        assert bool((cells[:, 0] == b).all())
        mine = {(int(y), int(x)): got["bboxes_yolox"][lo + i].numpy() for i, (_, y, x) in enumerate(cells)}
        assert len(mine) == hi - lo == want["positions_yolox"].shape[0], (name, b)
        for (y, x), boxes in zip(want["positions_yolox"], want["bboxes_yolox"]):
            assert np.array_equal(mine[(int(y), int(x))][:n_real], boxes) and not mine[(int(y), int(x))][n_real:].any(), (name, b)
        # targets in row-major order, then the one negative
        tg = [(int(y), int(x)) for y, x in torch.nonzero(got["targets"][b])]
        assert [tuple(c) for c in cells[:len(tg), 1:].tolist()] == tg and hi - lo == len(tg) + (len(tg) < gh * gw), (name, b)


def test_the_cases_reach_what_they_are_named_for():
    rec = {}
    _env_walk(tw.CASES["three_detours"], 0, 64, rec)
    kp = rec["keypoints"]
    assert len(rec["detours"]) == 3
    # a detour lands on a keypoint that is still to come when it is walked: it is passed over and visited again later
    got = tj.teacher_walks(**tw.CASES["three_detours"])
    walked = [tuple(p) for p in got["positions"][0, :int(got["n_steps"][0])].tolist()]
    assert any(d in kp and walked.index(d) < len(walked) - 1 - walked[::-1].index(d) for d in rec["detours"])
    rec = {}
    _env_walk(tw.CASES["grid_1x1"], 0, 4, rec)
    assert rec["keypoints"] == [(0, 0)] and rec["random"]
    t = tj.teacher_walks(**tw.CASES["ring_wrap"])
    assert bool((t["n_steps"] > tw.CASES["ring_wrap"]["T"]).all())
    t = tj.teacher_walks(**tw.CASES["zero_tail"])
    assert 1 < int(t["n_steps"][0]) < tw.CASES["zero_tail"]["T"] and float(t["masks"][0, -1]) == 0.0
    t = tj.teacher_walks(**tw.CASES["area_exactly_a_twentieth"])
    assert int(t["targets"][0, 0, 0]) == 0 and int(t["targets"][1, 0, 0]) == 1
    t = tj.teacher_walks(**tw.CASES["ties_8x8"])
    other = tj.teacher_walks(**{**tw.CASES["ties_8x8"], "seed": tw.CASES["ties_8x8"]["seed"] + 1})
    assert not torch.equal(t["positions"], other["positions"])
    again = tj.teacher_walks(**tw.CASES["ties_8x8"])
    assert all(torch.equal(t[k], again[k]) for k in t)
    assert tw.CASES["grid_64x64"]["gh"] * tw.CASES["grid_64x64"]["gw"] == tj.MAX_WALK_CELLS


def test_start_positions_outside_the_grid_are_refused():
    case = dict(tw.CASES["start_inside_a_box"])
    for bad in ([[4, 0]], [[0, 5]], [[-1, 0]]):
        with pytest.raises(AssertionError):
            tj.teacher_walks(**{**case, "start_positions": torch.tensor(bad)})


def test_area_rule_on_integers():
    """h * w / P**2 > 0.05 (the env's float test) is 20 * h * w > P * P, for every area a cell can hold."""
    for P in range(1, 65):
        for hw in range(0, P * P + 1):
            assert (hw / (P ** 2) > 0.05) == (20 * hw > P * P), (P, hw)


def test_binomial_is_a_bit_count():
    d = tj.PhiloxDraws(5, 0, tj.WALK_TAG_R)
    draws = [d.binomial(10, 0.5) for _ in range(2000)]
    assert d.k == 2000 and all(0 <= v <= 10 for v in draws)
    assert abs(sum(draws) / 2000 - 5) <= 0.25                 # sigma / sqrt(N) = 0.035: a bug catcher, not a statistical test
    d = tj.PhiloxDraws(5, 1, tj.WALK_TAG_R)
    assert 0 <= d.binomial(40) <= 40 and d.k == 2 and d.binomial(64) <= 64 and d.k == 4 and d.binomial(65) <= 65 and d.k == 7
    from jolineedle_amd.ragged import _philox4x32
    e = tj.PhiloxDraws(5, 1, tj.WALK_TAG_R)
    r0, r1 = (_philox4x32(5, 1, k, tj.WALK_TAG_R, 0)[0] for k in (0, 1))
    assert e.binomial(40) == bin(r0).count("1") + bin(r1 & 0xFF).count("1")
    assert e.integers(3, 9) == 3 + _philox4x32(5, 1, 2, tj.WALK_TAG_R, 0)[0] % 6
    assert len(e.integers(0, 4, size=0)) == 0 and e.k == 3
    assert e.choice([(2, 1), (0, 5), (1, 7)]) == sorted([(2, 1), (0, 5), (1, 7)])[_philox4x32(5, 1, 3, tj.WALK_TAG_R, 0)[0] % 3]
