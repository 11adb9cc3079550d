"""The teacher's action set on the host (jolineedle_amd/trajectory.py::teacher_action_sets) against the sets recorded
from the reference's NeedleSimpleEnv (tests/golden/g11_teacher_sets.npz, made by tests/golden/make_golden_teacher.py)
and against a brute-force restatement on random states.  Host integer logic: runs without a GPU."""
import torch

from jolineedle_amd.common import Action
from jolineedle_amd.trajectory import (move_towards, simple_env_targets, teacher_action_sets, teacher_agreement)
from tests.teacher_cases import load_g11, random_states


def brute_force_set(pos, visited, targets):
    """src/env/simple_env.py:590-629 + 84-125 cell by cell: the nearest (L1) remaining targets, one bit per direction."""
    y, x = int(pos[0]), int(pos[1])
    left = [(qy, qx) for qy in range(targets.shape[0]) for qx in range(targets.shape[1])
            if targets[qy, qx] and not visited[qy, qx]]
    if not left:
        return 0
    best = min(abs(qy - y) + abs(qx - x) for qy, qx in left)
    bits = 0
    for qy, qx in left:
        if abs(qy - y) + abs(qx - x) == best:
            a = move_towards((y, x), (qy, qx))
            if a is not Action.STOP:
                bits |= 1 << a.value
    return bits


def test_fixture_holds_the_cases_it_promises():
    g = load_g11()
    pop = torch.tensor([bin(int(s)).count("1") for s in g["sets"]])
    assert int(((g["n_nearest"] >= 2) & (pop >= 2)).sum()) >= 20
    assert int((g["n_nearest"] == 0).sum()) >= 10
    assert int((g["hw"].min(dim=1).values == 1).sum()) >= 5
    assert int(g["n_nearest"][0]) == 4 and int(g["sets"][0]) == 0b1111          # G8's `ties`: LEFT, RIGHT, UP, DOWN


def test_sets_equal_reference_state_by_state():
    g = load_g11()
    for i in range(len(g["sets"])):
        h, w = (int(v) for v in g["hw"][i])
        got = teacher_action_sets(g["position"][i:i + 1], g["visited"][i:i + 1, :h, :w], g["targets"][i:i + 1, :h, :w])
        assert got.dtype == torch.uint8 and got.shape == (1,)
        assert int(got[0]) == int(g["sets"][i]), (i, h, w, int(got[0]), int(g["sets"][i]))


def test_sets_equal_reference_as_one_padded_batch():
    """All states at once on the 9 x 9 canvas the fixture pads to: cells outside an agent's grid hold no target."""
    g = load_g11()
    assert torch.equal(teacher_action_sets(g["position"], g["visited"], g["targets"]), g["sets"])


def test_target_cells_equal_reference():
    g = load_g11()
    P = int(g["patch_size"])
    for i in range(len(g["sets"])):
        h, w = (int(v) for v in g["hw"][i])
        grid = simple_env_targets(g["boxes"][i, :int(g["n_boxes"][i])], h * P, w * P, P)
        assert torch.equal(grid, g["targets"][i, :h, :w]), i


def test_sets_equal_brute_force_on_random_states():
    n = 0
    for k, (Gh, Gw, nt) in enumerate([(1, 1, 1), (1, 7, 3), (6, 1, 2), (3, 4, 5), (9, 9, 12), (5, 8, 40), (12, 11, 30)]):
        B = 500 // 7 + 1
        pos, visited, targets = random_states(B, Gh, Gw, nt, seed=100 + k)
        if k == 3:
            visited[0] = 1                                        # everything visited
            targets[1] = 0                                        # no target at all
        got = teacher_action_sets(pos, visited, targets)
        for b in range(B):
            assert int(got[b]) == brute_force_set(pos[b], visited[b], targets[b]), (k, b)
        n += B
    assert n >= 500


def test_target_under_the_agent_is_stop_and_sets_no_bit():
    targets = torch.zeros((1, 3, 3), dtype=torch.uint8)
    targets[0, 1, 1] = targets[0, 0, 0] = 1
    got = teacher_action_sets(torch.tensor([[1, 1]]), torch.zeros_like(targets), targets)
    assert int(got[0]) == 0 == brute_force_set((1, 1), torch.zeros((3, 3)), targets[0])


def test_teacher_agreement():
    sets = torch.tensor([0b0001, 0, 0b0110, 0b1000_0000], dtype=torch.uint8)
    assert teacher_agreement(sets, torch.tensor([0, 5, 3, 7])) == 2 / 3          # step 1 has no opinion; step 2 misses
    assert teacher_agreement(sets, torch.tensor([1, 5, 2, 8])) == 1 / 3          # STOP is never a member
    assert teacher_agreement(torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 1, 2, 3])) == 0.0
    assert teacher_agreement(torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.int64)) == 0.0
