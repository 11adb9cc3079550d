"""``jn_teacher_actions`` (one wave per agent, kernels_env.hip) byte for byte against the sets recorded from the reference
(tests/golden/g11_teacher_sets.npz) and against the host function ``trajectory.teacher_action_sets``, which
tests/test_teacher_cpu.py pins to the same fixture and to a brute-force restatement."""
import pytest
import torch

from jolineedle_amd.trajectory import teacher_action_sets, teacher_action_sets_device
from tests.teacher_cases import load_g11, random_states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(pos, visited, targets):
    return teacher_action_sets_device(pos.to(DEV), visited.to(DEV), targets.to(DEV)).cpu()


def test_fixture_one_padded_batch():
    """The 201 recorded states in one launch on the fixture's 9 x 9 canvas (81 cells: the cell loop wraps once)."""
    g = load_g11()
    assert torch.equal(on_device(g["position"], g["visited"], g["targets"]), g["sets"])


def test_fixture_on_each_grid_of_its_own():
    """Every distinct grid size of the fixture as a launch of its own: 1 x 1 up to 9 x 9, rows and columns of one."""
    g = load_g11()
    sizes = sorted({(int(h), int(w)) for h, w in g["hw"]})
    assert (1, 1) in sizes or any(h == 1 for h, _ in sizes)
    for h, w in sizes:
        sel = ((g["hw"][:, 0] == h) & (g["hw"][:, 1] == w)).nonzero().flatten()
        got = on_device(g["position"][sel], g["visited"][sel][:, :h, :w], g["targets"][sel][:, :h, :w])
        assert torch.equal(got, g["sets"][sel]), (h, w)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Gh,Gw,nt", [(1, 1, 1), (1, 9, 3), (7, 1, 2), (3, 4, 5), (8, 8, 9), (9, 9, 20), (40, 50, 300)])
def test_random_grids_equal_host(B, Gh, Gw, nt):
    """Up to 9 x 9 (one pass of the cell loop at 64 cells, two at 81) and 40 x 50 with 300 targets (2000 cells: every
    lane loops 31 or 32 times); B = 1 and B = 5 (a second, partly empty block of four waves)."""
    pos, visited, targets = random_states(B, Gh, Gw, nt, seed=7 * Gh + Gw + B)
    if B == 5:
        visited[1] = 1                                            # an agent with every target visited
        targets[3] = 0                                            # an agent with no target at all
    want = teacher_action_sets(pos, visited, targets)
    if B == 5:
        assert int(want[1]) == 0 and int(want[3]) == 0
    assert torch.equal(on_device(pos, visited, targets), want)


def test_bool_inputs_and_far_targets_only():
    """bool grids are accepted; a single target in the far corner of the large grid is found by the last lane's last
    cell."""
    Gh, Gw = 40, 50
    targets = torch.zeros((2, Gh, Gw), dtype=torch.bool)
    targets[0, Gh - 1, Gw - 1] = True
    targets[1, 0, 0] = True
    visited = torch.zeros_like(targets)
    pos = torch.tensor([[0, 0], [Gh - 1, 0]])
    got = on_device(pos, visited, targets)
    assert got.tolist() == [1 << 7, 1 << 2]                       # RIGHT_DOWN; straight UP
    assert torch.equal(got, teacher_action_sets(pos, visited, targets))
