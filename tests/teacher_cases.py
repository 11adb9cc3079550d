"""Seeded teacher states shared by tests/test_teacher_cpu.py and tests/test_gpu_teacher.py: the recorded fixture
(tests/golden/g11_teacher_sets.npz, made by tests/golden/make_golden_teacher.py) and random grids."""
from pathlib import Path

import numpy as np
import torch

G11_PATH = Path(__file__).parent / "golden" / "g11_teacher_sets.npz"


def load_g11():
    g = dict(np.load(G11_PATH))
    return {k: torch.from_numpy(np.asarray(v)) for k, v in g.items()}


def random_states(B, Gh, Gw, n_targets, seed, visited_share=0.4):
    """positions [B,2] int64, visited / targets uint8 [B,Gh,Gw]: `n_targets` random target cells per agent, a share of
    them (and of the other cells: the agent's own trail) visited, the agent's own cell always visited, as in a walk."""
    g = torch.Generator().manual_seed(seed)
    cells = Gh * Gw
    targets = torch.zeros((B, cells), dtype=torch.uint8)
    for b in range(B):
        targets[b, torch.randperm(cells, generator=g)[:min(n_targets, cells)]] = 1
    visited = (torch.rand((B, cells), generator=g) < visited_share).to(torch.uint8)
    pos = torch.stack((torch.randint(0, Gh, (B,), generator=g), torch.randint(0, Gw, (B,), generator=g)), 1)
    visited[torch.arange(B), pos[:, 0] * Gw + pos[:, 1]] = 1
    return pos, visited.view(B, Gh, Gw), targets.view(B, Gh, Gw)
