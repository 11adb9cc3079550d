"""gpt_step_kernel against the bits of a named commit's library (tests/golden/gpt_step_bits.npz, recorded by
tests/golden/make_gpt_step_bits.py): the kernel's scheduling and data movement may change, its floating-point operations,
their operands and their order may not.  Decision-only models (no patch encoder, no atomics): gpt-nano takes the
256-thread form, gpt-mini the 1024-thread form; the full call walks every cache length 0 .. T, the recurrent calls the
given-embedding prefix and the new token at 1-D position 0.
tests/golden/gpt_wide_bits.npz holds the same for the agents-batched route (kernels_gptwide.hip) and whole rollouts on
both routes: the decision behind the head is one function both routes call (gpt_decide_and_step, jn_gpt_device.h), and
the recorded rollouts hold it to what each route's own copy of that block computed in the named commit."""
import importlib.util
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_gpt_step_bits",
                                               Path(__file__).resolve().parent / "golden" / "make_gpt_step_bits.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.mark.parametrize("case", rec.CASES, ids=[rec.case_name(*c) for c in rec.CASES])
def test_gpt_step_bits(golden, case):
    g = golden("gpt_step_bits.npz")
    assert str(g["commit"]), "the fixture names the commit whose library recorded it"
    for run in range(2):                                  # twice: the kernel is deterministic as well as equal
        got = rec.run_case(*case)
        for k, v in got.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(g[k])), (k, run)


def test_gpt_step_bits_when_the_kv_rows_do_not_fit_lds(golden):
    """n_embd 192 at block size 100: the K / V rows of a layer (155 KB) do not fit the workgroup beside the rest, the
    kernel reads them from the cache in global memory — every admitted (n_embd, block_size) runs, with the same bits."""
    g = golden("gpt_step_bits_long.npz")
    for run in range(2):
        got = rec.run_case(*rec.LONG_CASES[0], nb=rec.LONG_B, recurrent=False)
        for k, v in got.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(g[k])), (k, run)


@pytest.mark.parametrize("case", rec.WIDE_CASES, ids=[rec.case_name(*c) for c in rec.WIDE_CASES])
def test_gpt_wide_step_bits(golden, case):
    """The wide route (contexts created under JN_GPT_WIDE=1; rec.build asserts the route): no float atomics, so its
    logits and embeddings are held to the recorded bits like the per-agent kernel's."""
    g = golden("gpt_wide_bits.npz")
    assert str(g["commit"]), "the fixture names the commit whose library recorded it"
    for run in range(2):
        got = rec.run_case(*case, wide=True)
        for k, v in got.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(g[k])), (k, run)


@pytest.mark.parametrize("case", rec.ROLLOUT_CASES, ids=[rec.rollout_name(*c) for c in rec.ROLLOUT_CASES])
def test_decision_rollout_bits(golden, case):
    """A whole rollout on either route — sampled (Philox key, cdf walk), forced (every agent stops at step 2: the skip
    path; ids outside the action range: the clamp) and greedy (first maximum): the actions, positions, masks and rewards
    written, the env state left behind, and the bits of log-probs, entropies and logits."""
    g = golden("gpt_wide_bits.npz")
    for run in range(2):
        got = rec.run_rollout(*case)
        for k, v in got.items():
            assert torch.equal(torch.from_numpy(v), torch.from_numpy(g[k])), (k, run)
