"""gpt_step_kernel against the bits of a named commit's library (tests/golden/gpt_step_bits.npz, recorded by
tests/golden/make_gpt_step_bits.py): the kernel's scheduling and data movement may change, its floating-point operations,
their operands and their order may not.  Decision-only models (no patch encoder, no atomics): gpt-nano takes the
256-thread form, gpt-mini the 1024-thread form; the full call walks every cache length 0 .. T, the recurrent calls the
given-embedding prefix and the new token at 1-D position 0."""
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
