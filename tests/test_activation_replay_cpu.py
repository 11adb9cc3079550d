"""Activation replay, host side (no device): the chunk rule the encoder's backward walks (``jn_replay_chunks``), the
config default and the exports."""
import ctypes as C

import pytest

from jolineedle_amd import _lib
from jolineedle_amd.config import model_config

NEW_EXPORTS = ("jn_set_activation_slots", "jn_activation_slots_info", "jn_replay_chunks", "jn_debug_replay_diff")


def _chunks(S, act_slots, g_slots):
    lib = _lib.load_library()
    t0, n = (C.c_int * S)(), (C.c_int * S)()
    count = lib.jn_replay_chunks(S, act_slots, g_slots, t0, n, S)
    assert 0 <= count <= S, (S, act_slots, g_slots, count)
    return [(t0[i], n[i]) for i in range(count)]


def _restated(S, act_slots, g_slots):
    """The rule in the test's own words: chunks of min(act_slots, g_slots) steps in walk order, the last one shorter;
    act_slots = 0 (all resident): today's loop, `for t0 in range(0, S, g_slots)`."""
    size = g_slots if act_slots == 0 else min(act_slots, g_slots)
    return [(t0, min(size, S - t0)) for t0 in range(0, S, size)]


@pytest.mark.parametrize("act_slots", [0, 1, 2, 3, 5, 64])
@pytest.mark.parametrize("g_slots", [1, 2, 4, 64])
def test_replay_chunks_partition_the_walk(act_slots, g_slots):
    for S in range(1, 41):
        got = _chunks(S, act_slots, g_slots)
        assert got == _restated(S, act_slots, g_slots), (S, act_slots, g_slots, got)
        covered = [t for t0, n in got for t in range(t0, t0 + n)]
        assert covered == list(range(S)), (S, act_slots, g_slots, got)            # an exact partition, in walk order
        bound = min(act_slots or S, g_slots)
        assert all(1 <= n <= bound for _, n in got), (S, act_slots, g_slots, got)
        if act_slots == 0:
            assert got == [(t0, min(g_slots, S - t0)) for t0 in range(0, S, g_slots)]


def test_replay_chunks_arguments():
    lib = _lib.load_library()
    t0, n = (C.c_int * 4)(), (C.c_int * 4)()
    assert lib.jn_replay_chunks(0, 2, 2, t0, n, 4) == 0
    assert lib.jn_replay_chunks(10, 2, 4, t0, n, 4) == 5                           # the count, although only `cap` were written
    assert [(t0[i], n[i]) for i in range(4)] == [(0, 2), (2, 2), (4, 2), (6, 2)]
    assert lib.jn_replay_chunks(10, 2, 4, None, None, 0) == 5
    for bad in ((-1, 0, 1), (3, -1, 1), (3, 0, 0)):
        assert lib.jn_replay_chunks(*bad, t0, n, 4) < 0, bad


def test_config_default_keeps_every_step_resident():
    assert model_config().activation_slots == 0


def test_new_exports_are_in_the_signature_table():
    lib = _lib.load_library()
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
