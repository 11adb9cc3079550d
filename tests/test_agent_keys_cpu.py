"""Per-agent random streams without a GPU: the export (``jn_set_rollout_keys``) and its refusals, the host tables the
batched helpers hand to it (``ragged.loop_agent_keys`` / ``walk_agent_keys``, ``dist.shard_agent_keys``) against
hand-written seeds, and the tie between an agent's stream and the start position the batched helpers inject."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from jolineedle_amd import _lib, dist, ragged
from jolineedle_amd.engine import make_jn_config
from tests.helpers import model_config

M64 = 0xFFFFFFFFFFFFFFFF


def test_header_declares_and_library_exports_the_setter():
    lib = _lib.load_library()
    assert lib.jn_abi_version() == 2 == _lib.ABI_VERSION
    res, args = _lib.SIGNATURES["jn_set_rollout_keys"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int]
    fn = lib.jn_set_rollout_keys
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    header = (_lib.LIB_PATH.parents[2] / "include" / "jnroll.h").read_text()
    assert "int jn_set_rollout_keys(jn_ctx* ctx, const uint64_t* keys_host, int n);" in header
    assert "#define JN_ABI_VERSION 2" in header


@pytest.fixture()
def ctx():
    lib = _lib.load_library()
    cfg = make_jn_config(model_config(patch_size=64, block_size=6, image_processor=None, with_detector=False), 0, 8, 9)
    h = C.c_void_p()
    assert lib.jn_create(C.byref(cfg), C.byref(h)) == 0, lib.jn_last_error()
    yield lib, h
    lib.jn_destroy(h)


def _table(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).reshape(-1, 2))


def test_setter_refuses_bad_tables_and_disarms(ctx):
    """Every refusal comes before any device call (this machine has no device), and a refused table leaves nothing armed
    that a later call would trip over."""
    lib, h = ctx
    call = lambda handle, tab, n: lib.jn_set_rollout_keys(handle, None if tab is None else tab.ctypes.data_as(C.c_void_p), n)
    good = _table([[7, 0], [M64, 0xFFFFFFFF], [0, 3]])           # a 64-bit seed, the largest stream index
    assert call(h, good, 3) == 0, lib.jn_last_error()
    assert call(None, good, 3) == -1                              # a null ctx
    assert b"jn_set_rollout_keys" in lib.jn_last_error()
    assert call(None, None, 0) == -1
    assert call(h, good, 0) == -1 and call(h, good, -2) == -1     # n < 1 with a table
    for bad_at in range(3):                                       # a stream index >= 2^32, wherever it stands
        rows = good.copy()
        rows[bad_at, 1] = 1 << 32
        assert call(h, rows, 3) == -1
        assert b"32 bits" in lib.jn_last_error()
    assert call(h, _table([[1, M64]]), 1) == -1
    assert call(h, good, 1) == 0                                  # a prefix of a table is a table
    assert call(h, None, 0) == 0 and call(h, None, 5) == 0        # disarming, n ignored; twice is fine
    assert call(h, good, 3) == 0 and call(h, None, 0) == 0


def _trainer(seed):
    return SimpleNamespace(seed=seed)


def test_loop_agent_keys_against_hand_written_seeds():
    # the seed of rollout r of a trainer seeded s is (s * 1000003 + r) mod 2^64 (ReinforceTrainer.rollout)
    got = ragged.loop_agent_keys(_trainer(1), 1, [0, 1, 4])
    assert got.dtype == np.uint64 and got.shape == (3, 2)
    assert got.tolist() == [[1000004, 0], [1000005, 0], [1000008, 0]]
    assert ragged.loop_agent_keys(_trainer(3), 10, [2]).tolist() == [[3000021, 0]]
    assert ragged.loop_agent_keys(_trainer(0), 1, [5, 0]).tolist() == [[6, 0], [1, 0]]         # in the order of `indices`
    # a seed that wraps: 2^61 * 1000003 = 2^61 * (8 * 125000 + 3) = 3 * 2^61 mod 2^64
    assert ragged.loop_agent_keys(_trainer(1 << 61), 1, [0]).tolist() == [[(3 << 61) + 1, 0]]
    assert ragged.loop_agent_keys(_trainer(1), 1, []).shape == (0, 2)
    assert ragged.rollout_seed(_trainer(1), 7) == 1000010


def test_walk_agent_keys_against_hand_written_seeds():
    # K = 3 walks of images 0 and 2 from rollout 1 on: walk (i, k) is rollout 1 + 3 i + k in every mode
    got = ragged.walk_agent_keys(_trainer(1), 1, [0, 2], 3)
    assert got.tolist() == [[1000004, 0], [1000005, 0], [1000006, 0], [1000010, 0], [1000011, 0], [1000012, 0]]
    assert ragged.walk_agent_keys(_trainer(1), 1, [0, 1, 4], 1).tolist() == ragged.loop_agent_keys(_trainer(1), 1, [0, 1, 4]).tolist()
    # "rollouts" mode: one start per image (walk 0's), K streams
    starts = ragged.walk_start_positions(_trainer(1), 1, [0, 2], [(3, 4), (2, 5)], 3, "rollouts")
    assert starts.shape == (2, 3, 2) and bool((starts == starts[:, :1]).all())
    assert len({tuple(k) for k in got.tolist()}) == 6


@pytest.mark.parametrize("seed,first", [(1, 1), (5, 40), ((1 << 63) + 12345, 3)])
def test_draw_0_of_the_reset_stream_is_the_loop_start_position(seed, first):
    """What the engine draws for an armed agent without start_positions — Philox(key[0], ((uint32) key[1], 0, "RESE", 0))
    modulo its own extent — on the host mirror: the position ``loop_start_positions`` injects."""
    tr = _trainer(seed)
    idx = [0, 3, 1, 6]
    extents = [(2, 3), (4, 4), (1, 7), (5, 2)]
    keys = ragged.loop_agent_keys(tr, first, idx).tolist()
    want = ragged.loop_start_positions(tr, first, idx, extents).tolist()
    got = []
    for (k, i), (gh, gw) in zip(keys, extents):
        r = ragged._philox4x32(k, i & 0xFFFFFFFF, 0, 0x52455345, 0)
        got.append([r[0] % gh, r[1] % gw])
    assert got == want
    assert all(0 <= y < gh and 0 <= x < gw for (y, x), (gh, gw) in zip(got, extents))
    # and the walks of the multistart evaluation: walk (i, k) starts at draw 0 of ITS stream
    K = 2
    wk = ragged.walk_agent_keys(tr, first, [0, 1], K).tolist()
    ws = ragged.walk_start_positions(tr, first, [0, 1], [(3, 4), (2, 5)], K, "multistart").reshape(-1, 2).tolist()
    ext = [(3, 4), (3, 4), (2, 5), (2, 5)]
    for (k, i), (gh, gw), w in zip(wk, ext, ws):
        r = ragged._philox4x32(k, i, 0, 0x52455345, 0)
        assert [r[0] % gh, r[1] % gw] == w


def test_philox_mirror_known_answer():
    # Philox4x32-10, counter 0, key 0 (Random123 known-answer test)
    assert ragged._philox4x32(0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def test_shard_agent_keys_are_disjoint_and_do_not_depend_on_the_world_size():
    seed, number, G = 3, 17, 16
    rs = 3 * 1000003 + 17
    whole = []
    for world in (1, 2, 8):
        B = G // world
        shards = [dist.shard_agent_keys(seed, number, rank, world, B) for rank in range(world)]
        for s in shards:
            assert s.dtype == np.uint64 and s.shape == (B, 2)
        rows = [tuple(r) for s in shards for r in s.tolist()]
        assert len(set(rows)) == G                                 # no stream twice, within a rank or across ranks
        whole.append(rows)
    assert whole[0] == whole[1] == whole[2] == [(rs, g) for g in range(G)]
    assert dist.shard_agent_keys(seed, number, 1, 2, 8).tolist()[0] == [rs, 8]
    # another rollout, another seed: other streams
    assert dist.shard_agent_keys(seed, number + 1, 0, 1, 2).tolist() == [[rs + 1, 0], [rs + 1, 1]]
    assert dist.shard_agent_keys(1 << 61, 1, 0, 1, 1).tolist() == [[(3 << 61) + 1, 0]]          # modulo 2^64
    with pytest.raises(AssertionError):
        dist.shard_agent_keys(seed, number, 2, 2, 4)
