"""Class-conditioned rollouts without a GPU: the export (``jn_set_rollout_classes``) and its refusals, the Python
wrappers' own check of the ids (before any engine call), the mapping of image classes to walks, and — on the oracle
alone — the precondition of tests/test_gpu_class_rollout.py: the class ids it uses move the rollout's logits by at least
1e-2, a hundred times its eval logit bar, so that a walk under the wrong row of ``embed_class`` cannot pass."""
import ctypes as C
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, ragged
from jolineedle_amd.engine import make_jn_config
from jolineedle_amd.reinforce import _classes_table
from tests import class_rollout_ref as ref
from tests.helpers import model_config


def test_header_declares_and_library_exports_the_setter():
    lib = _lib.load_library()
    assert lib.jn_abi_version() == 2 == _lib.ABI_VERSION                       # an added export: the ABI stays
    res, args = _lib.SIGNATURES["jn_set_rollout_classes"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int]
    fn = lib.jn_set_rollout_classes
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    header = (_lib.LIB_PATH.parents[2] / "include" / "jnroll.h").read_text()
    assert "int jn_set_rollout_classes(jn_ctx* ctx, const int64_t* classes_host, int n);" in header
    assert "src/supervised.py:284, 317-331, 663-687" in header


@pytest.fixture()
def ctx():
    lib = _lib.load_library()
    cfg = make_jn_config(model_config(patch_size=64, block_size=6, image_processor=None, with_detector=False), 0, 8, 9)
    h = C.c_void_p()
    assert lib.jn_create(C.byref(cfg), C.byref(h)) == 0, lib.jn_last_error()
    yield lib, h
    lib.jn_destroy(h)


def test_setter_takes_valid_ids_refuses_bad_tables_and_disarms(ctx):
    """Every refusal comes before any device call (this machine has no device) and names the agent and the id."""
    lib, h = ctx

    def call(handle, ids, n=None):
        tab = None if ids is None else np.ascontiguousarray(np.array(ids, dtype=np.int64))
        return lib.jn_set_rollout_classes(handle, None if tab is None else tab.ctypes.data_as(C.c_void_p), len(ids) if n is None else n)

    assert call(h, [0, 3, 99]) == 0, lib.jn_last_error()
    for ids, agent, bad in (([0, 3, 100], 2, 100), ([-1, 3, 99], 0, -1), ([0, 1 << 40, 5], 1, 1 << 40)):
        assert call(h, ids) == -1
        err = lib.jn_last_error().decode()
        assert "jn_set_rollout_classes" in err and f"agent {agent}" in err and f", {bad}," in err, err
    assert call(h, [0, 3, 99], 0) == -1 and call(h, [0, 3, 99], -2) == -1      # n < 1 with a table
    assert b"n = " in lib.jn_last_error()
    assert call(None, [0, 3, 99]) == -1 and call(None, None, 0) == -1          # a null ctx
    assert call(h, None, 0) == 0 and call(h, None, 5) == 0                     # NULL clears, n ignored; twice is fine
    assert call(h, [99]) == 0 and call(h, None, 0) == 0


def test_classes_table_takes_tensors_and_sequences_and_raises_what_gpt_forward_raises():
    for ids in ([3, 99, 0], torch.tensor([3, 99, 0]), torch.tensor([3, 99, 0], dtype=torch.int32), np.array([3, 99, 0]), (3, 99, 0)):
        tab = _classes_table(ids, 3)
        assert tab.dtype == np.int64 and tab.flags["C_CONTIGUOUS"] and tab.tolist() == [3, 99, 0]
    for bad in ([0, 100, 1], [-1, 0, 1], torch.tensor([0, 1, 100])):
        with pytest.raises(AssertionError, match="class id outside embed_class"):
            _classes_table(bad, 3)
    with pytest.raises(AssertionError, match=r"classes must be \[3\]"):
        _classes_table([1, 2], 3)


class _NoEngine:
    """A model whose every engine-side attribute is an error: the wrappers must have checked the ids before."""
    patch_size, device, max_batch = 64, torch.device("cpu"), 8
    config = SimpleNamespace(no_recurrent_embedding=False)
    training = False

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __getattr__(self, name):
        raise RuntimeError(f"the engine was reached ({name})")


def test_wrappers_raise_for_id_100_before_any_engine_call():
    cfg = ja.CfgNode(max_seq_len=4, entropy_weight=0.01, stop_enabled=True, reward_norm=False, seed=1, patch_size=64)
    tr = ja.ReinforceTrainer(cfg, _NoEngine())
    env = SimpleNamespace(batch_size=3)
    images = [torch.zeros((3, 100, 100), dtype=torch.uint8)] * 3
    boxes = [torch.zeros((0, 4), dtype=torch.long)] * 3
    with pytest.raises(RuntimeError, match="the engine was reached"):          # the stub works: valid ids go on to the engine
        tr.rollout(env, classes=[0, 3, 99])
    calls = [lambda: tr.rollout(env, classes=[0, 100, 3]), lambda: tr.rollout(env, classes=torch.tensor([0, 3, -1])),
             lambda: tr.train_iteration(env, classes=[0, 100, 3]),
             lambda: tr.eval_on_images(images, boxes, 2, class_ids=[0, 100, 3]),
             lambda: list(ragged.rollout_chunks(tr, images, boxes, 2, walks=2, class_ids=[0, 100, 3])),
             lambda: ja.infer_images(tr, images, class_ids=[0, 100, 3]),
             lambda: ja.infer_images(tr, images, batch_size=2, class_ids=[0, 100, 3])]
    sup = ja.SupervisedTrainer(ja.CfgNode(patch_size=64, max_seq_len=4, stop_enabled=True, seed=1), _NoEngine())
    calls += [lambda: sup.eval_on_images(images, boxes, 2, do_detection=False, class_ids=[0, 100, 3])]
    for f in calls:
        with pytest.raises(AssertionError, match="class id outside embed_class"):
            f()
    with pytest.raises(AssertionError, match="one class per image"):
        tr.eval_on_images(images, boxes, 2, class_ids=[0, 1])


def test_image_classes_reach_every_walk_of_their_image():
    assert ragged.walk_classes([5, 9], [0, 1], 2) == [5, 5, 9, 9]              # K = 2: [c0, c0, c1, c1]
    assert ragged.walk_classes([5, 9, 7, 2], [3, 1], 3) == [2, 2, 2, 9, 9, 9]  # a chunk's own images, in its order
    assert ragged.walk_classes([5, 9, 7], [2, 0]) == [7, 5]
    assert ragged.walk_classes(None, [0, 1], 2) is None
    assert ragged.image_classes(None, 4) is None
    assert ragged.image_classes(torch.tensor([3, 99, 0]), 3) == [3, 99, 0]
    assert ragged.image_classes((0, 99), 2) == [0, 99]


def test_class_tokens_is_off_by_default():
    from jolineedle_amd.config import args_to_config, get_args
    t, _ = args_to_config(get_args([]))
    assert t.class_tokens is False


# ---- the oracle alone: the ids of the GPU tests move the logits -------------------------------------------------------
@pytest.mark.parametrize("sequence", [False, True], ids=["recurrent", "sequence"])
@pytest.mark.parametrize("name", list(ref.DIMS))
def test_the_chosen_class_ids_move_the_logits_of_the_rollout(name, sequence):
    """Forced rollouts of the GPU tests' batch on the oracle under each of the ids in use: for every agent, any two
    different ids leave logits at least 1e-2 apart (largest distance over the steps and actions) — a walk under a wrong
    row, 0 included, sits 100 bars from the right one."""
    oracle = ref.decision_oracle(name, sequence)
    ids = sorted(set(ref.CLASS_IDS) | {7})
    with torch.no_grad():
        logits = {c: ref.forced_rollout(oracle, [c] * ref.B)["logits"] for c in ids}
    worst = min(float((logits[a][b] - logits[c][b]).abs().max()) for a, c in itertools.combinations(ids, 2) for b in range(ref.B))
    print(f"{name} {'sequence' if sequence else 'recurrent'}: the closest two classes leave logits {worst:.3e} apart")
    assert worst >= ref.MOVE_BAR, worst


def test_the_chosen_class_ids_move_the_train_mode_logits():
    oracle = ref.decision_oracle("gpt-nano")
    try:
        oracle.train()
        import copy
        with torch.no_grad():
            a = ref.forced_rollout(copy.deepcopy(oracle), ref.CLASS_IDS, stop_early=True)["logits"]
            z = ref.forced_rollout(copy.deepcopy(oracle), [0] * ref.B, stop_early=True)["logits"]
    finally:
        oracle.eval()
    d = [float((a[b] - z[b]).abs().max()) for b in range(ref.B)]
    print("train-mode logits, table against zeros, per agent:", d)
    assert d[0] >= ref.MOVE_BAR and d[1] >= ref.MOVE_BAR and d[2] == 0.0      # (class 0 stays class 0: BatchNorm sees patches only)


def test_the_image_classes_move_the_greedy_walks_and_leave_no_near_tie():
    """The evaluation / inference tests compare greedy walks of one engine at several batch sizes: on the oracle, under
    the image's class, every decision from every start cell has a top-2 gap of at least 1e-3 (the precondition of the
    ragged-batch tests, ``ragged_ref.LOGIT_GAP``: five times the 2e-4 bar between two batch sizes, so no argmax can
    flip), and the image's class moves the first decision's logits by at least 1e-2 against class 0."""
    oracle, images = ref.detector_oracle()
    worst_gap, moved = float("inf"), []
    for (im, boxes), c in zip(images, ref.IMAGE_CLASS_IDS):
        gh, gw = -(-im.shape[-2] // ref.P), -(-im.shape[-1] // ref.P)
        for y in range(gh):
            for x in range(gw):
                w = ref.greedy_walk(oracle, im, boxes, (y, x), c)
                worst_gap = min(worst_gap, w["gap"])
                if c != 0:
                    z = ref.greedy_walk(oracle, im, boxes, (y, x), 0)
                    moved.append(float((w["logits"][0] - z["logits"][0]).abs().max()))
    print(f"smallest top-2 gap {worst_gap:.3e}; first-step logits moved by at least {min(moved):.3e}")
    assert worst_gap >= ref.GAP, worst_gap
    assert min(moved) >= ref.MOVE_BAR, moved
