"""The host-side parts of batched inference over images of unequal size that need no device: the grid extents of image
views, the chunking plan of ``infer_images``, the start positions the per-image loop would draw, and the workload of
tools/infer_ab.py."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from jolineedle_amd import ragged
from jolineedle_amd.views import ImageViews

ROOT = Path(__file__).resolve().parent.parent


def test_grid_extents_are_the_rotated_sizes_in_patches():
    P = 64
    srcs = [torch.zeros((3, h, w), dtype=torch.uint8) for h, w in [(64, 128), (65, 127), (100, 300), (1, 1), (192, 64)]]
    views = ImageViews(srcs, rot=[0, 90, 270, 180, 90], patch_size=P)
    ext = views.grid_extents(P)
    assert ext.dtype == torch.int32 and ext.tolist() == [[1, 2], [2, 2], [5, 2], [1, 1], [1, 3]]
    assert views.canvas == (5 * P, 3 * P)
    assert views.grid_extents(32).tolist() == [[2, 4], [4, 3], [10, 4], [1, 1], [2, 6]]
    for kw in ({"ty": [0, 0, 1, 0, 0]}, {"tx": [0, -2, 0, 0, 0]}):
        with pytest.raises(AssertionError):
            ImageViews(srcs, rot=[0, 90, 270, 180, 90], patch_size=P, **kw).grid_extents(P)


def test_plan_chunks_keeps_order_splits_element_types_and_takes_the_smallest_canvas():
    P = 32
    sizes = [(40, 40), (100, 33), (64, 64), (10, 200), (32, 32), (65, 31), (90, 90)]
    u8 = [True, True, False, True, False, False, True]
    images = [torch.zeros((3, h, w), dtype=torch.uint8 if u else torch.float32) for (h, w), u in zip(sizes, u8)]
    plan = ragged.plan_chunks(images, 3, P, max_batch=8)
    assert [c["indices"] for c in plan] == [[0, 1], [2], [3], [4, 5], [6]]
    assert [c["uint8"] for c in plan] == [True, False, True, False, True]
    assert [c["canvas"] for c in plan] == [(128, 64), (64, 64), (32, 224), (96, 32), (96, 96)]
    covered = sorted(i for c in plan for i in c["indices"])
    assert covered == list(range(len(images)))
    for c in plan:
        assert len(c["indices"]) <= 3 and c["indices"] == sorted(c["indices"])
        assert all((images[i].dtype == torch.uint8) == c["uint8"] for i in c["indices"])
    one = ragged.plan_chunks(images[:2], 64, P, max_batch=64)
    assert [c["indices"] for c in one] == [[0, 1]] and one[0]["canvas"] == (128, 64)
    assert ragged.plan_chunks([], 4, P) == []
    with pytest.raises(AssertionError):
        ragged.plan_chunks(images, 9, P, max_batch=8)
    with pytest.raises(AssertionError):
        ragged.plan_chunks(images, 0, P)


def test_stack_inert_pads_with_a_box_that_marks_nothing():
    rows = [torch.tensor([[1, 2, 3, 4]]), torch.zeros((1, 4), dtype=torch.long), torch.tensor([[5, 6, 7, 8], [9, 10, 11, 12]])]
    bb = ragged.stack_inert(rows)
    assert bb.shape == (3, 2, 4) and bb[0, 1].tolist() == list(ragged.INERT_BOX) and bb[1, 0].tolist() == [0, 0, 0, 0]
    from jolineedle_amd.detection import split_bboxes_over_patches
    _, masks = split_bboxes_over_patches(bb, 2, 2, 8)
    assert not bool(masks[0, :, :, 1].any()) and bool(masks[1, 0, 0, 0]) and not bool(masks[1, :, :, 1].any())


def test_loop_start_positions_follow_the_engines_reset_draw():
    from oracle.dropout_ref import philox4x32

    class Tr:
        seed = 7
    ext = [[3, 5], [1, 2], [10, 10]]
    got = ragged.loop_start_positions(Tr, 4, [0, 2, 5], ext)
    for (i, (gh, gw)), row in zip(zip([0, 2, 5], ext), got.tolist()):
        seed = 7 * 1000003 + 4 + i
        r = philox4x32(seed, *[np.array([c], dtype=np.uint32) for c in (0, 0, 0x52455345, 0)])
        assert row == [int(r[0][0]) % gh, int(r[1][0]) % gw]


def test_chunk_walks_lay_out_the_walks_of_two_chunks_as_the_per_image_loop_numbers_them():
    """Three images in two chunks (batch_size 2), K = 2, seed 1, first rollout 4, classes [5, 9, 7]: per chunk the
    agent -> image map, the classes, the keys of every (mode, streams) pair and the starts; then the final counter."""
    class Tr:
        seed = 1
    P, K, first, class_ids = 64, 2, 4, [5, 9, 7]
    images = [torch.zeros((3, h, w)) for h, w in [(100, 200), (64, 64), (130, 70)]]
    plan = ragged.plan_chunks(images, 2, P, ragged.images_per_chunk(8, K))
    assert [c["indices"] for c in plan] == [[0, 1], [2]]
    assert ragged.images_per_chunk(8, K) == 4 and ragged.images_per_chunk(8, 1) == 8 and ragged.images_per_chunk(None, K) is None
    ext = ImageViews(images, patch_size=P).grid_extents(P).tolist()
    assert ext == [[2, 4], [1, 1], [3, 2]]
    want = [([0, 1, 2, 3], [0, 0, 1, 1], [5, 5, 9, 9]), ([4, 5], [2, 2], [7, 7])]
    for chunk, (sel, image_of, classes) in zip(plan, want):
        idx = chunk["indices"]
        e = [ext[i] for i in idx]
        for sample, streams in ((True, "loop"), (True, "batch"), (False, "loop"), (False, "batch")):
            got = ragged.chunk_walks(Tr, first, idx, e, K, sample, streams, class_ids)
            assert got["sel"] == sel and got["image_of"] == image_of
            assert got["classes"] == classes == ragged.walk_classes(class_ids, idx, K)
            if sample and streams == "loop":
                keys = ragged.walk_agent_keys(Tr, first, idx, K)
                assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], keys)
                assert keys.tolist() == [[1 * 1000003 + first + a, 0] for a in sel]
            else:
                assert got["keys"] is None
            starts = ragged.loop_start_positions(Tr, first, sel, [x for x in e for _ in range(K)])
            assert got["starts"].dtype == torch.int64 and torch.equal(got["starts"], starts)
        assert ragged.chunk_walks(Tr, first, idx, e, K)["classes"] is None
        given = ragged.chunk_walks(Tr, first, idx, e, K, walk_starts=lambda f, i, x: torch.full((len(i), K, 2), 7))
        assert given["starts"].tolist() == [[7, 7]] * len(sel)
    assert ragged.rollouts_after(first, len(images), K) == first - 1 + 3 * 2 == 9


def test_own_steps_and_slices_of_a_batched_rollout():
    masks = torch.tensor([[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]], dtype=torch.bool)
    ro = {"masks": masks, "rewards": torch.arange(12.).reshape(3, 4), "positions": torch.zeros((3, 5, 2), dtype=torch.long),
          "bboxes": [[] for _ in range(3)], "patches": None}
    assert ragged.own_steps(ro) == [4, 2, 1]
    s = ragged.slice_rollout(ro, 1, 2)
    assert s["masks"].tolist() == [[True, True, False]] and s["rewards"].tolist() == [[4., 5.]] and s["positions"].shape == (1, 3, 2)
    assert s["bboxes"] == [[]] and s["patches"] is None


def test_infer_ab_help_and_toy_workload():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "infer_ab.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--images" in r.stdout and "--step-timeout" in r.stdout
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import infer_ab
    finally:
        sys.path.pop(0)
    images, boxes = infer_ab.make_workload(6, 16, 3, 10, seed=1)
    again, _ = infer_ab.make_workload(6, 16, 3, 10, seed=1)
    assert len(images) == len(boxes) == 6 and all(torch.equal(a, b) for a, b in zip(images, again))
    assert len({tuple(im.shape) for im in images}) > 1
    for im, bb in zip(images, boxes):
        assert im.dtype == torch.uint8 and im.shape[0] == 3
        h, w = im.shape[1:]
        assert 2 * 16 < h <= 10 * 16 and 2 * 16 < w <= 10 * 16
        assert 1 <= len(bb) <= 3 and bool((bb[:, 0] <= bb[:, 2]).all()) and bool((bb[:, 2] < w).all()) and bool((bb[:, 3] < h).all())
    assert images[0].shape[1] <= 3 * 16 and images[1].shape[1] > 9 * 16
