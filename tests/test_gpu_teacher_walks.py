"""``jn_teacher_walks`` (csrc/kernels_env.hip) against its host statement ``trajectory.teacher_walks``, bit for bit on every
output of every case of tests/teacher_walk_cases.py; the entry point's refusals; the device route of
``SupervisedTrainer.generate_trajectories`` and one training iteration with ``config.device_trajectories``."""
from types import SimpleNamespace

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib
from jolineedle_amd import trajectory as tj
from jolineedle_amd._lib import ptr
from tests import teacher_walk_cases as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("positions", "current_actions", "next_actions", "labels", "masks", "local_bboxes", "n_steps", "targets",
         "cells_yolox", "bboxes_yolox", "offsets")
FILL = 93                                  # the sentinel: no output of these cases holds it (coordinates stay below it)


def _raw_call(case, fill=FILL, **over):
    """One ``jn_teacher_walks`` into buffers filled with `fill` (detector rows: B * gh * gw); returns (rc, buffers)."""
    a = dict(case)
    a.update(over)
    bb = a["bboxes"].to(DEV).contiguous()
    B, nb = (int(v) for v in bb.shape[:2])
    B = a.get("B", B)
    gh, gw, T = a["gh"], a["gw"], a["T"]
    rows, Tn = max(1, bb.shape[0] * max(case["gh"], 1) * max(case["gw"], 1)), max(case["T"], 1)
    nB = max(bb.shape[0], 1)
    f = lambda shape, dt: torch.full(shape, fill, device=DEV, dtype=dt)
    buf = {"positions": f((nB, Tn, 2), torch.int64), "current_actions": f((nB, Tn), torch.int64),
           "next_actions": f((nB, Tn), torch.int64), "labels": f((nB, Tn), torch.int64), "masks": f((nB, Tn), torch.float32),
           "local_bboxes": f((nB, Tn, max(nb, 1), 6), torch.float32), "n_steps": f((nB,), torch.int32),
           "targets": f((nB, case["gh"], case["gw"]), torch.uint8), "cells_yolox": f((rows, 3), torch.int64),
           "bboxes_yolox": f((rows, max(nb, 1), 6), torch.float32), "offsets": f((nB + 1,), torch.int32)}
    starts = None if a["start_positions"] is None else a["start_positions"].to(DEV).contiguous()
    for k in a.get("null", ()):
        buf[k] = None
    rc = _lib.load_library().jn_teacher_walks(
        None if "bboxes" in a.get("null", ()) else ptr(bb), ptr(starts), B, a.get("nb", nb), gh, gw, a["P"], T,
        a["min_keypoints"], a["max_keypoints"], int(a["binomial_keypoints"]), a["seed"] & (2 ** 64 - 1), a.get("capacity", rows),
        *(ptr(buf[k]) for k in NAMES), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, buf


@pytest.fixture(scope="module")
def host_walks():
    """The host statement of every case, computed once."""
    return {name: tj.teacher_walks(**case) for name, case in tw.CASES.items()}


@pytest.mark.parametrize("name", list(tw.CASES))
def test_device_equals_host_bit_for_bit(name, host_walks):
    case, want = tw.CASES[name], host_walks[name]
    B, nb = case["bboxes"].shape[:2]
    rc, buf = _raw_call(case)
    assert rc == 0, _lib.load_library().jn_last_error()
    n = int(want["offsets"][B])
    assert torch.equal(buf["offsets"].cpu(), want["offsets"]), name
    for k in NAMES[:8]:
        got = buf[k].cpu()
        if k == "local_bboxes" and nb == 0:
            assert bool((got == FILL).all()), (name, k)               # no column to write
            continue
        assert got.dtype == want[k].dtype and got.shape == want[k].shape and torch.equal(got, want[k]), (name, k)
    assert torch.equal(buf["cells_yolox"][:n].cpu(), want["cells_yolox"]), name
    assert bool((buf["cells_yolox"][n:] == FILL).all()) and bool((buf["bboxes_yolox"][n:] == FILL).all()), name   # rows >= n: untouched
    if nb:
        assert torch.equal(buf["bboxes_yolox"][:n].cpu(), want["bboxes_yolox"]), name
    # the wrapper: the same tensors, the detector rows cut to n
    got = tj.teacher_walks_device(case["bboxes"].to(DEV), **{k: v for k, v in case.items() if k != "bboxes"})
    assert set(got) == set(want)
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k].cpu(), want[k]), (name, k)
        assert got[k].is_cuda == (k != "offsets"), k


def test_equal_seeds_give_equal_bytes_and_other_seeds_other_walks(host_walks):
    case = tw.CASES["ties_8x8"]
    _, a = _raw_call(case)
    _, b = _raw_call(case)
    for k in NAMES:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    _, c = _raw_call(case, seed=case["seed"] + 1)
    assert not torch.equal(a["positions"], c["positions"])
    assert torch.equal(c["targets"], a["targets"])
    want = tj.teacher_walks(**{**case, "seed": case["seed"] + 1})
    assert torch.equal(c["positions"].cpu(), want["positions"]) and torch.equal(c["next_actions"].cpu(), want["next_actions"])


def test_capacity_cuts_the_detector_rows(host_walks):
    case, want = tw.CASES["three_images"], host_walks["three_images"]
    B = case["bboxes"].shape[0]
    n, first_of_last = int(want["offsets"][B]), int(want["offsets"][B - 1])
    assert 0 < first_of_last < n - 1
    for cap in (0, 1, first_of_last, first_of_last + 1, n - 1, n):
        rc, buf = _raw_call(case, capacity=cap)
        assert rc == 0 and torch.equal(buf["offsets"].cpu(), want["offsets"]), cap
        assert torch.equal(buf["cells_yolox"][:cap].cpu(), want["cells_yolox"][:cap]), cap
        assert torch.equal(buf["bboxes_yolox"][:cap].cpu(), want["bboxes_yolox"][:cap]), cap
        assert bool((buf["cells_yolox"][cap:] == FILL).all()) and bool((buf["bboxes_yolox"][cap:] == FILL).all()), cap
        assert torch.equal(buf["positions"].cpu(), want["positions"]), cap


def test_bad_arguments_are_refused():
    """Host-side checks: a refused call launches nothing (every buffer keeps its sentinel)."""
    lib = _lib.load_library()
    case = tw.CASES["three_images"]
    assert _raw_call(case)[0] == 0
    bad = {"a grid of 4097 cells": dict(gh=1, gw=tj.MAX_WALK_CELLS + 1), "a grid of 65 x 64 cells": dict(gh=65, gw=64),
           "Gh = 0": dict(gh=0), "Gw = 0": dict(gw=0), "P = 0": dict(P=0),
           "T = 0": dict(T=0), "T = -1": dict(T=-1), "T beyond the ring": dict(T=tj.MAX_WALK_STEPS + 1),
           "min_keypoints = -1": dict(min_keypoints=-1), "max below min": dict(min_keypoints=2, max_keypoints=1),
           "max_keypoints beyond the table": dict(max_keypoints=tj.MAX_WALK_KEYPOINTS + 1),
           "B * Gh * Gw beyond int32": dict(B=2 ** 31 // (6 * 7) + 1), "B = -1": dict(B=-1), "nb = -1": dict(nb=-1),
           "capacity = -1": dict(capacity=-1),
           "null boxes with nb > 0": dict(null=("bboxes",)), "null local boxes with nb > 0": dict(null=("local_bboxes",)),
           "null detector boxes": dict(null=("bboxes_yolox",)), "null cells": dict(null=("cells_yolox",)),
           "null offsets": dict(null=("offsets",)), "null positions": dict(null=("positions",)), "null masks": dict(null=("masks",)),
           "null n_steps": dict(null=("n_steps",)), "null targets": dict(null=("targets",))}
    for tag, kw in bad.items():
        rc, buf = _raw_call(case, **kw)
        assert rc == -1, tag                                                            # JN_EINVAL
        assert b"jn_teacher_walks" in lib.jn_last_error(), tag
        assert all(bool((t == FILL).all()) for t in buf.values() if t is not None), tag
    # the limits themselves are taken
    assert _raw_call(case, max_keypoints=tj.MAX_WALK_KEYPOINTS, min_keypoints=tj.MAX_WALK_KEYPOINTS)[0] == 0
    with pytest.raises(_lib.JnError):
        tj.teacher_walks_device(case["bboxes"].to(DEV), 65, 64, 4, 6, 0, 0, False, 1)
    with pytest.raises(AssertionError):                                                 # the wrapper's host-side check
        tj.teacher_walks_device(case["bboxes"].to(DEV), 6, 7, 4, 6, 0, 0, False, 1, start_positions=[[0, 0], [6, 0], [0, 0]])
    # B = 0: empty outputs, offsets = [0]
    out = tj.teacher_walks_device(torch.zeros((0, 2, 4), dtype=torch.int64, device=DEV), 6, 7, 4, 6, 0, 1, False, 1)
    assert out["offsets"].tolist() == [0] and out["positions"].shape == (0, 6, 2) and out["cells_yolox"].shape == (0, 3)


def test_a_ring_of_the_largest_T():
    """T = 4096, the most the LDS ring holds, on a walk far shorter than that: one live row block, a long zero tail."""
    case = {**tw.CASES["zero_tail"], "T": tj.MAX_WALK_STEPS}
    want = tj.teacher_walks(**case)
    got = tj.teacher_walks_device(case["bboxes"].to(DEV), **{k: v for k, v in case.items() if k != "bboxes"})
    for k in NAMES:
        assert torch.equal(got[k].cpu(), want[k]), k


# ---- the trainer's device route --------------------------------------------------------------------------------------------
BOXES = torch.tensor([[[1, 1, 7, 3], [18, 14, 27, 23], [0, 0, 0, 0]],
                      [[0, 0, 0, 0], [9, 5, 14, 11], [0, 0, 0, 0]],
                      [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.int64)
INT_KEYS = ("positions", "current_actions", "next_actions", "labels", "masks", "local_bboxes", "bboxes_yolox")


def _walk_trainer(**kw):
    """A trainer for ``generate_trajectories`` alone: that method needs the model's device, nothing else of it."""
    cfg = ja.CfgNode(patch_size=4, max_seq_len=6, min_keypoints=0, max_keypoints=2, binomial_keypoints=False, seed=3, **kw)
    return ja.SupervisedTrainer(cfg, SimpleNamespace(device=torch.device(DEV)))


@pytest.mark.parametrize("kind", ["f32", "uint8"])
@pytest.mark.parametrize("rotations", [False, True], ids=["plain", "rotations"])
def test_generate_trajectories_on_the_device(kind, rotations):
    from jolineedle_amd.views import stack_bboxes
    g = torch.Generator().manual_seed(7)
    B, P, T, s = 3, 4, 6, 12345
    if kind == "uint8":
        images = torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8)
    else:
        images = torch.rand((B, 3, 32, 32), generator=g)
    tr = _walk_trainer(uint8_images=kind == "uint8", rotations=rotations)
    batch = {"image": images.to(DEV), "bboxes": BOXES, "class_id": torch.tensor([2, 0, 1])}
    t = tr.generate_trajectories(batch, seed=s, device=True)
    host_keys = set(_walk_trainer(uint8_images=kind == "uint8").generate_trajectories(batch, seed=s))
    assert set(t) == host_keys
    views = tr.last_views
    assert (views is not None) == rotations
    boxes = views.transform_bboxes(stack_bboxes(BOXES, B)) if rotations else BOXES
    if rotations:
        assert views.canvas == (32, 32) and not torch.equal(boxes, BOXES)
    want = tj.teacher_walks(boxes, 8, 8, P, T, 0, 2, False, s)
    for k in INT_KEYS:
        assert t[k].is_cuda and t[k].dtype == want[k].dtype and torch.equal(t[k].cpu(), want[k]), k
    assert torch.equal(t["class_id"].cpu(), torch.tensor([2, 0, 1]))
    src = images.to(DEV)
    ii = torch.where(want["masks"] > 0, torch.arange(B)[:, None].expand(B, T), torch.full((B, T), -1)).reshape(-1)
    patches = tj.gather_indexed(src, ii, want["positions"].reshape(-1, 2), P, views=views)
    assert t["patches"].shape == (B, T, 3, P, P) and torch.equal(t["patches"], patches.view(B, T, 3, P, P))
    cells = want["cells_yolox"]
    assert torch.equal(t["patches_yolox"], tj.gather_indexed(src, cells[:, 0], cells[:, 1:], P, views=views))
    assert len(cells) > 0 and float(want["masks"].sum()) < B * T             # zero patches behind a short walk are compared too
    # position=(y, x): every image starts there; seed=None: the trainer's own counter
    t2 = tr.generate_trajectories(batch, seed=s, device=True, position=(7, 0), use_views=False)
    want2 = tj.teacher_walks(BOXES, 8, 8, P, T, 0, 2, False, s, start_positions=torch.tensor([[7, 0]] * B))
    assert all(torch.equal(t2[k].cpu(), want2[k]) for k in INT_KEYS)
    calls = tr._device_walks
    t3 = tr.generate_trajectories(batch, device=True, use_views=False)
    want3 = tj.teacher_walks(BOXES, 8, 8, P, T, 0, 2, False, 3 * 1000003 + calls + 1)
    assert tr._device_walks == calls + 1 and all(torch.equal(t3[k].cpu(), want3[k]) for k in INT_KEYS)
    # the config picks the route when `device` is not given; the default is the host route
    assert tr.generate_trajectories(batch, seed=s, use_views=False)["bboxes_yolox"].shape[1] == 2      # host: the real rows only
    tr.config.device_trajectories = True
    t4 = tr.generate_trajectories(batch, seed=s, use_views=False)
    want4 = tj.teacher_walks(BOXES, 8, 8, P, T, 0, 2, False, s)
    assert all(torch.equal(t4[k].cpu(), want4[k]) for k in INT_KEYS)


def test_train_iteration_with_device_trajectories():
    """One ``train_iteration`` by each route from the same weights, at the sizes above with the smallest patch the engine
    takes (32 px: images of 256 x 256 on the same 8 x 8 grid).  This shows that the route is wired, it does not compare
    two random streams."""
    from tests.helpers import make_pair
    P, T, B = 32, 6, 3
    g = torch.Generator().manual_seed(11)
    images = torch.rand((B, 3, 8 * P, 8 * P), generator=g)
    batch = {"image": images.to(DEV), "bboxes": BOXES * 8, "class_id": torch.zeros(B, dtype=torch.long)}
    for route in (True, False):
        product, _ = make_pair(9, patch_size=P, block_size=T, image_processor="yolox-nano", gpt_backbone="yolox-nano",
                               max_batch=B * T)
        cfg = ja.CfgNode(patch_size=P, max_seq_len=T, min_keypoints=0, max_keypoints=2, binomial_keypoints=False,
                         stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, yolo_lr=1e-3, gradient_accumulation=1,
                         detection_enabled=True, seed=3, device_trajectories=route)
        tr = ja.SupervisedTrainer(cfg, product)
        m = tr.train_iteration(batch, seed=77)
        assert torch.isfinite(torch.as_tensor(float(m["loss"]))) and torch.isfinite(torch.as_tensor(float(m["yolo_total_loss"]))), route
        traj = m["trajectories"]
        assert tr._device_walks == int(route)
        if route:
            want = tj.teacher_walks(BOXES * 8, 8, 8, P, T, 0, 2, False, 77)
            assert torch.equal(traj["masks"].sum(1).cpu(), want["n_steps"].clamp(max=T).float())
            assert torch.equal(traj["positions"].cpu(), want["positions"])
        del product, tr
        torch.cuda.empty_cache()
