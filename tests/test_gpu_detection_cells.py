"""``jn_detection_cells`` (csrc/kernels_env.hip) against its host statement ``detection.detection_cells``, bit for bit; the
device route of ``NeedleGeneralEnv.get_detection_batch`` against the host method on fp32, uint8 and view envs; and one
training iteration with ``config.device_detection_batch``.  Inputs: tests/detection_cells_cases.py."""
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, detection
from jolineedle_amd._lib import ptr
from jolineedle_amd.views import ImageViews
from tests import detection_cells_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = dc.P
SEED = 0xFEDC_BA98_7654_3210          # above 2**63: the seed is an unsigned 64-bit key


def _same(got, want, tag):
    cells, targets, offsets, n_pos = got
    assert cells.dtype == targets.dtype == torch.int64 and offsets.dtype == n_pos.dtype == torch.int32, tag
    for name, a, b in zip(("cells", "targets", "offsets", "n_pos"), got, want):
        assert a.shape == b.shape and torch.equal(a.cpu(), b), (tag, name)


@pytest.mark.parametrize("grid", dc.GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_device_equals_host_bit_for_bit(grid):
    n_rows = 0
    for gh, gw, B, nb, bb, ext in dc.all_cases():
        if (gh, gw) != grid:
            continue
        for sn in dc.sample_negs(gh, gw):
            want = detection.detection_cells(bb, gh, gw, P, sn, SEED, extents=ext)
            got = detection.detection_cells_device(bb.to(DEV), gh, gw, P, sn, SEED, extents=ext)
            _same(got, want, (gh, gw, B, nb, sn, ext is not None))
            n_rows += int(want[2][B])
    print(f"grid {grid}: {n_rows} rows compared")
    assert n_rows > 0


def _raw_call(bb, ext, B, nb, gh, gw, p, sn, seed, cap, fill=-7):
    """One ``jn_detection_cells`` into buffers of B * gh * gw rows filled with `fill`; returns (rc, cells, targets, offsets, n_pos)."""
    rows = max(1, B * max(gh, 1) * max(gw, 1))
    cells = torch.full((rows, 3), fill, device=DEV, dtype=torch.int64)
    targets = torch.full((rows, max(nb, 1), 5), fill, device=DEV, dtype=torch.int64)
    offsets = torch.full((B + 1,), fill, device=DEV, dtype=torch.int32)
    n_pos = torch.full((max(B, 1),), fill, device=DEV, dtype=torch.int32)
    rc = _lib.load_library().jn_detection_cells(ptr(bb), ptr(ext), B, nb, gh, gw, p, sn, seed, cap, ptr(cells), ptr(targets),
                                                ptr(offsets), ptr(n_pos), _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, cells, targets, offsets, n_pos


def test_capacity_cuts_the_rows_and_still_reports_n():
    gh, gw, B, nb = 3, 5, 3, 3
    bb = dc.make_boxes(gh, gw, B, nb, shift=1)
    want = detection.detection_cells(bb, gh, gw, P, 2, SEED)
    n = int(want[2][B])
    first_of_last = int(want[2][B - 1])
    assert 0 < first_of_last < n - 1
    for cap in (0, 1, first_of_last, first_of_last + 1, n - 1, n, n + 3):       # cuts between and inside images, none
        rc, cells, targets, offsets, n_pos = _raw_call(bb.to(DEV), None, B, nb, gh, gw, P, 2, SEED, cap)
        assert rc == 0, cap
        assert torch.equal(offsets.cpu(), want[2]) and torch.equal(n_pos.cpu(), want[3]), cap
        k = min(cap, n)
        assert torch.equal(cells[:k].cpu(), want[0][:k]) and torch.equal(targets[:k].cpu(), want[1][:k]), cap
        assert bool((cells[k:] == -7).all()) and bool((targets[k:] == -7).all()), cap   # rows >= capacity and >= n: untouched


def test_bad_arguments_are_refused():
    lib = _lib.load_library()
    gh, gw, B, nb = 2, 2, 3, 1
    bb = dc.make_boxes(gh, gw, B, nb).to(DEV)
    good_ext = torch.tensor([[1, 2], [2, 2], [2, 1]], dtype=torch.int32, device=DEV)
    assert _raw_call(bb, None, B, nb, gh, gw, P, 1, 5, B * gh * gw)[0] == 0
    assert _raw_call(bb, good_ext, B, nb, gh, gw, P, 1, 5, B * gh * gw)[0] == 0
    bad = {"nb = 0": dict(nb=0), "P = 0": dict(p=0), "sample_neg = -1": dict(sn=-1), "Gh = 0": dict(gh=0), "Gw = 0": dict(gw=0),
           "a grid of 4097 cells": dict(gh=1, gw=detection.MAX_DETECTION_CELLS + 1), "a grid of 65 x 64 cells": dict(gh=65, gw=64)}
    for tag, kw in bad.items():
        a = dict(nb=nb, gh=gh, gw=gw, p=P, sn=1)
        a.update(kw)
        # (a refused call launches nothing: the buffers, sized for the 2 x 2 grid, are never addressed)
        cells = torch.zeros((B * 4, 3), device=DEV, dtype=torch.int64)
        targets = torch.zeros((B * 4, 1, 5), device=DEV, dtype=torch.int64)
        offsets = torch.zeros((B + 1,), device=DEV, dtype=torch.int32)
        n_pos = torch.zeros((B,), device=DEV, dtype=torch.int32)
        rc = lib.jn_detection_cells(ptr(bb), None, B, a["nb"], a["gh"], a["gw"], a["p"], a["sn"], 5, B * 4, ptr(cells), ptr(targets),
                                    ptr(offsets), ptr(n_pos), _lib.current_stream(torch.device(DEV)))
        assert rc == -1, tag                                                            # JN_EINVAL
        assert b"jn_detection_cells" in lib.jn_last_error(), tag
    for tag, rows in {"an extent of 0": [[1, 2], [0, 2], [2, 1]], "an extent beyond Gh": [[1, 2], [3, 2], [2, 1]],
                      "an extent beyond Gw": [[1, 2], [2, 2], [2, 3]]}.items():
        ext = torch.tensor(rows, dtype=torch.int32, device=DEV)
        assert _raw_call(bb, ext, B, nb, gh, gw, P, 1, 5, B * gh * gw)[0] == -1, tag
    with pytest.raises(_lib.JnError):
        detection.detection_cells_device(bb, 65, 64, P, 1, 5)


# ---- get_detection_batch(device=True) against the host method -------------------------------------------------------------
H, W, B_ENV, T_ENV = 24, 40, 3, 4          # a 3 x 5 grid of 8 px cells


def _env_boxes():
    # image 0: across a corner + inside one cell + padding; image 1: three cells + a box beyond the right edge; image 2: padding only
    return torch.tensor([[[6, 5, 10, 9], [33, 17, 38, 22], [0, 0, 0, 0]],
                         [[2, 10, 22, 13], [36, 2, 44, 6], [0, 0, 0, 0]],
                         [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.int64)


def _make_env(kind):
    """(env, canvas [B, 3, H, W] fp32 on the host: what every patch is a slice of)."""
    g = torch.Generator().manual_seed(41)
    u8 = torch.randint(0, 256, (B_ENV, 3, H, W), generator=g, dtype=torch.uint8)
    if kind == "f32":
        img = torch.rand((B_ENV, 3, H, W), generator=g)
        return ja.NeedleGeneralEnv(img.to(DEV), _env_boxes(), P, T_ENV, 1, True), img
    if kind == "uint8":
        return ja.NeedleGeneralEnv(u8.to(DEV), _env_boxes(), P, T_ENV, 1, True, uint8_images=True), u8.float().div(255)
    srcs = [torch.rand((3, H, W), generator=g), torch.rand((3, W, H), generator=g), torch.rand((3, H, W), generator=g)]
    views = ImageViews([s.to(DEV) for s in srcs], rot=[0, 90, 0], ty=[0, 0, 3], tx=[0, 0, -5], patch_size=P)
    assert views.canvas == (H, W)
    stored = _env_boxes()
    stored[1] = torch.tensor([[3, 4, 9, 30], [12, 1, 20, 6], [0, 0, 0, 0]])             # in the stored 40 x 24 image
    stored[2, 0] = torch.tensor([10, 8, 20, 12])                                         # moves with the translation
    env = ja.NeedleGeneralEnv(None, views.transform_bboxes(stored), P, T_ENV, 1, True, views=views)
    return env, views.materialize().cpu()


@pytest.mark.parametrize("kind", ["f32", "uint8", "views"])
def test_get_detection_batch_device_against_the_host_method(kind):
    env, canvas = _make_env(kind)
    host_p, host_b = env.get_detection_batch(sample_neg=0)
    dev_p, dev_b = env.get_detection_batch(sample_neg=0, device=True, seed=3)
    assert dev_p.dtype == host_p.dtype == torch.float32 and dev_b.dtype == host_b.dtype == torch.int64
    assert dev_p.is_cuda and dev_b.is_cuda and len(host_p) >= 4
    assert torch.equal(dev_p, host_p) and torch.equal(dev_b, host_b)
    # with negatives: every patch is the canvas slice of the cell the host restatement names
    bb = env._bboxes_dev.cpu()
    cells, targets, offsets, n_pos = detection.detection_cells(bb, H // P, W // P, P, 2, 11)
    dev_p, dev_b = env.get_detection_batch(sample_neg=2, device=True, seed=11)
    assert dev_p.shape == (len(cells), 3, P, P) and int(offsets[B_ENV]) == int(n_pos.sum()) + 2 * B_ENV
    assert torch.equal(dev_b.cpu(), targets)
    for row, (i, y, x) in enumerate(cells.tolist()):
        assert torch.equal(dev_p[row].cpu(), canvas[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P]), (kind, row)
    again_p, again_b = env.get_detection_batch(sample_neg=2, device=True, seed=11)
    assert torch.equal(again_p, dev_p) and torch.equal(again_b, dev_b)


def test_get_detection_batch_device_in_ragged_mode_keeps_to_the_extents():
    """clamp_to_image: the env hands its grid extents to the kernel, so every row lies inside its image's own grid."""
    g = torch.Generator().manual_seed(43)
    srcs = [torch.rand((3, h, w), generator=g).to(DEV) for h, w in ((H, W), (16, 20), (8, 8))]
    views = ImageViews(srcs, patch_size=P)
    assert views.canvas == (H, W)
    boxes = torch.tensor([[[6, 5, 10, 9], [0, 0, 0, 0]], [[2, 3, 30, 6], [10, 12, 13, 20]], [[0, 0, 0, 0], [0, 0, 0, 0]]])
    env = ja.NeedleGeneralEnv(None, boxes, P, T_ENV, 1, True, views=views, clamp_to_image=True)
    assert env.grid_extents.tolist() == [[3, 5], [2, 3], [1, 1]]
    canvas = views.materialize().cpu()
    for sn in (0, 2):
        cells, targets, offsets, n_pos = detection.detection_cells(boxes, H // P, W // P, P, sn, 17, extents=env.grid_extents)
        dev_p, dev_b = env.get_detection_batch(sample_neg=sn, device=True, seed=17)
        assert torch.equal(dev_b.cpu(), targets) and dev_p.shape[0] == len(cells)
        for row, (i, y, x) in enumerate(cells.tolist()):
            assert y < env.grid_extents[i, 0] and x < env.grid_extents[i, 1]
            assert torch.equal(dev_p[row].cpu(), canvas[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P]), row
    assert (offsets[1:] - offsets[:-1]).tolist() == [4 + 2, 4 + 2, 1 + 0]      # image 1: pieces beyond its 2 x 3 grid dropped; image 2: one cell, positive


def test_get_detection_batch_device_on_a_batch_without_boxes():
    """nb = 0: negatives only with targets [n, 0, 5], as the host route gives them."""
    g = torch.Generator().manual_seed(47)
    img = torch.rand((B_ENV, 3, H, W), generator=g)
    env = ja.NeedleGeneralEnv(img.to(DEV), torch.zeros((B_ENV, 0, 4), dtype=torch.int64), P, T_ENV, 1, True)
    host_p, host_b = env.get_detection_batch(sample_neg=2)
    dev_p, dev_b = env.get_detection_batch(sample_neg=2, device=True, seed=9)
    assert dev_b.shape == host_b.shape == (2 * B_ENV, 0, 5) and dev_b.dtype == host_b.dtype == torch.int64
    assert dev_p.shape == host_p.shape == (2 * B_ENV, 3, P, P)
    inert = torch.tensor([0, 0, -1, -1]).repeat(B_ENV, 1, 1)
    cells, _, offsets, n_pos = detection.detection_cells(inert, H // P, W // P, P, 2, 9)
    assert n_pos.tolist() == [0] * B_ENV and offsets.tolist() == [0, 2, 4, 6]
    for row, (i, y, x) in enumerate(cells.tolist()):
        assert torch.equal(dev_p[row].cpu(), img[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P]), row
    assert env.get_detection_batch(sample_neg=0, device=True)[0].shape == (0, 3, P, P)


KEYS = ("loss", "yolo_total_loss", "yolo_iou_loss", "yolo_conf_loss", "yolo_cls_loss", "yolo_l1_loss", "yolo_num_fg")


@pytest.fixture
def detection_batch_calls(monkeypatch):
    """Records every ``NeedleGeneralEnv.get_detection_batch`` call: (sample_neg, device, seed, patches, boxes)."""
    calls = []
    inner = ja.NeedleGeneralEnv.get_detection_batch

    def recording(self, sample_neg=1, generator=None, device=False, seed=0):
        out = inner(self, sample_neg, generator, device=device, seed=seed)
        calls.append((int(sample_neg), bool(device), int(seed), out[0].clone(), out[1].clone()))
        return out
    monkeypatch.setattr(ja.NeedleGeneralEnv, "get_detection_batch", recording)
    return calls


def _detector_trainer(route, sample_neg, Pt, Tn, **kw):
    from tests.test_gpu_parity import _cfg, _detector_pair
    product, _ = _detector_pair(Pt, 0.5, image_processor="yolox-nano", max_batch=8)
    cfg = _cfg(T=Tn, learning_rate=1e-3, gradient_accumulation=1, **kw)
    cfg.detection_enabled, cfg.yolo_lr, cfg.detection_sample_neg, cfg.device_detection_batch = True, 2e-3, sample_neg, route
    return product, ja.ReinforceTrainer(cfg, product)


def _seed_of(tr):
    assert tr.rank == 0
    return (tr.seed * 1000003 + tr.iter_num) & (2 ** 64 - 1)


def test_train_iteration_with_the_device_detection_batch(detection_batch_calls):
    """``train_iteration`` with a detector at the sizes of test_reinforce_iteration_with_detector_training (test_gpu_parity.py),
    ``detection_sample_neg = 0``, from the same weights: the host route twice and ``device_detection_batch`` once.
    The trainer takes the route the flag names (one ``get_detection_batch`` call, with ``device=True`` and the seed of
    the trainer's seed and iteration counter, or with neither), and hands the detector the same bytes on both.  Every
    reported metric of the device run is then no further from the host run than the second host run is: the bound is the
    run-to-run difference of the host route itself, measured here (the atomics of the BatchNorm statistics; it was 0.0
    for every metric when this was written, which makes the check an equality).  On the weights the checks are the
    windows of the named test, for every run."""
    from tests.helpers import synth_batch
    Pt, Tn, B = 64, 3, 2
    images, bboxes, start = synth_batch(B, 3, 3, Pt, seed=8)
    runs, batches = {}, {}
    for tag, route in (("host", False), ("host again", False), ("device", True)):
        product, tr = _detector_trainer(route, 0, Pt, Tn)
        env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, Pt, Tn, 1, True)
        before = {k: v.clone() for k, v in product.state_dict().items()}
        del detection_batch_calls[:]
        m = tr.train_iteration(env, start_positions=start)
        assert len(detection_batch_calls) == 1, tag
        sn, device, seed, patches, boxes = detection_batch_calls[0]
        assert sn == 0 and device == route and seed == (_seed_of(tr) if route else 0), (tag, sn, device, seed)
        assert tr.iter_num == 1 and seed == (1 * 1000003 + 1 if route else 0)               # _cfg: seed = 1
        batches[tag] = (patches, boxes)
        for k in KEYS:
            assert k in m and torch.isfinite(torch.as_tensor(float(m[k]))), (tag, k)
        product.pull_parameters()
        after = product.state_dict()
        kd, kg = "yolox.head.obj_preds.0.weight", "transformer.wte.weight"
        d_det = (after[kd].cpu() - before[kd].cpu()).abs().max().item()
        d_gpt = (after[kg].cpu() - before[kg].cpu()).abs().max().item()
        assert 1e-3 < d_det < 2.5e-3 and 5e-4 < d_gpt < 1.2e-3, (tag, d_det, d_gpt)
        runs[tag] = {k: float(m[k]) for k in KEYS}
        del product, tr, env
    assert len(batches["host"][0]) > 0 and runs["device"]["yolo_num_fg"] > 0
    for tag in ("host again", "device"):
        assert torch.equal(batches[tag][0], batches["host"][0]) and torch.equal(batches[tag][1], batches["host"][1]), tag
    for k in KEYS:
        noise, diff = abs(runs["host"][k] - runs["host again"][k]), abs(runs["host"][k] - runs["device"][k])
        print(f"{k}: host {runs['host'][k]!r} device {runs['device'][k]!r} |host - device| {diff:.3e} |host - host again| {noise:.3e}")
        assert diff <= noise, (k, runs["host"][k], runs["device"][k], noise)


def test_training_step_and_eval_on_batch_take_the_device_route(detection_batch_calls):
    """The other two call sites: ``training_step`` (``detection_sample_neg = 1``: negatives are drawn, from the seed of
    that iteration) and the ``sample_neg = 0`` call of ``eval_on_batch``; without the flag neither passes ``device``."""
    from tests.helpers import synth_batch
    Pt, Tn, B = 64, 3, 2
    images, bboxes, start = synth_batch(B, 3, 3, Pt, seed=8)
    batch = {"image": images.to(DEV), "bboxes": bboxes}
    for route in (False, True):
        product, tr = _detector_trainer(route, 1, Pt, Tn)
        og, oy = product.configure_optimizers(tr.config)
        for it in (1, 2):
            del detection_batch_calls[:]
            m = tr.training_step(batch, og, oy, start_positions=start)
            assert tr.iter_num == it and len(detection_batch_calls) == 1
            sn, device, seed, patches, boxes = detection_batch_calls[0]
            assert sn == 1 and device == route and seed == (_seed_of(tr) if route else 0), (route, it, seed)
            assert all(torch.isfinite(torch.as_tensor(float(m[k]))) for k in KEYS), (route, it)
            if route:                                            # the batch is the one the host statement names for that seed
                cells, targets, _, _ = detection.detection_cells(bboxes, 3, 3, Pt, 1, seed)
                assert torch.equal(boxes.cpu(), targets) and len(patches) == len(cells)
                for row, (i, y, x) in enumerate(cells.tolist()):
                    assert torch.equal(patches[row].cpu(), images[i, :, y * Pt:(y + 1) * Pt, x * Pt:(x + 1) * Pt]), row
        del product, tr
        product, tr = _detector_trainer(route, 1, Pt, Tn)       # a fresh model, as eval_on_batch's own test evaluates one
        del detection_batch_calls[:]
        env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, Pt, Tn, 1, True)
        m = tr.eval_on_batch(env, do_detection=True)
        assert "yolo_map" in m and len(detection_batch_calls) == 1
        sn, device, seed, patches, boxes = detection_batch_calls[0]
        assert sn == 0 and device == route
        host_p, host_b = ja.NeedleGeneralEnv.get_detection_batch(env, 0)
        assert torch.equal(patches, host_p) and torch.equal(boxes, host_b)
        del product, tr, env
