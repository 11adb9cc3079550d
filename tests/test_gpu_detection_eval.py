"""Detection evaluation on the device (csrc/kernels_eval.hip): ``jn_merge_boxes`` against the reference's own outputs
(tests/golden/g10_merge_boxes.npz, ``torch.equal``), ``jn_match_detections`` / ``jn_average_precision`` against the host
``map_50`` on the same inputs, and ``eval_on_images`` / ``infer_images`` with ``device_metrics=True`` against ``False``.

Bar of the mAP comparison, 1e-12: both sides perform the same IEEE fp64 operations on the same thresholds; the only
freedom is the order of a sum of 101 terms in [0, 1], and 101 * 101 * 2**-53 ~ 1.1e-12.  Hits and selected rows are
integers and compare exactly.  `map` of the integration tests is stored as fp32: 1e-6."""
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, detection
from jolineedle_amd._lib import ptr
from jolineedle_amd.config import model_config
from tests import ragged_ref
from tests.test_detection_eval_cpu import g10, g10_cases, parallel_merge  # noqa: F401  (g10 is a fixture)
from tests.test_gpu_ragged_batch import SEED_64, SIZES_64, _cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAP_BAR = 1e-12


# ---- merge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pred", "tgt"])
def test_merge_boxes_device_equals_the_reference_in_one_ragged_launch(g10, form):
    """Every G10 case side by side in one launch (counts 0, 1, 4, 6, 40, 64, 255, 256, 257, 600; Nmax = 600)."""
    cases = [(name, boxes, want) for name, f, boxes, want in g10_cases(g10) if f == form]
    batch = [None] + [boxes for _, boxes, _ in cases]                       # image 0 has no box at all
    packed, counts = detection.pack_boxes(batch, 7 if form == "pred" else 5, DEV)
    assert packed.shape[1] == 600 and {0, 1, 6, 64, 255, 256, 257, 600} <= set(counts.tolist())
    packed[0] = float("nan")                                                # rows past an image's count are never read
    for i, (_, boxes, _) in enumerate(cases):
        packed[i + 1, len(boxes):] = float("nan")
    out, out_counts, rounds = detection.merge_boxes_device(packed, counts, 2, target=form == "tgt", return_rounds=True)
    out, out_counts, rounds = out.cpu(), out_counts.tolist(), rounds.tolist()
    assert out_counts[0] == 0
    print("relaxation rounds:", dict(zip(["empty"] + [c[0] for c in cases], rounds)))
    for i, (name, _, want) in enumerate(cases):
        assert out_counts[i + 1] == len(want), (name, out_counts[i + 1], len(want))
        assert torch.equal(out[i + 1, :len(want)], want.float()), name
    assert max(rounds) <= 64 and min(rounds) >= 1


def test_merge_boxes_device_at_the_largest_count():
    """4096 boxes per image: 96 KB of LDS, every thread owning 16 boxes.  Sparse boxes with links, against the parallel
    rule in plain torch (pinned to the reference by the CPU suite)."""
    g = torch.Generator().manual_seed(5)
    n = 4096
    xs, ys = torch.randperm(n, generator=g) * 40, torch.randperm(n, generator=g) * 40
    wh = torch.randint(5, 20, (n, 2), generator=g)
    b = torch.stack((xs, ys, xs + wh[:, 0], ys + wh[:, 1]), 1)
    for _ in range(600):                                                     # links: a box moved to the right of another
        i, j = (int(v) for v in torch.randint(0, n, (2,), generator=g))
        if i != j:
            b[j] = torch.stack((b[i, 2] + 1, b[i, 1] + 1, b[i, 2] + 10, b[i, 3] + 3))
    pred = torch.cat((b.float(), torch.rand((n, 2), generator=g), torch.zeros((n, 1))), 1)
    want, _ = parallel_merge(pred, 2, False)
    assert len(want) < n - 300
    out, cnt, rounds = detection.merge_boxes_device(pred.unsqueeze(0).to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV), 2,
                                                    return_rounds=True)
    print("groups", int(cnt), "rounds", int(rounds))
    assert int(cnt) == len(want) and torch.equal(out[0, :len(want)].cpu(), want)


def test_merge_boxes_abi_refuses_more_than_4096_boxes_without_a_launch():
    lib = _lib.load_library()
    boxes = torch.zeros((1, 8, 7), device=DEV)
    counts = torch.zeros((1,), dtype=torch.int32, device=DEV)
    out = torch.full((1, 8, 6), -7.0, device=DEV)
    out_counts = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rc = lib.jn_merge_boxes(ptr(boxes), ptr(counts), 1, 4097, 7, 0, 2.0, ptr(out), ptr(out_counts), None, _lib.current_stream(DEV))
    assert rc == -1                                                          # JN_EINVAL
    msg = lib.jn_last_error().decode()
    assert "jn_merge_boxes" in msg and "4097" in msg and "4096" in msg
    torch.cuda.synchronize()
    assert int(out_counts) == -7 and bool((out == -7).all())                 # nothing ran


def test_merge_boxes_batched_device_keeps_the_list_contract(g10):
    names = ["random0000" if "random0000" in g10["names"] else g10["names"][0], "duplicates", "negative"]
    tg = [torch.from_numpy(g10[f"{n}.tgt"]).to(DEV) for n in names]
    got = detection.merge_boxes_batched_device([tg[0], None, tg[1], tg[2]], target=True)
    assert got[1] is None
    for g, n in zip([got[0], got[2], got[3]], names):
        assert g.dtype == torch.long and torch.equal(g.cpu(), torch.from_numpy(g10[f"{n}.tgt_out"]))
    pr = [torch.from_numpy(g10[f"{n}.pred"]).to(DEV) for n in names]
    got = detection.merge_boxes_batched_device([None, pr[0], pr[1], pr[2]])
    assert got[0] is None
    for g, n in zip(got[1:], names):
        assert g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(g10[f"{n}.pred_out"]))
    assert detection.merge_boxes_batched_device([None, None]) == [None, None]


# ---- match / average precision ------------------------------------------------------------------------------------------
def host_match(out, tgt, max_det=100):
    """The per-image half of ``detection.map_50``, returning (selected rows, hits)."""
    if out is None or len(out) == 0:
        return [], []
    out = out.detach().to("cpu", torch.float64)
    order = torch.argsort(out[:, 4], descending=True, stable=True)[:max_det]
    gt = tgt[:, 1:5].detach().to("cpu", torch.float64)
    iou = detection._iou_matrix(out[order, :4], gt) if len(gt) else torch.zeros((len(order), 0), dtype=torch.float64)
    taken, hits = [False] * len(gt), []
    for p in range(len(order)):
        best, best_j = 0.5, -1
        for j in range(len(gt)):
            if not taken[j] and iou[p, j] >= best:
                best, best_j = float(iou[p, j]), j
        if best_j >= 0:
            taken[best_j] = True
        hits.append(int(best_j >= 0))
    return order.tolist(), hits


def _p(rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)


def _t(rows):
    return torch.tensor([[0] + list(r) for r in rows], dtype=torch.float32).reshape(-1, 5)


def _map_cases(golden):
    g7 = torch.from_numpy(golden("g7_known_answers.npz")["targets_expected"])
    p2 = _p([[410, 410, 447, 446, 0.5, 1], [448, 410, 500, 447, 0.9, 1], [410, 448, 447, 500, 0.8, 1],
             [448, 448, 500, 500, 0.7, 1], [1500, 1500, 1600, 1600, 0.6, 1]])
    cases = {"g7_known_answers": ([None, p2, p2[[0, 2, 3, 4]]], [g7, g7, g7])}
    # IoU exactly 0.5 (50 / 100) is a hit; a box 0.001 px taller has IoU just below
    cases["iou_at_and_below_half"] = ([_p([[0, 0, 10, 10, 0.9, 1]]), _p([[0, 0, 10, 10.001, 0.9, 1]])],
                                      [_t([[0, 0, 10, 5]]), _t([[0, 0, 10, 5]])])
    # two targets at IoU 0.6 each: the higher index is taken, so the second prediction (which overlaps only that one) misses
    cases["two_targets_at_equal_iou"] = ([_p([[0, 0, 10, 10, 0.9, 1], [0, 5, 10, 10, 0.8, 1], [0, 0, 10, 5, 0.7, 1]])],
                                         [_t([[0, 0, 10, 6], [0, 4, 10, 10]])])
    # equal scores across a hit and a miss, in both orders, inside an image and across images
    hit, miss = [0, 0, 10, 10, 0.5, 1], [50, 50, 60, 60, 0.5, 1]
    cases["equal_scores"] = ([_p([hit, miss, [100, 100, 110, 110, 0.5, 1]]), _p([miss, hit]), _p([miss]), _p([hit])],
                             [_t([[0, 0, 10, 10], [100, 100, 110, 112]])] + [_t([[0, 0, 10, 10]])] * 3)
    # 257 predictions against 10 targets: the max_det cut, recalls of exactly k / 10, quantised scores (many ties)
    g = torch.Generator().manual_seed(11)
    xy = torch.randint(0, 2000, (257, 2), generator=g).float()
    many = torch.cat((xy, xy + torch.randint(5, 40, (257, 2), generator=g)), 1)
    tg = torch.cat((torch.zeros((10, 1)), many[torch.randperm(257, generator=g)[:10]]), 1)
    scores = torch.randint(1, 100, (257, 1), generator=g).float() / 100
    cases["many_predictions"] = ([torch.cat((many, scores, torch.ones((257, 1))), 1)], [tg])
    cases["empty_sides"] = ([None, _p([hit, miss]), _p([hit])], [_t([[0, 0, 10, 10]]), torch.zeros((0, 5)), _t([[0, 0, 10, 10]])])
    cases["no_target_at_all"] = ([_p([hit]), None, _p([miss, hit])], [torch.zeros((0, 5))] * 3)
    return cases


def _check_map(name, outs, tgts):
    outs_d = [None if o is None else o.to(DEV) for o in outs]
    tgts_d = [t.to(DEV) for t in tgts]
    m = detection.match_detections_device(outs_d, tgts_d)
    n_pred, n_gt = m["n_pred"].tolist(), m["n_gt"].tolist()
    for b, (o, t) in enumerate(zip(outs, tgts)):
        order, hits = host_match(o, t)
        assert n_pred[b] == len(order) and n_gt[b] == len(t), (name, b)
        assert m["sel"][b, :len(order)].tolist() == order, (name, b)
        assert m["hits"][b, :len(order)].tolist() == hits, (name, b)
        if o is not None:
            assert torch.equal(m["scores"][b, :len(order)].cpu(), o[order, 4].double()), (name, b)
    pooled_h, pooled_d = detection.map_50(outs, tgts), detection.map_50_device(outs_d, tgts_d)
    per_h = [detection.map_50([o], [t]) for o, t in zip(outs, tgts)]
    per_d = detection.map_50_device(outs_d, tgts_d, per_image=True)
    print(name, "pooled", pooled_h, pooled_d, "per image", per_h, per_d)
    assert abs(pooled_h - pooled_d) <= MAP_BAR, (name, pooled_h, pooled_d)
    assert len(per_d) == len(per_h) and all(abs(a - b) <= MAP_BAR for a, b in zip(per_h, per_d)), (name, per_h, per_d)
    return per_d, pooled_d, m


def test_map_50_device_equals_the_host_case_by_case(golden):
    cases = _map_cases(golden)
    res = {name: _check_map(name, *c) for name, c in cases.items()}
    assert res["g7_known_answers"][0][0] == 0.0 and abs(res["g7_known_answers"][0][1] - 1.0) <= MAP_BAR
    assert abs(res["g7_known_answers"][0][2] - 0.8) <= 0.008                 # the reference's own bar: approx(0.8, 0.01)
    m = res["iou_at_and_below_half"][2]
    assert m["hits"][:, 0].tolist() == [1, 0]
    assert res["two_targets_at_equal_iou"][2]["hits"][0, :3].tolist() == [1, 0, 1]
    assert res["many_predictions"][2]["n_pred"].tolist() == [100]
    assert res["empty_sides"][0][:2] == [0.0, 0.0] and res["no_target_at_all"][1] == 0.0
    assert float(detection.compute_detection_metrics_device([o.to(DEV) for o in cases["many_predictions"][0]],
                                                            [t.to(DEV) for t in cases["many_predictions"][1]])["map"]) == \
        float(detection.compute_detection_metrics(*cases["many_predictions"])["map"])


def test_map_50_device_on_all_cases_as_one_batch(golden):
    """Every image of every case side by side: 17 images with 0..257 predictions and 0..10 targets, six columns."""
    outs, tgts = [], []
    for o, t in _map_cases(golden).values():
        outs += o
        tgts += [x.float() for x in t]
    _check_map("all", outs, tgts)


def test_map_50_device_takes_the_packed_merge_output(g10):
    """rollout boxes -> merge -> mAP without leaving the device: the packed (rows, counts) form, 6-column merged rows."""
    names = [n for n in g10["names"].tolist() if n.startswith("random")][:6] + ["fractional", "sparse257"]
    preds = [torch.from_numpy(g10[f"{n}.pred"]) for n in names]
    tgts = [torch.from_numpy(g10[f"{n}.tgt"]) for n in names]
    pm = detection.merge_boxes_device(*detection.pack_boxes(preds, 7, DEV))
    tm = detection.merge_boxes_device(*detection.pack_boxes(tgts, 5, DEV), target=True)
    per_d = detection.map_50_device(pm, tm, per_image=True)
    pooled_d = detection.map_50_device(pm, tm)
    hp, ht = detection.merge_boxes_batched(preds), detection.merge_boxes_batched(tgts, target=True)
    per_h = [detection.map_50([o], [t]) for o, t in zip(hp, ht)]
    print(per_h, per_d)
    assert max(per_h) > 0 and all(abs(a - b) <= MAP_BAR for a, b in zip(per_h, per_d))
    assert abs(detection.map_50(hp, ht) - pooled_d) <= MAP_BAR


# ---- integration --------------------------------------------------------------------------------------------------------
def _product(P, T, thr):
    images = ragged_ref.image_set(SIZES_64, SEED_64)
    oracle = ragged_ref.build_oracle(SEED_64, P, T, ragged_ref.calib_patches(images, P))
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=thr,
                                  max_det_per_patch=512), max_batch=8)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product, images


def _same_metrics(host, dev):
    assert list(dev) == list(host)
    for k in host:
        assert len(dev[k]) == len(host[k])
        for i, (h, d) in enumerate(zip(host[k], dev[k])):
            if k == "map":
                print("map", i, h, d)
                assert abs(h - d) <= 1e-6, (i, h, d)
            else:
                assert h == d or (h != h and d != d), (k, i, h, d)


@pytest.mark.parametrize("stop,thr", [(True, ragged_ref.THR), (False, ragged_ref.THR), (True, 1e-3)])
def test_eval_on_images_device_metrics_equal_the_host_metrics(stop, thr):
    """The shapes of test_eval_on_images_matches_eval_on_batch_per_image; with the detector's threshold lowered at least
    one image carries more than 64 boxes into the merge."""
    P, T = 64, 6
    product, images = _product(P, T, thr)
    imgs = [im.float().div(255) if i in (2, 5) else im for i, (im, _) in enumerate(images)]
    boxes = [b for _, b in images]
    cfg = dict(T=T, stop=stop, detection_enabled=True, merge_bboxes=True)
    tr_h, tr_d = ja.ReinforceTrainer(_cfg(**cfg), product), ja.ReinforceTrainer(_cfg(**cfg), product)
    host = tr_h.eval_on_images(imgs, boxes, batch_size=4)
    dev = tr_d.eval_on_images(imgs, boxes, batch_size=4, device_metrics=True)
    _same_metrics(host, dev)
    assert tr_d._rollouts == tr_h._rollouts == len(imgs)
    assert len(tr_d.last_return_values) == len(tr_h.last_return_values) == len(imgs)
    for a, b in zip(tr_d.last_return_values, tr_h.last_return_values):
        assert torch.equal(a, b)
    res = ja.infer_images(ja.ReinforceTrainer(_cfg(patch_size=P, **cfg), product), imgs, boxes, sample_actions=False, do_detection=True, batch_size=4)
    counts = [0 if b is None else len(b) for b in res["boxes"]]
    print("boxes per image:", counts)
    if thr < ragged_ref.THR:
        assert max(counts) > 64, counts
        # the rollout's own boxes (not a fixture) through both merges
        host, dev = detection.merge_boxes_batched(res["boxes"]), detection.merge_boxes_batched_device(res["boxes"])
        print("merged boxes per image:", [0 if m is None else len(m) for m in host])
        assert all((h is None and d is None) or torch.equal(h, d) for h, d in zip(host, dev))
    else:
        assert max(counts) > 0


def test_infer_images_device_metrics_equal_the_host_metrics():
    P, T = 64, 6
    product, images = _product(P, T, ragged_ref.THR)
    imgs = [im for im, _ in images]
    targets = [None if i == 3 else b for i, (_, b) in enumerate(images)]

    def run(device_metrics):
        tr = ja.ReinforceTrainer(_cfg(T=T, detection_enabled=True, patch_size=P), product)
        res = ja.infer_images(tr, imgs, targets, sample_actions=False, do_detection=True, batch_size=4, device_metrics=device_metrics)
        return res, tr
    (h, tr_h), (d, tr_d) = run(False), run(True)
    assert list(d["metrics"]) == list(h["metrics"])
    for k, v in h["metrics"].items():
        print(k, v, d["metrics"][k])
        assert abs(v - d["metrics"][k]) <= 1e-6 if k == "map" else v == d["metrics"][k], (k, v, d["metrics"][k])
    assert tr_d._rollouts == tr_h._rollouts == len(imgs)
    for a, b in zip(tr_d.last_return_values, tr_h.last_return_values):
        assert torch.equal(a, b)
    for a, b in zip(h["boxes"], d["boxes"]):
        assert (a is None and b is None) or torch.equal(a, b)
    with pytest.raises(ValueError):
        ja.infer_images(tr_d, imgs, targets, do_detection=True, device_metrics=True)
