"""The multistart evaluation on the device: ``jn_pool_walk_detections`` against the host rule (which
tests/test_multistart_cpu.py holds to the reference's loops) with ``torch.equal``, ``jn_average_precision_segments``
against ``map_50`` over each segment's lists, and ``SupervisedTrainer.eval_envs_on_images`` with device metrics against
host metrics and against a loop of one-image calls.

Bars.  Pool: every stored value is a copy and every decision an fp32 comparison both sides round alike: exact.  mAP
1e-12: the bar and derivation of tests/test_gpu_detection_eval.py (same IEEE fp64 operations; 101 * 101 * 2**-53).
`map*` of the integration tests are stored as fp32: 1e-6.  Across batch sizes: the bars of
tests/test_gpu_ragged_batch.py (equal positions under its logit-gap precondition, values to a relative 1e-5)."""
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, detection, ragged
from jolineedle_amd._lib import ptr
from jolineedle_amd.config import model_config
from tests import multistart_cases as mc
from tests import ragged_ref
from tests.ragged_ref import LOGIT_GAP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAP_BAR = 1e-12


def device_pool(pr, n_starts=None, M=None):
    count = pr["walk_count"] if n_starts is None else [n_starts] * len(pr["walk_count"])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return detection.pool_walk_detections_device(pr["det_boxes"].to(DEV), pr["det_counts"].to(DEV), pr["positions"].to(DEV),
                                                 i32(pr["walk_tokens"]), i32(pr["walk_first"]), i32(count), max(count), pr["grid"],
                                                 pr["M"] if M is None else M)


def host_pool(pr):
    return detection.pool_walk_detections(pr["det_boxes"], pr["det_counts"], pr["positions"], pr["walk_tokens"], pr["walk_first"],
                                          pr["walk_count"], pr["grid"], pr["M"])


def assert_same_pool(dev, host):
    got = mc.unpack_device_pool(dev)
    assert torch.equal(got["visited"], host["visited"])
    assert torch.equal(got["stats"], host["stats"])
    for i, cells in enumerate(host["boxes"]):
        for c, want in enumerate(cells):
            assert int(got["counts"][i, c]) == (0 if want is None else len(want)), (i, c)
            assert (want is None) == (got["boxes"][i][c] is None), (i, c)
            if want is not None:
                assert torch.equal(got["boxes"][i][c], want), (i, c, got["boxes"][i][c], want)


# ---- the pool kernel --------------------------------------------------------------------------------------------------
def test_pool_kernel_equals_the_host_rule_on_every_case_in_one_launch():
    pr = mc.combine(list(mc.cases().values()))
    assert bool(torch.isnan(pr["det_boxes"]).any())                        # NaN beyond every count: never read
    host = host_pool(pr)
    mc.assert_pool_equals_reference(pr, host)
    dev = device_pool(pr)
    assert_same_pool(dev, host)
    assert int(dev["stats"][..., 1].max()) > pr["M"]                       # a reached cap shows in the stats
    # rows beyond a count are left alone
    pre = torch.full_like(dev["boxes"], -7.0)
    lib = _lib.load_library()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    b, c, p = pr["det_boxes"].to(DEV), pr["det_counts"].to(DEV), pr["positions"].to(DEV)
    cnt, vis = torch.empty_like(dev["counts"]), torch.empty(dev["counts"].shape, dtype=torch.uint8, device=DEV)
    A, S1, K = b.shape[:3]
    assert lib.jn_pool_walk_detections(ptr(b), ptr(c), ptr(p), ptr(i32(pr["walk_tokens"])), ptr(i32(pr["walk_first"])),
                                       ptr(i32(pr["walk_count"])), A, S1 - 1, S1 - 1, K, len(pr["rows"]), 2, *pr["grid"], pr["M"],
                                       ptr(pre), ptr(cnt), None, ptr(vis), _lib.current_stream(DEV)) == 0      # stats may be NULL
    assert torch.equal(cnt, dev["counts"])
    rows = torch.arange(pr["M"], device=DEV)[None, None, :] < cnt[..., None]
    assert bool((pre[~rows] == -7).all()) and torch.equal(pre[rows], dev["boxes"][rows])
    # the prefix k = 1 of the same buffers
    assert_same_pool(device_pool(pr, n_starts=1),
                     detection.pool_walk_detections(pr["det_boxes"], pr["det_counts"], pr["positions"], pr["walk_tokens"],
                                                    pr["walk_first"], [1] * len(pr["rows"]), pr["grid"], pr["M"]))


def test_pool_kernel_reads_a_slice_of_longer_rollout_buffers_in_place():
    """``eval_envs_on_images`` hands the kernel the [:, :S + 1] slices of the rollout's [A, T + 1, ...] buffers: the walk
    stride is T + 1 tokens, the token limit S + 1.  Every CPU case again, inside buffers 3 tokens longer whose extra tokens
    stand on cell (0, 0) with full counts of real boxes, and with every second walk claiming more tokens than the slice
    holds: the extra tokens change nothing, through the wrapper and through the entry itself (T != S)."""
    pr = mc.combine(list(mc.cases().values()))
    A, S1, K = pr["det_boxes"].shape[:3]
    T1 = S1 + 3
    g = torch.Generator().manual_seed(9)
    xy = torch.rand((A, T1, K, 2), generator=g) * 40
    long_boxes = torch.cat((xy, xy + 8, torch.rand((A, T1, K, 1), generator=g), torch.zeros((A, T1, K, 2))), -1)
    long_counts = torch.full((A, T1), K, dtype=torch.int32)
    long_pos = torch.zeros((A, T1, 2), dtype=torch.int64)
    long_boxes[:, :S1], long_counts[:, :S1], long_pos[:, :S1] = pr["det_boxes"], pr["det_counts"], pr["positions"]
    tokens = [t + (T1 if a % 2 and t == S1 else 0) for a, t in enumerate(pr["walk_tokens"])]
    assert any(t > S1 for t in tokens)
    host = host_pool(pr)
    b, c, p = long_boxes.to(DEV), long_counts.to(DEV), long_pos.to(DEV)
    sliced = dict(pr, det_boxes=b[:, :S1], det_counts=c[:, :S1], positions=p[:, :S1], walk_tokens=tokens)
    assert not sliced["det_boxes"].is_contiguous() and sliced["det_counts"].stride(0) == T1
    assert_same_pool(device_pool(sliced), host)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    NI, cells, M = len(pr["rows"]), pr["grid"][0] * pr["grid"][1], pr["M"]
    out = torch.zeros((NI, cells, M, 7), device=DEV)
    cnt, stats = torch.empty((NI, cells), dtype=torch.int32, device=DEV), torch.empty((NI, cells, 2), dtype=torch.int32, device=DEV)
    vis = torch.empty((NI, cells), dtype=torch.uint8, device=DEV)
    assert _lib.load_library().jn_pool_walk_detections(ptr(b), ptr(c), ptr(p), ptr(i32(tokens)), ptr(i32(pr["walk_first"])),
                                                       ptr(i32(pr["walk_count"])), A, T1 - 1, S1 - 1, K, NI, max(pr["walk_count"]),
                                                       *pr["grid"], M, ptr(out), ptr(cnt), ptr(stats), ptr(vis),
                                                       _lib.current_stream(DEV)) == 0
    assert_same_pool({"boxes": out, "counts": cnt, "stats": stats, "visited": vis.bool()}, host)


def _lattice_pool(n, seed):
    """n boxes on an integer lattice: 4 x 4 boxes 8 px apart (IoU 0 between sites) and, on the same sites, their shadows
    at IoU exactly 3/4 (4 x 3) and 1/2 (4 x 2) and copies of all three; scores from five values (ties everywhere)."""
    g = torch.Generator().manual_seed(seed)
    site = torch.randint(0, max(2, n // 3), (n,), generator=g)
    x0, y0 = (site % 64) * 8.0, (site // 64) * 8.0
    hgt = torch.tensor([4.0, 3.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    score = torch.randint(1, 6, (n,), generator=g).float() / 8
    return torch.stack((x0, y0, x0 + 4, y0 + hgt, score, torch.rand(n, generator=g), torch.zeros(n)), 1)


def _float_pool(n, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((n, 2), generator=g) * 60
    wh = 2 + torch.rand((n, 2), generator=g) * 30
    return torch.cat((xy, xy + wh, torch.rand((n, 1), generator=g), torch.ones((n, 1)), torch.zeros((n, 1))), 1)


def _single_cell_problem(pools, S1=64, K=64):
    """Every pool on one cell of an image of its own: one walk whose S1 tokens all stand on (0, 0), K boxes per token."""
    A = len(pools)
    det = torch.full((A, S1, K, 7), float("nan"))
    cnt = torch.zeros((A, S1), dtype=torch.int32)
    for a, pool in enumerate(pools):
        for t in range(S1):
            part = pool[t * K:(t + 1) * K]
            cnt[a, t] = len(part)
            det[a, t, :len(part)] = part
    return {"det_boxes": det, "det_counts": cnt, "positions": torch.zeros((A, S1, 2), dtype=torch.int64), "walk_tokens": [S1] * A,
            "walk_first": list(range(A)), "walk_count": [1] * A, "rows": [None] * A, "grid": (1, 1), "M": 4096}


def test_pool_kernel_at_the_block_and_lds_boundaries():
    """Pool sizes around the multiples of the 256 threads and at the 4096 boxes the LDS holds (96 KB), plus one pool of
    random floats whose closest IoU to the threshold is printed."""
    sizes = [1, 255, 256, 257, 1023, 1025, 4096]
    pools = [_lattice_pool(n, 100 + n) for n in sizes] + [_float_pool(1500, 5)]
    pr = _single_cell_problem(pools)
    host = host_pool(pr)
    dev = device_pool(pr)
    assert dev["stats"][:, 0, 0].tolist() == sizes + [1500]
    print("pool -> survivors:", dict(zip(sizes + ["float1500"], dev["stats"][:, 0, 1].tolist())))
    assert_same_pool(dev, host)
    for i, n in enumerate(sizes[1:], 1):
        assert 0 < int(dev["stats"][i, 0, 1]) < n                           # something suppressed, something kept
    f = pools[-1]
    lt, rb = torch.maximum(f[:, None, :2], f[None, :, :2]), torch.minimum(f[:, None, 2:4], f[None, :, 2:4])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = (f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1])
    iou32 = inter / ((area[:, None] + area[None, :]) - inter)
    print(f"random-float pool: smallest |iou32 - 0.5| = {float((iou32 - 0.5).abs().min()):.3e}")
    # the cap on the same buffers: the first M survivors, the stats unchanged
    capped = device_pool(pr, M=3)
    assert torch.equal(capped["stats"], dev["stats"]) and capped["counts"].flatten().tolist() == [min(3, s) for s in dev["stats"][:, 0, 1].tolist()]
    for i in range(len(pools)):
        k = int(capped["counts"][i, 0])
        assert torch.equal(capped["boxes"][i, 0, :k], dev["boxes"][i, 0, :k])


def test_pool_abi_refuses_a_pool_of_4097_without_a_launch():
    lib = _lib.load_library()
    boxes = torch.zeros((1, 1, 4097, 7), device=DEV)
    counts = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    pos = torch.zeros((1, 1, 2), dtype=torch.int64, device=DEV)
    one, zero = torch.ones((1,), dtype=torch.int32, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
    out = torch.full((1, 1, 4, 7), -7.0, device=DEV)
    cnt, stats = torch.full((1, 1), -7, dtype=torch.int32, device=DEV), torch.full((1, 1, 2), -7, dtype=torch.int32, device=DEV)
    vis = torch.full((1, 1), 249, dtype=torch.uint8, device=DEV)
    rc = lib.jn_pool_walk_detections(ptr(boxes), ptr(counts), ptr(pos), ptr(one), ptr(zero), ptr(one), 1, 0, 0, 4097, 1, 1, 1, 1, 4,
                                     ptr(out), ptr(cnt), ptr(stats), ptr(vis), _lib.current_stream(DEV))
    assert rc == -1                                                          # JN_EINVAL
    msg = lib.jn_last_error().decode()
    assert "jn_pool_walk_detections" in msg and "4097" in msg and "4096" in msg
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(cnt) == -7 and bool((stats == -7).all()) and int(vis) == 249
    # the wrapper pools such a shape on the host
    pr = _single_cell_problem([_lattice_pool(300, 1)], S1=1, K=4097)
    pr["M"] = 8
    assert_same_pool(device_pool(pr), host_pool(pr))


# ---- segmented average precision --------------------------------------------------------------------------------------
def _units():
    """23 units (cells): predictions [n, 7] or None and targets [m, 5], a few of them empty on either side."""
    g = torch.Generator().manual_seed(21)
    outs, tgts = [], []
    for u in range(23):
        m = int(torch.randint(0, 4, (1,), generator=g)) if u % 5 else 0
        xy = torch.randint(0, 40, (m, 2), generator=g).float()
        t = torch.cat((torch.zeros((m, 1)), xy, xy + torch.randint(8, 20, (m, 2), generator=g)), 1)
        n = int(torch.randint(0, 7, (1,), generator=g)) if u % 4 else 0
        pxy = torch.randint(0, 40, (n, 2), generator=g).float()
        p = torch.cat((pxy, pxy + torch.randint(8, 20, (n, 2), generator=g), torch.randint(1, 9, (n, 1), generator=g).float() / 8,
                       torch.ones((n, 1)), torch.zeros((n, 1))), 1)
        k = min(n, m)
        if k:
            p[:k, :4] = t[:k, 1:5]                                            # some exact hits
        outs.append(p if n else None), tgts.append(t)
    return outs, tgts


def test_segmented_average_precision_equals_map_50_per_segment():
    outs, tgts = _units()
    U = len(outs)
    outs_d, tgts_d = [None if o is None else o.to(DEV) for o in outs], [t.to(DEV) for t in tgts]
    # one unit, many units, uneven offsets, an empty segment; unit 0 has no target and no prediction
    seg = [0, 1, 2, 9, 9, 12, 20, U]
    want = detection.map_50_segments(outs, tgts, seg)
    got = detection.map_50_segments_device(outs_d, tgts_d, seg)
    print("segments", want, got)
    assert len(got) == len(seg) - 1 and all(abs(a - b) <= MAP_BAR for a, b in zip(want, got))
    assert max(want) > 0 and want[0] == got[0] == 0.0 and got[3] == 0.0
    # a segment without targets and one without predictions
    no_t = [i for i, t in enumerate(tgts) if len(t) == 0 and outs[i] is not None][0]
    no_p = [i for i, o in enumerate(outs) if o is None and len(tgts[i])][0]
    for u in (no_t, no_p):
        assert detection.map_50_segments_device(outs_d, tgts_d, [u, u + 1]) == [0.0] == detection.map_50_segments(outs, tgts, [u, u + 1])
    # one segment over all units IS the pooled entry
    m = detection.match_detections_device(outs_d, tgts_d, 100)
    pooled = detection.average_precision_device(m, pooled=True)
    whole = detection.average_precision_segments_device(m, torch.tensor([0, U], dtype=torch.int32), U)
    assert torch.equal(pooled, whole) and abs(float(whole) - detection.map_50(outs, tgts)) <= MAP_BAR
    # and one segment per unit the per-image entry
    per = detection.average_precision_device(m, pooled=False)
    assert torch.equal(per, detection.average_precision_segments_device(m, torch.arange(U + 1, dtype=torch.int32), 1))
    # the slot count follows the rows a unit can offer: 92 units x min(100, 6 rows) fit where 92 x 100 slots would not
    assert abs(detection.map_50_segments_device(outs_d * 4, tgts_d * 4, [0, 4 * U])[0] - detection.map_50(outs * 4, tgts * 4)) <= MAP_BAR


def test_existing_average_precision_entry_is_unchanged():
    """The inputs of test_gpu_detection_eval.py's "equal_scores" and "two_targets_at_equal_iou" cases through the
    existing entry, before and after the segmented entry ran on the same match."""
    p = lambda rows: torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)
    t = lambda rows: torch.tensor([[0] + list(r) for r in rows], dtype=torch.float32).reshape(-1, 5)
    hit, miss = [0, 0, 10, 10, 0.5, 1], [50, 50, 60, 60, 0.5, 1]
    outs = [p([hit, miss, [100, 100, 110, 110, 0.5, 1]]), p([miss, hit]), p([miss]), p([hit]),
            p([[0, 0, 10, 10, 0.9, 1], [0, 5, 10, 10, 0.8, 1], [0, 0, 10, 5, 0.7, 1]])]
    tgts = [t([[0, 0, 10, 10], [100, 100, 110, 112]])] + [t([[0, 0, 10, 10]])] * 3 + [t([[0, 0, 10, 6], [0, 4, 10, 10]])]
    m = detection.match_detections_device([o.to(DEV) for o in outs], [x.to(DEV) for x in tgts])
    before = (detection.average_precision_device(m, pooled=False), detection.average_precision_device(m, pooled=True))
    detection.average_precision_segments_device(m, torch.tensor([0, 2, 5], dtype=torch.int32), 3)
    after = (detection.average_precision_device(m, pooled=False), detection.average_precision_device(m, pooled=True))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    per_h = [detection.map_50([o], [x]) for o, x in zip(outs, tgts)]
    assert all(abs(a - b) <= MAP_BAR for a, b in zip(per_h, after[0].tolist()))
    assert abs(detection.map_50(outs, tgts) - float(after[1])) <= MAP_BAR


# ---- integration ------------------------------------------------------------------------------------------------------
SIZES = [(100, 150), (64, 128), (180, 120), (130, 200), (100, 150)]          # five images, four sizes
SEED = 0
KD = 64                                                                      # 4 walks x 7 tokens x 64 boxes stays below 4096


def _product(P, T, thr=1e-3, max_batch=20):
    images = ragged_ref.image_set(SIZES, SEED)
    oracle = ragged_ref.build_oracle(SEED, P, T, ragged_ref.calib_patches(images, P))
    # boxes of positive area: the seeded regression heads give boxes that collapse to a line or leave the patch and are
    # clamped to zero area; with the regression outputs at 0 every candidate is its anchor's own stride x stride square
    # (cut at the patch border), and only the scores depend on the image
    with torch.no_grad():
        for conv in oracle.yolox.head.reg_preds:
            conv.weight.zero_(), conv.bias.zero_()
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=thr,
                                  max_det_per_patch=KD), max_batch=max_batch)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product, [im for im, _ in images], [b for _, b in images]


def _trainer(product, P, T):
    return ja.SupervisedTrainer(ja.CfgNode(patch_size=P, max_seq_len=4, test_max_seq_len=T, stop_enabled=True, seed=1,
                                           detection_enabled=True), product)


def _close(a, b, rel=1e-5):
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-30) or a == b


WALK_KEYS = ("prop_patches_found", "episode_length", "teacher_agreement", "stopped_inside_bbox")


@pytest.fixture(scope="module")
def runs():
    """One model, K = 2 multistart on five images: device metrics, host metrics, and the loop of one-image calls."""
    P, T = 64, 6
    product, imgs, boxes = _product(P, T)
    out = {"P": P, "T": T, "product": product, "imgs": imgs, "boxes": boxes}
    for name, dm in (("device", True), ("host", False)):
        tr = _trainer(product, P, T)
        out[name] = (tr.eval_envs_on_images(imgs, boxes, batch_size=5, device_metrics=dm), tr.last_eval_rollouts, tr)
    tr = _trainer(product, P, T)
    loop, walks = {}, []
    for im, b in zip(imgs, boxes):                       # the reference's form: one image at a time, host pooling
        for k, v in tr.eval_envs_on_images([im], [b], batch_size=1, device_metrics=False).items():
            loop.setdefault(k, []).extend(v)
        walks += tr.last_eval_rollouts
    out["loop"] = (loop, walks, tr)
    return out


def test_eval_envs_device_metrics_equal_host_metrics(runs):
    dev, host = runs["device"][0], runs["host"][0]
    n = len(runs["imgs"])
    assert list(dev) == list(host)
    per_image = [f"{m}{s}" for s in ("", "_multistart_2") for m in ("map_traj", "prop_patches_found_traj", "map")]
    assert set(dev) == set(WALK_KEYS) | set(per_image)
    for k in dev:
        assert len(dev[k]) == len(host[k]) == (2 * n if k in WALK_KEYS else n), k
        for i, (h, d) in enumerate(zip(host[k], dev[k])):
            if k.startswith("map"):
                print(k, i, h, d)
                assert abs(h - d) <= 1e-6, (k, i, h, d)
            else:
                assert h == d, (k, i, h, d)
    # (a seeded detector rarely hits a target: test_walk_cell_maps_on_the_rollouts_own_boxes scores the same boxes
    # against targets cut from them)
    assert all(a <= b + 1e-6 for a, b in zip(dev["map"], dev["map_traj"]))              # false negatives only lower it
    assert all(a <= b for a, b in zip(dev["prop_patches_found_traj"], dev["prop_patches_found_traj_multistart_2"]))
    for name in ("device", "host"):
        tr = runs[name][2]
        assert tr._eval_runner()._rollouts == 2 * n                                       # first - 1 + n_images * K
        stats = tr.last_eval_pool_stats[0]
        assert stats.shape[:2] == (2, n) and int(stats[..., 0].max()) > 0
    assert torch.equal(runs["device"][2].last_eval_pool_stats[0], runs["host"][2].last_eval_pool_stats[0])


def test_eval_envs_batched_equals_the_loop_of_single_images(runs):
    (bat, bw, _), (loop, lw, tr) = runs["device"], runs["loop"]
    n = len(runs["imgs"])
    assert len(bw) == len(lw) == 2 * n and tr._eval_runner()._rollouts == 2 * n
    for a, walk in enumerate(lw):
        top = walk["logits"].topk(2, dim=-1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        print(f"walk {a}: steps {walk['actions'].numel()} top-2 logit gap {gap:.3e}")
        assert gap >= LOGIT_GAP, f"precondition: walk {a} has a top-2 logit gap of {gap}"
    for a, (x, y) in enumerate(zip(bw, lw)):
        for k in ("actions", "positions", "teacher_sets"):
            assert torch.equal(x[k], y[k]), (a, k)
    assert list(bat) == list(loop)
    for k in bat:
        for i, (x, y) in enumerate(zip(bat[k], loop[k])):
            print(k, i, x, y)
            assert (x == y) if k in WALK_KEYS else _close(x, y), (k, i, x, y)
    # the two walks of an image start where the per-image loop's resets put them, and differ somewhere
    runner = runs["device"][2]._eval_runner()
    ext = [(-(-im.shape[-2] // runs["P"]), -(-im.shape[-1] // runs["P"])) for im in runs["imgs"]]
    want = ragged.walk_start_positions(runner, 1, list(range(n)), ext, 2, "multistart").reshape(-1, 2)
    assert [w["positions"][0].tolist() for w in bw] == want.tolist()
    assert any(bw[2 * i]["positions"][0].tolist() != bw[2 * i + 1]["positions"][0].tolist() for i in range(n))


def test_rollouts_mode_with_greedy_actions_reports_the_single_walk(runs):
    """Two greedy walks from one start are the same walk: every pooled box meets its copy at IoU 1 and is suppressed, so
    k = 2 reports what k = 1 reports — provided no box has zero area (two such copies would both stay)."""
    P, T, product = runs["P"], runs["T"], runs["product"]
    imgs, boxes = runs["imgs"], runs["boxes"]
    tr = _trainer(product, P, T)
    res = tr.eval_envs_on_images(imgs, boxes, batch_size=5, eval_mode="rollouts", n_starts=2)
    walks = tr.last_eval_rollouts
    starts = torch.stack([w["positions"][0] for w in walks[::2]])                  # (K changes the rollout numbers of the starts)
    one = _trainer(product, P, T).eval_envs_on_images(imgs, boxes, batch_size=5, eval_mode="rollouts", start_positions=starts.unsqueeze(1))
    for i in range(len(imgs)):
        assert torch.equal(walks[2 * i]["positions"], walks[2 * i + 1]["positions"])
    # the precondition: no zero-area box among the detections
    env = ragged.image_env(tr._eval_runner(), imgs, boxes)
    ro = tr._eval_runner().rollout(env, do_detection=True, sample_actions=False, bbox_lists=False, token_positions="sequence",
                                   start_positions=starts)
    live = torch.arange(KD, device=DEV)[None, None, :] < ro["det_counts"][..., None]
    b = ro["det_boxes"][live]
    assert len(b) > 0 and bool(((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])).all()), "precondition: a zero-area box"
    stats = tr.last_eval_pool_stats[0]                                            # [K, n, cells, 2]
    assert int(stats[1, ..., 0].sum()) == 2 * int(stats[0, ..., 0].sum()) > 0     # every box pooled twice ...
    assert torch.equal(stats[1, ..., 1], stats[0, ..., 1])                        # ... and its copy suppressed
    for m in ("map_traj", "prop_patches_found_traj", "map"):
        assert res[m + "_rollouts_2"] == res[m], m
        assert all(_close(a, b) for a, b in zip(res[m], one[m])), m                # the K = 1 run is another batch size


def test_corners_mode_walks_from_the_four_corners_of_every_grid(runs):
    P, T, product = runs["P"], runs["T"], runs["product"]
    imgs, boxes = runs["imgs"][:3], runs["boxes"][:3]
    tr = _trainer(product, P, T)
    res = tr.eval_envs_on_images(imgs, boxes, batch_size=3, eval_mode="corners")
    assert len(tr.last_eval_rollouts) == 12 and len(res["episode_length"]) == 12 and len(res["map"]) == 3
    assert all(f"{m}_corners_{k}" in res for m in ("map", "map_traj", "prop_patches_found_traj") for k in (2, 3, 4))
    for i, im in enumerate(imgs):
        gh, gw = -(-im.shape[-2] // P), -(-im.shape[-1] // P)
        got = [tr.last_eval_rollouts[4 * i + k]["positions"][0].tolist() for k in range(4)]
        assert got == [[0, 0], [gh - 1, 0], [gh - 1, gw - 1], [0, gw - 1]], (i, got)
    # explicit starts override the mode (and its K)
    given = torch.tensor([[[0, 0]], [[0, 1]], [[1, 0]]])
    res = tr.eval_envs_on_images(imgs, boxes, batch_size=3, eval_mode="multistart", n_starts=2, start_positions=given)
    assert [w["positions"][0].tolist() for w in tr.last_eval_rollouts] == given.reshape(-1, 2).tolist() and len(res["map"]) == 3
    with pytest.raises(AssertionError, match="max_batch"):
        tr.eval_envs_on_images(runs["imgs"], runs["boxes"], batch_size=6, eval_mode="corners")    # 6 x 4 walks > max_batch 20


@pytest.fixture(scope="module")
def chunk(runs):
    """The one chunk of a K = 2 multistart run as the walker yields it."""
    tr = _trainer(runs["product"], runs["P"], runs["T"])
    return list(tr._eval_walks(runs["imgs"], runs["boxes"], 5, True, walks=2))[-1]


def test_walk_cell_maps_on_the_rollouts_own_boxes(runs, chunk):
    """The rollout's own detections through pool + match + segmented AP on the device against the host functions, scored
    against targets cut from the detections themselves (every second survivor of every second visited cell, edges rounded
    to whole pixels), so that hits, misses and false negatives all occur."""
    P, K = runs["P"], 2
    env, ro, steps = chunk["env"], chunk["rollout"], chunk["steps"]
    n, grid = len(runs["imgs"]), (env.n_vertical_patches, env.n_horizontal_patches)
    tokens = torch.tensor([s + 1 for s in steps], dtype=torch.int32)
    first = torch.arange(n, dtype=torch.int32) * K
    some = False
    for k in (1, 2):
        count = torch.full((n,), k, dtype=torch.int32)
        dev = detection.pool_walk_detections_device(ro["det_boxes"], ro["det_counts"], ro["positions"], tokens.to(DEV), first.to(DEV),
                                                    count.to(DEV), k, grid, 64)
        host = detection.pool_walk_detections(ro["det_boxes"], ro["det_counts"], ro["positions"], tokens, first, count, grid, 64)
        assert_same_pool(dev, host)
        cells = grid[0] * grid[1]
        tg, tc = torch.zeros((n, cells, 4, 5)), torch.zeros((n, cells), dtype=torch.int32)
        target_cells = torch.zeros((n, cells), dtype=torch.bool)
        for i in range(n):
            target_cells[i, (i * 3) % cells] = True                              # a target cell, visited or not
            for c in range(cells):
                rows = host["boxes"][i][c]
                if rows is not None and len(rows) and c % 2 == 0:
                    pick = rows[::2][:4, :4].round()
                    tg[i, c, :len(pick), 1:], tc[i, c] = pick, len(pick)
                elif target_cells[i, c]:
                    tg[i, c, 0, 1:], tc[i, c] = torch.tensor([1.0, 1.0, 20.0, 20.0]), 1
        want = detection.walk_cell_maps(host, tg, tc, target_cells)
        got = detection.walk_cell_maps_device(dev, tg.to(DEV), tc.to(DEV), target_cells.to(DEV)).tolist()
        print("k", k, "map_traj", want[0], got[0], "map", want[1], got[1])
        for v in (0, 1):
            assert all(abs(a - b) <= MAP_BAR for a, b in zip(want[v], got[v])), (k, v, want[v], got[v])
        some = some or (0 < max(want[0]) and any(a < b for a, b in zip(want[1], want[0])))
    assert some, "no cell scores, or no false negative lowers a value: the comparison is empty"


def test_last_token_detections_and_shared_storage(runs, chunk):

    """The tokens of a walk include the patch its last step reached (src/supervised.py:354-363): the detections stored
    at token steps[a] are jn_detect's on the patch gathered at the walk's final position.  And the K walks of an image
    read ONE stored image: the rows of the view table carry the same source address."""
    P, T, product = runs["P"], runs["T"], runs["product"]
    imgs, boxes, K = runs["imgs"], runs["boxes"], 2
    env, ro, steps = chunk["env"], chunk["rollout"], chunk["steps"]
    table = env.views.table_host()
    src = [table[a].src for a in range(len(imgs) * K)]
    assert all(src[i * K] == src[i * K + 1] for i in range(len(imgs))) and len(set(src)) == len(imgs)
    assert [s.data_ptr() for s in env.views.sources] == src
    A = len(steps)
    final = torch.stack([ro["positions"][a, steps[a]] for a in range(A)])
    patches = env.views.gather(torch.arange(A), final, P)
    out, _, _ = product.yolox(patches)
    n = 0
    for a in range(A):
        k = int(ro["det_counts"][a, steps[a]])
        assert (out[a] is None) == (k == 0), a
        if k:
            got = ro["det_boxes"][a, steps[a], :k]
            assert got.shape == out[a].shape and float((got[:, :4] - out[a][:, :4]).abs().max()) <= 2e-3, a
            assert float((got[:, 4:] - out[a][:, 4:]).abs().max()) <= 1e-5, a
            n += k
    assert n > 0, "no final patch holds a box: the comparison is empty"
