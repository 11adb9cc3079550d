"""`postprocess_all_kernel` (candidate policy "all": every passing anchor reaches the NMS) through the context-free
`jn_postprocess_all` against the exact NumPy reference on the committed cases of tests/postprocess_all_cases.py, and the
sticky switch `jn_set_det_candidates` on the paths that run the stage inside a context.  Everything is compared bit for
bit (tests/test_postprocess_all_cases_cpu.py shows why that is fair: the reference equals the uncapped oracle and every
compared IoU is exactly 0, 1/2, 3/4 or 1)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, yolox
from jolineedle_amd._lib import check, ptr
from jolineedle_amd.engine import Engine, make_jn_config
from tests import postprocess_all_cases as pa
from tests import postprocess_cases as pc
from tests.helpers import make_pair, model_config, synth_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7777.0
ISENT = -777
SMALL = [c for c in pc.CASES if c.name not in ("cap-2049", "cap-3000")]   # at most 2048 anchors pass: the policies coincide


def _launch(raw, conf, nms, P, max_out, with_stats=True, entry="jn_postprocess_all"):
    """`entry` on raw [N, A, 6] into sentinel-filled buffers with a guard behind the last patch.  Returns CPU
    (boxes [N * max_out + GUARD_ROWS, 7], counts [N + 2], stats [N + 1, 2])."""
    raw = torch.from_numpy(np.array(raw, np.float32)).to(DEV)
    N, A = raw.shape[0], raw.shape[1]
    boxes = torch.full((N * max_out + pa.GUARD_ROWS, 7), SENTINEL, device=DEV)
    counts = torch.full((N + 2,), ISENT, device=DEV, dtype=torch.int32)
    stats = torch.full((N + 1, 2), ISENT, device=DEV, dtype=torch.int32)
    check(getattr(_lib.load_library(), entry)(ptr(raw), N, A, C.c_float(conf), C.c_float(nms), C.c_float(P - 1), max_out,
                                              ptr(boxes), ptr(counts), ptr(stats) if with_stats else None,
                                              _lib.current_stream(torch.device(DEV))), entry)
    torch.cuda.synchronize()
    return boxes.cpu(), counts.cpu(), stats.cpu()


def _check_patch(boxes, counts, stats, n, max_out, case, ref):
    rows, count, (n_pass, n_keep) = ref
    got = boxes[n * max_out:(n + 1) * max_out]
    assert int(counts[n]) == count, (case.name, int(counts[n]), count)
    assert stats[n].tolist() == [n_pass, n_keep], (case.name, stats[n].tolist(), (n_pass, n_keep))
    want = torch.from_numpy(np.array(rows)).reshape(-1, 7)
    if not torch.equal(got[:count], want):
        bad = (got[:count] != want).any(1).nonzero().flatten().tolist()
        raise AssertionError((case.name, "first differing rows", bad[:5], got[bad[0]].tolist(), want[bad[0]].tolist()))
    assert bool((got[count:] == SENTINEL).all()), (case.name, "rows beyond the count were written")


@functools.lru_cache(maxsize=None)
def _single(case):
    return _launch(pa.build(case)[None], case.conf, case.nms, case.P, case.max_out)


@pytest.mark.parametrize("case", pa.CASES, ids=lambda c: c.name)
def test_kernel_vs_exact_reference(case):
    boxes, counts, stats = _single(case)
    _check_patch(boxes, counts, stats, 0, case.max_out, case, pa.reference(case))
    assert bool((boxes[case.max_out:] == SENTINEL).all()), "the guard behind the last row was written"
    assert counts[1:].tolist() == [ISENT, ISENT] and stats[1].tolist() == [ISENT, ISENT]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_up_to_2048_candidates_the_policies_coincide(case):
    """The first-2048 cases with at most 2048 passing anchors: at A <= 2048 the launcher hands them to postprocess_kernel,
    at A = 4116 the new kernel itself runs on few candidates."""
    boxes, counts, stats = _launch(pc.build(case)[None], case.conf, case.nms, case.P, case.max_out)
    _check_patch(boxes, counts, stats, 0, case.max_out, case, pc.reference(case))
    assert bool((boxes[case.max_out:] == SENTINEL).all()) and counts[1:].tolist() == [ISENT, ISENT]


def test_the_small_cases_reach_both_kernels():
    assert [c for c in pc.CASES if pc.reference(c)[2][0] <= pc.DET_CAP] == SMALL
    assert sum(c.A > pc.DET_CAP for c in SMALL) >= 8 and sum(c.A <= pc.DET_CAP for c in SMALL) >= 8


@pytest.mark.parametrize("launch", pa.launches(), ids=lambda l: f"{l[0]}-{l[1]}-P{l[2]}-K{l[3]}-N{len(l[4])}")
def test_one_launch_of_many_patches_equals_the_single_launches(launch):
    conf, nms, P, max_out, cases = launch
    N = len(cases)
    boxes, counts, stats = _launch(pa.stack(cases), conf, nms, P, max_out)
    for n, case in enumerate(cases):
        _check_patch(boxes, counts, stats, n, max_out, case, pa.reference(case))
        b1, c1, s1 = _single(case)
        assert torch.equal(boxes[n * max_out:(n + 1) * max_out], b1[:max_out]) and counts[n] == c1[0] and torch.equal(stats[n], s1[0])
    assert bool((boxes[N * max_out:] == SENTINEL).all()), "the guard behind the last patch was written"
    assert counts[N:].tolist() == [ISENT, ISENT] and stats[N].tolist() == [ISENT, ISENT]


@pytest.mark.parametrize("name", ["max-out-64", "count-4097", "all-copies-8400", "mixed-300"])
def test_stats_are_optional(name):
    """Without stats the greedy loop may stop at max_out kept boxes: the same boxes and counts either way."""
    case = pa.BY_NAME[name]
    b0, c0, s0 = _launch(pa.build(case)[None], case.conf, case.nms, case.P, case.max_out, with_stats=False)
    b1, c1, _ = _single(case)
    assert torch.equal(b0, b1) and torch.equal(c0, c1) and bool((s0 == ISENT).all())


def test_the_wrapper_routes_by_policy():
    case = pa.BY_NAME["max-out-64"]
    raw = torch.from_numpy(np.array(pa.build(case)))[None].to(DEV)
    boxes, counts, stats = yolox.postprocess(raw, case.conf, case.nms, case.P, case.max_out, candidates="all")
    rows, count, st = pa.reference(case)
    assert boxes.shape == (1, case.max_out, 7) and counts.tolist() == [count] and stats.tolist() == [list(st)]
    assert torch.equal(boxes[0, :count].cpu(), torch.from_numpy(np.array(rows)))
    capped = pc.run(pa.build(case), case.conf, case.nms, case.P, case.max_out)
    for kw in ({}, dict(candidates="first2048")):
        boxes, counts, stats = yolox.postprocess(raw, case.conf, case.nms, case.P, case.max_out, **kw)
        assert counts.tolist() == [capped[1]] and stats.tolist() == [list(capped[2])]
        assert torch.equal(boxes[0, :capped[1]].cpu(), torch.from_numpy(capped[0]))
    assert not np.array_equal(capped[0], rows)


# ---- inside a context ---------------------------------------------------------------------------------------------------
P_HOT = 352                                        # A = 1936 + 484 + 121 = 2541: the smallest multiple of 32 with A > 2048
A_HOT = 2541
HOT_SEED = 9                                       # with these weights every anchor of both patches passes 1e-5


@functools.lru_cache(maxsize=None)
def _hot_product():
    """yolox-nano detector at P = 352, threshold 1e-5, and as many output rows as anchors so that the cut to
    max_det_per_patch hides nothing of the candidate policy."""
    product, _ = make_pair(HOT_SEED, patch_size=P_HOT, block_size=2, image_processor="yolox-nano",
                           detector_conf_threshold=1e-5, max_batch=2, max_det_per_patch=A_HOT)
    product.sync_weights()
    return product


def _detect(eng, x):
    N, K = x.shape[0], eng.cfg.max_det_per_patch
    raw = torch.empty((N, A_HOT, 6), device=DEV)
    boxes = torch.full((N, K, 7), SENTINEL, device=DEV)
    counts = torch.full((N,), ISENT, device=DEV, dtype=torch.int32)
    check(eng.lib.jn_detect(eng.handle, ptr(x), N, ptr(boxes), ptr(counts), ptr(raw), _lib.current_stream(torch.device(DEV))),
          "jn_detect")
    torch.cuda.synchronize()
    return boxes.cpu(), counts.cpu(), raw.cpu()


def test_jn_detect_follows_the_switch_and_the_switch_is_restorable():
    """The hot path: under "all" jn_detect's boxes and counts are jn_postprocess_all of the raw rows it hands back, byte
    for byte, and not jn_postprocess of them; back under "first2048" they are jn_postprocess of them again."""
    N = 2
    product = _hot_product()
    eng = product.engine()
    K, conf, nms = eng.cfg.max_det_per_patch, eng.cfg.det_conf_threshold, eng.cfg.det_nms_threshold
    assert K == A_HOT == sum((P_HOT // s) ** 2 for s in (8, 16, 32)) and abs(conf - 1e-5) < 1e-9
    assert product.det_candidates == "first2048"
    x = torch.rand((N, 3, P_HOT, P_HOT), generator=torch.Generator().manual_seed(3)).to(DEV)
    try:
        product.set_det_candidates("all")
        assert product.det_candidates == "all"
        boxes, counts, raw = _detect(eng, x)
        passing = ((raw[..., 4] * raw[..., 5]) >= conf).sum(1)
        print("passing anchors per patch:", passing.tolist(), "boxes:", counts.tolist())
        assert int(passing.max()) > pc.DET_CAP, passing.tolist()   # a condition of the test: the cap would have cut
        b_all, c_all, s_all = _launch(raw.numpy(), conf, nms, P_HOT, K)
        b_cap, c_cap, s_cap = _launch(raw.numpy(), conf, nms, P_HOT, K, entry="jn_postprocess")
        assert s_all[:N, 0].tolist() == s_cap[:N, 0].tolist() == passing.tolist()
        assert torch.equal(c_all[:N], counts) and torch.equal(b_all[:N * K].view(N, K, 7), boxes)       # sentinels included
        assert not torch.equal(c_cap[:N], counts) or not torch.equal(b_cap[:N * K].view(N, K, 7), boxes)
        with pytest.raises(ValueError):
            product.set_det_candidates("first-2048")
        assert product.det_candidates == "all"
    finally:
        product.set_det_candidates("first2048")
    boxes, counts, raw2 = _detect(eng, x)
    assert torch.equal(raw2, raw)
    assert torch.equal(c_cap[:N], counts) and torch.equal(b_cap[:N * K].view(N, K, 7), boxes)


def test_rollout_detections_under_all_are_the_detector_forward():
    B, T = 2, 2
    product = _hot_product()
    images, bboxes, start = synth_batch(B, 2, 3, P_HOT, seed=4)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P_HOT, T, 1, False)
    tr = ja.ReinforceTrainer(ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=False, reward_norm=True, seed=1), product)
    try:
        product.set_det_candidates("all")
        ro = tr.rollout(env, sample_actions=False, start_positions=start, do_detection=True, keep_patches=True, bbox_lists=False)
        S = ro["actions"].shape[1]
        assert S == T and int(ro["det_counts"].max()) > pc.DET_CAP, ro["det_counts"].tolist()      # the cap would have cut
        for t in range(S + 1):
            outs, _, _ = product.yolox(ro["patches"][:, t])
            for b in range(B):
                c = int(ro["det_counts"][b, t])
                assert (outs[b] is None) == (c == 0) and (c == 0 or (outs[b].shape[0] == c and torch.equal(outs[b], ro["det_boxes"][b, t, :c]))), (b, t)
    finally:
        product.set_det_candidates("first2048")
    capped = tr.rollout(env, sample_actions=False, start_positions=start, do_detection=True, bbox_lists=False)
    assert int(capped["det_counts"].max()) <= pc.DET_CAP and torch.equal(capped["positions"], ro["positions"])


def test_the_config_field_sets_the_policy_at_creation():
    product = ja.GPT(model_config(patch_size=64, block_size=2, image_processor="yolox-nano", det_candidates="all"), max_batch=1)
    assert product.det_candidates == "all"
    with pytest.raises(ValueError):
        ja.GPT(model_config(patch_size=64, block_size=2, image_processor="yolox-nano", det_candidates="every"), max_batch=1)


def test_entry_point_contract():
    lib = _lib.load_library()
    raw = torch.zeros((1, pa.POST_ALL_MAX_A + 1, 6), device=DEV)
    boxes = torch.full((4, 7), SENTINEL, device=DEV)
    counts = torch.full((1,), ISENT, device=DEV, dtype=torch.int32)

    def call(raw_=raw, N=1, A=84, max_out=4, boxes_=boxes, counts_=counts):
        return lib.jn_postprocess_all(ptr(raw_), N, A, C.c_float(0.25), C.c_float(0.45), C.c_float(63.0), max_out, ptr(boxes_),
                                      ptr(counts_), None, _lib.current_stream(torch.device(DEV)))
    assert call(raw_=None) == -1 and b"null" in lib.jn_last_error()
    assert call(boxes_=None) == -1 and call(counts_=None) == -1
    assert call(N=0) == -1 and call(A=0) == -1 and b"A=0" in lib.jn_last_error()
    assert call(max_out=0) == -1 and b"max_out" in lib.jn_last_error()
    assert call(A=pa.POST_ALL_MAX_A + 1) == -1 and b"A=8401" in lib.jn_last_error()
    torch.cuda.synchronize()
    assert bool((boxes == SENTINEL).all()) and int(counts) == ISENT                              # nothing was launched
    for A in (84, pa.POST_ALL_MAX_A):                              # either kernel on a patch where nothing passes
        counts.fill_(ISENT)
        assert call(A=A) == 0
        torch.cuda.synchronize()
        assert bool((boxes == SENTINEL).all()) and int(counts) == 0
    with pytest.raises(_lib.JnError):
        yolox.postprocess(raw, 0.25, 0.45, 64, 4, candidates="all")
    # the switch: JN_ESTATE without a detector, JN_EINVAL beyond 8400 anchors or on a null context
    bare = ja.GPT(model_config(patch_size=64, block_size=2, with_detector=False, image_processor=None), max_batch=1)
    for flag in (0, 1):
        assert lib.jn_set_det_candidates(bare.engine().handle, flag) == -5 and b"detector" in lib.jn_last_error()
    with pytest.raises(_lib.JnError):
        bare.set_det_candidates("all")
    assert bare.det_candidates == "first2048" and lib.jn_set_det_candidates(None, 1) == -1
    big = Engine(make_jn_config(model_config(patch_size=672, block_size=2, image_processor="yolox-nano"), 0, 1, 9))
    assert lib.jn_set_det_candidates(big.handle, 1) == -1 and b"A=9261" in lib.jn_last_error()
    assert lib.jn_set_det_candidates(big.handle, 0) == 0
