"""`postprocess_kernel` through the context-free `jn_postprocess` against the exact NumPy reference on the committed cases of
tests/postprocess_cases.py: scores and IoUs exactly on their thresholds, equal scores decided by the anchor index, a box
that overlaps only a suppressed one, zero-area boxes, clamping after the NMS, both silent caps (2048 candidates,
max_out) with their counters, candidate counts around the powers of two, 2048 greedy rounds.  Everything is compared bit for
bit (tests/test_postprocess_cases_cpu.py shows why that is fair: the reference equals the oracle and every IoU comparison
stands 16 x the fp32 IoU's error away from the threshold or exactly on it)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from jolineedle_amd import _lib, yolox
from jolineedle_amd._lib import check, ptr
from tests import postprocess_cases as pc
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7777.0
ISENT = -777


def _launch(raw, conf, nms, P, max_out, with_stats=True):
    """jn_postprocess on raw [N, A, 6] into sentinel-filled buffers with a guard behind the last patch.  Returns CPU
    (boxes [N * max_out + GUARD_ROWS, 7], counts [N + 2], stats [N + 1, 2])."""
    raw = torch.from_numpy(np.array(raw, np.float32)).to(DEV)
    N, A = raw.shape[0], raw.shape[1]
    boxes = torch.full((N * max_out + pc.GUARD_ROWS, 7), SENTINEL, device=DEV)
    counts = torch.full((N + 2,), ISENT, device=DEV, dtype=torch.int32)
    stats = torch.full((N + 1, 2), ISENT, device=DEV, dtype=torch.int32)
    check(_lib.load_library().jn_postprocess(ptr(raw), N, A, C.c_float(conf), C.c_float(nms), C.c_float(P - 1), max_out, ptr(boxes),
                                             ptr(counts), ptr(stats) if with_stats else None,
                                             _lib.current_stream(torch.device(DEV))), "jn_postprocess")
    torch.cuda.synchronize()
    return boxes.cpu(), counts.cpu(), stats.cpu()


def _check_patch(boxes, counts, stats, n, max_out, case):
    rows, count, (n_pass, n_keep) = pc.reference(case)
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
    return _launch(pc.build(case)[None], case.conf, case.nms, case.P, case.max_out)


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_kernel_vs_exact_reference(case):
    boxes, counts, stats = _single(case)
    _check_patch(boxes, counts, stats, 0, case.max_out, case)
    assert bool((boxes[case.max_out:] == SENTINEL).all()), "the guard behind the last row was written"
    assert counts[1:].tolist() == [ISENT, ISENT] and stats[1].tolist() == [ISENT, ISENT]


@pytest.mark.parametrize("launch", pc.launches(), ids=lambda l: f"{l[0]}-{l[1]}-P{l[2]}-K{l[3]}-N{len(l[4])}")
def test_one_launch_of_many_patches_equals_the_single_launches(launch):
    conf, nms, P, max_out, cases = launch
    N = len(cases)
    boxes, counts, stats = _launch(pc.stack(cases), conf, nms, P, max_out)
    for n, case in enumerate(cases):
        _check_patch(boxes, counts, stats, n, max_out, case)
        b1, c1, s1 = _single(case)
        assert torch.equal(boxes[n * max_out:(n + 1) * max_out], b1[:max_out]) and counts[n] == c1[0] and torch.equal(stats[n], s1[0])
    assert bool((boxes[N * max_out:] == SENTINEL).all()), "the guard behind the last patch was written"
    assert counts[N:].tolist() == [ISENT, ISENT] and stats[N].tolist() == [ISENT, ISENT]


def test_stats_are_optional_and_the_wrapper_returns_zero_filled_rows():
    case = pc.BY_NAME["max-out-4"]
    b0, c0, s0 = _launch(pc.build(case)[None], case.conf, case.nms, case.P, case.max_out, with_stats=False)
    b1, c1, _ = _single(case)
    assert torch.equal(b0, b1) and torch.equal(c0, c1) and bool((s0 == ISENT).all())
    case = pc.BY_NAME["clusters-525"]
    boxes, counts, stats = yolox.postprocess(torch.from_numpy(np.array(pc.build(case)))[None].to(DEV), case.conf, case.nms, case.P,
                                             case.max_out)
    rows, count, st = pc.reference(case)
    assert boxes.shape == (1, case.max_out, 7) and counts.tolist() == [count] and stats.tolist() == [list(st)]
    assert torch.equal(boxes[0, :count].cpu(), torch.from_numpy(np.array(rows))) and bool((boxes[0, count:] == 0).all())


def test_jn_detect_runs_the_same_stage():
    """The hot path: jn_detect's boxes and counts are jn_postprocess of the raw rows it hands back, byte for byte."""
    P, N = 64, 2
    product, _ = make_pair(9, patch_size=P, block_size=4, image_processor="yolox-nano", detector_conf_threshold=1e-3,
                           max_batch=N)
    product.sync_weights()
    eng = product.engine()
    K, A = eng.cfg.max_det_per_patch, sum((P // s) ** 2 for s in (8, 16, 32))
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(3)).to(DEV)
    raw = torch.empty((N, A, 6), device=DEV)
    boxes = torch.full((N, K, 7), SENTINEL, device=DEV)
    counts = torch.full((N,), ISENT, device=DEV, dtype=torch.int32)
    check(eng.lib.jn_detect(eng.handle, ptr(x), N, ptr(boxes), ptr(counts), ptr(raw), _lib.current_stream(torch.device(DEV))),
          "jn_detect")
    torch.cuda.synchronize()
    assert abs(eng.cfg.det_conf_threshold - 1e-3) < 1e-9 and int(counts.min()) >= 1            # the stage had work to do
    b2, c2, s2 = _launch(raw.cpu().numpy(), eng.cfg.det_conf_threshold, eng.cfg.det_nms_threshold, P, K)
    assert torch.equal(c2[:N], counts.cpu())
    assert torch.equal(b2[:N * K].view(N, K, 7), boxes.cpu())                                    # sentinels included
    assert bool((s2[:N, 0] >= s2[:N, 1]).all()) and bool((s2[:N, 1] >= c2[:N]).all())
    score = (raw[..., 4] * raw[..., 5]).cpu()                      # one IEEE multiply: the first counter is exact on any input
    assert s2[:N, 0].tolist() == (score >= eng.cfg.det_conf_threshold).sum(1).tolist()


def test_entry_point_contract():
    lib = _lib.load_library()
    raw = torch.zeros((1, 84, 6), device=DEV)
    boxes = torch.full((4, 7), SENTINEL, device=DEV)
    counts = torch.full((1,), ISENT, device=DEV, dtype=torch.int32)

    def call(raw_=raw, N=1, A=84, max_out=4, boxes_=boxes, counts_=counts):
        return lib.jn_postprocess(ptr(raw_), N, A, C.c_float(0.25), C.c_float(0.45), C.c_float(63.0), max_out, ptr(boxes_),
                                  ptr(counts_), None, _lib.current_stream(torch.device(DEV)))
    assert call(raw_=None) == -1 and b"null" in lib.jn_last_error()
    assert call(boxes_=None) == -1 and call(counts_=None) == -1
    assert call(N=0) == -1 and call(A=0) == -1 and b"A=0" in lib.jn_last_error()
    assert call(max_out=0) == -1 and b"max_out" in lib.jn_last_error()
    torch.cuda.synchronize()
    assert bool((boxes == SENTINEL).all()) and int(counts) == ISENT                              # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((boxes == SENTINEL).all()) and int(counts) == 0
    with pytest.raises(_lib.JnError):
        yolox.postprocess(raw, 0.25, 0.45, 64, 0)
