"""Committed inputs for the detector's threshold / sort / NMS stage under the candidate policy "all"
(`postprocess_all_kernel` through `jn_postprocess_all`) and their exact reference.

Shared by the CPU test that shows the cases mean something (tests/test_postprocess_all_cases_cpu.py) and the GPU test that
holds the kernel to them (tests/test_gpu_postprocess_all.py).  Builders, the Case tuple and the fp32 IoU are those of
tests/postprocess_cases.py (`pc`); nothing is drawn at test time.

The reference (`run_all`) is `pc.run` with one line changed: the candidate set is EVERY passing anchor, not the first
2048.  That is oracle/yolox_ref.py::postprocess (which has no candidate cap) + the clamp + the cut to max_out rows, and the
CPU test holds it to that bit for bit without doctoring an input.

Every box here sits on an integer lattice, so each IoU the greedy loop compares is exactly 0, 1/2, 3/4 or 1 in fp32 and
in fp64 (margin (b) = 0), and the thresholds 0.45 / 0.5 stand 0.05 or more away from every one of them that is not
exactly on 0.5 (margin (a) >= 0.05 > pc.MARGIN_BAR).  The lattice: 4 x 8 boxes at pitch 5 x 9, (P // 5) x (P // 9) disjoint
cells (640 px: 128 x 71 = 9088; 448 px: 89 x 49 = 4361).  With shadows every third candidate is a box inside a lattice
box, of height 6 (IoU 3/4) or 4 (IoU 1/2).  The last column of the 640 px lattice ends at x = 640 and is clamped to 639.

Kinds:
- lattice (n, shadows, seed): n candidates at random anchors; for n > 2048 the patch's best score sits on the LAST passing
  anchor, which the first-2048 policy never sees.  n = 2049, 3000, 4095, 4096, 4097, 4116 at A = 4116 and 8191, 8192,
  8193, 8400 at A = 8400 (around the sort's powers of two; every anchor passing); 300 and 2100 at A = 2541 so that a
  launch mixes patch sizes; all-disjoint-8400 (no shadows: 8400 greedy rounds, 8400 rows written); max-out-64 (3000
  candidates, 64 rows written, the survivors before the cut counted).
- copies: 8400 copies of one box with distinct scores: one survives, the last anchor.
- ties-far: three pairs of a box and its 3/4 shadow with bit-identical scores on anchors (2047, 2048), (4095, 4096),
  (8191, 8192), among 3000 disjoint others: only the anchor index says which of a pair survives.
- negative: 8400 disjoint boxes, every score in (-0.98, -0.02), conf = -1: anything the sort pads with must rank below.
- empty, last: nothing passes; only anchor 8399 passes.
"""
import functools

import numpy as np

from tests import postprocess_cases as pc
from tests.postprocess_cases import Case, F

POST_ALL_MAX_A = 8400            # anchors postprocess_all_kernel holds in LDS (640 px at strides 8 / 16 / 32)
TIE_PAIRS = ((2047, 0.8, 0.7), (4095, 0.6, 0.9), (8191, 0.5, 0.9))       # first anchor of the pair, obj, cls
GUARD_ROWS = pc.GUARD_ROWS

K = POST_ALL_MAX_A
CASES = [
    Case("count-2049", 4116, 448, 0.25, 0.5, K, "lattice", (2049, 1, 2049)),
    Case("count-3000", 4116, 448, 0.25, 0.45, K, "lattice", (3000, 1, 3000)),
    Case("count-4095", 4116, 448, 0.25, 0.5, K, "lattice", (4095, 1, 4095)),
    Case("count-4096", 4116, 448, 0.25, 0.45, K, "lattice", (4096, 1, 4096)),
    Case("count-4097", 4116, 448, 0.25, 0.5, K, "lattice", (4097, 1, 4097)),
    Case("count-4116", 4116, 448, 0.25, 0.45, K, "lattice", (4116, 1, 4116)),
    Case("count-8191", 8400, 640, 0.25, 0.5, K, "lattice", (8191, 1, 8191)),
    Case("count-8192", 8400, 640, 0.25, 0.45, K, "lattice", (8192, 1, 8192)),
    Case("count-8193", 8400, 640, 0.25, 0.5, K, "lattice", (8193, 1, 8193)),
    Case("count-8400", 8400, 640, 0.25, 0.45, K, "lattice", (8400, 1, 8400)),
    Case("mixed-300", 2541, 640, 0.25, 0.45, K, "lattice", (300, 1, 300)),
    Case("mixed-2100", 2541, 640, 0.25, 0.5, K, "lattice", (2100, 1, 2100)),
    Case("all-disjoint-8400", 8400, 640, 0.25, 0.45, K, "lattice", (8400, 0, 4)),
    Case("all-copies-8400", 8400, 640, 0.25, 0.45, 100, "copies"),
    Case("ties-far", 8400, 640, 0.25, 0.45, K, "ties-far"),
    Case("negative-8400", 8400, 640, -1.0, 0.45, K, "negative"),
    Case("max-out-64", 4116, 448, 0.25, 0.45, 64, "lattice", (3000, 1, 64)),
    Case("empty-8400", 8400, 640, 0.25, 0.45, 100, "empty"),
    Case("last-8400", 8400, 640, 0.25, 0.45, 100, "last"),
]
BY_NAME = {c.name: c for c in CASES}


# ---- builders ---------------------------------------------------------------------------------------------------------
def n_cells(P):
    return (P // 5) * (P // 9)


def _cell_box(cell, P):
    i, j = cell % (P // 5), cell // (P // 5)
    return 5 * i + 1, 9 * j + 1, 5 * i + 5, 9 * j + 9


def _build_lattice(case):
    n, shadows, seed = case.args
    rng = np.random.RandomState(seed)
    raw = pc._background(case.A, case.P)
    n_sh = n // 3 if shadows else 0
    n_main = n - n_sh
    assert n_main <= n_cells(case.P) and n <= case.A <= POST_ALL_MAX_A
    cells = rng.permutation(n_cells(case.P))[:n_main]
    where = np.sort(rng.permutation(case.A)[:n])
    slot = rng.permutation(n)                                      # candidate k sits on anchor where[slot[k]]
    obj, cls = pc._scores(rng, n, case.conf)
    if n > pc.DET_CAP:                                             # the best score of the patch on the last passing anchor
        k_last, k_best = int(np.argmax(slot)), int(np.argmax(obj * cls))
        obj[[k_last, k_best]], cls[[k_last, k_best]] = obj[[k_best, k_last]], cls[[k_best, k_last]]
    for k in range(n):
        x1, y1, x2, y2 = _cell_box(cells[k if k < n_main else k - n_main], case.P)
        if k >= n_main:                                            # a shadow of main box k - n_main: IoU 3/4 or 1/2 with it
            y2 = y1 + (6 if (k - n_main) % 2 == 0 else 4)
        pc._put(raw, where[slot[k]], x1, y1, x2, y2, obj[k], cls[k])
    return raw


def _build_ties(case):
    rng = np.random.RandomState(11)
    raw = pc._background(case.A, case.P)
    taken = {a for a0, _, _ in TIE_PAIRS for a in (a0, a0 + 1)}
    others = [a for a in rng.permutation(case.A) if a not in taken][:3000]
    cells = rng.permutation(n_cells(case.P))
    obj, cls = pc._scores(rng, 3000, case.conf)
    for q, a in enumerate(others):
        pc._put(raw, a, *_cell_box(cells[q], case.P), obj[q], cls[q])
    for g, (a0, o, c) in enumerate(TIE_PAIRS):
        x1, y1, x2, y2 = _cell_box(cells[3000 + g], case.P)
        pc._put(raw, a0, x1, y1, x2, y2, o, c)
        pc._put(raw, a0 + 1, x1, y1, x2, y1 + 6, o, c)             # the 3/4 shadow, same score bits, the higher index
    return raw


def _build(case):
    A, P = case.A, case.P
    raw = pc._background(A, P)
    if case.kind == "empty":
        pass
    elif case.kind == "last":
        pc._put(raw, A - 1, 5, 6, 25, 30, 0.9, 0.8)
    elif case.kind == "copies":
        obj, cls = pc._scores(np.random.RandomState(6), A, case.conf)
        best = int(np.argmax(obj * cls))                           # the survivor is the last anchor
        obj[[A - 1, best]], cls[[A - 1, best]] = obj[[best, A - 1]], cls[[best, A - 1]]
        for a in range(A):
            pc._put(raw, a, 100, 120, 180, 240, obj[a], cls[a])
    elif case.kind == "negative":                                  # with conf = -1 the background would pass: every anchor is set
        rng = np.random.RandomState(8)
        cells = rng.permutation(n_cells(P))
        obj, cls = pc._scores(rng, A, 0.0)
        for a in range(A):
            pc._put(raw, a, *_cell_box(cells[a], P), -obj[a], cls[a])
    else:
        raise KeyError(case.kind)
    return raw


@functools.lru_cache(maxsize=None)
def build(case):
    """raw [A, 6] fp32 of the case's patch (read-only, shared)."""
    raw = {"lattice": _build_lattice, "ties-far": _build_ties}.get(case.kind, _build)(case)
    assert raw.dtype == F and raw.shape == (case.A, 6) and bool(np.isfinite(raw).all()) and bool((raw[:, 2:4] >= 0).all())
    raw.setflags(write=False)
    return raw


# ---- the reference ----------------------------------------------------------------------------------------------------
def run_all(raw, conf, nms, P, max_out, *, tie_high_index=False, acc=None):
    """pc.run with the candidate set = every passing anchor.  Returns (rows [count, 7] fp32, count, (passing, survivors)).
    `tie_high_index` is the one deliberate mistake the ties need.  `acc`, a dict, accumulates pc.margins' figures over
    every pair the greedy loop compares (a, b, exact, nan, pairs)."""
    raw = np.asarray(raw, F)
    conf, nms, hi = F(conf), F(nms), F(P - 1)
    thr = float(nms)
    score = raw[:, 4] * raw[:, 5]
    passing = np.nonzero(score >= conf)[0]
    cand = passing
    order = cand[np.lexsort((-cand if tie_high_index else cand, -score[cand]))]
    edges = pc.xyxy(raw)
    clamped = np.minimum(np.maximum(edges, F(0)), hi)
    b = edges[order]
    n = len(order)
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        js = np.arange(i + 1, n)
        js = js[~dead[js]]
        if len(js) == 0:
            continue
        iou = pc._iou_row(b, i, js, F)
        if acc is not None:
            i64 = pc._iou_row(b, i, js, np.float64)
            nan = np.isnan(i64)
            assert bool((np.isnan(iou) == nan).all())
            i32 = iou[~nan].astype(np.float64)
            i64 = i64[~nan]
            exact = (i32 == thr) & (i64 == thr)
            acc["nan"] += int(nan.sum())
            acc["exact"] += int(exact.sum())
            acc["pairs"] += len(nan)
            acc["values"] |= set(np.unique(i64).tolist())
            if len(i64):
                acc["b"] = max(acc["b"], float(np.abs(i32 - i64).max()))
            if (~exact).any():
                acc["a"] = min(acc["a"], float(np.abs(i64[~exact] - thr).min()))
        dead[js[iou > nms]] = True
    kept = order[keep[:max_out]]
    rows = np.concatenate((clamped[kept], raw[kept, 4:6], np.zeros((len(kept), 1), F)), 1).astype(F)
    return rows, len(kept), (len(passing), len(keep))


_REFERENCE = {}


def reference(case):
    """(rows, count, (passing, survivors)) of the case under the policy "all"; computed once (about 2.4 s for a case of
    8400 greedy rounds), by margins(case) if that ran first."""
    if case not in _REFERENCE:
        rows, count, stats = run_all(build(case), case.conf, case.nms, case.P, case.max_out)
        rows.setflags(write=False)
        _REFERENCE[case] = (rows, count, stats)
    return _REFERENCE[case]


@functools.lru_cache(maxsize=None)
def margins(case):
    """pc.margins over the uncapped run, plus "values": the set of fp64 IoUs compared.  The same run is the reference."""
    acc = dict(a=float("inf"), b=0.0, exact=0, nan=0, pairs=0, values=set())
    rows, count, stats = run_all(build(case), case.conf, case.nms, case.P, case.max_out, acc=acc)
    rows.setflags(write=False)
    _REFERENCE.setdefault(case, (rows, count, stats))
    return acc


# ---- launches: patches of one (conf, nms, P, max_out), padded with background to a common A ---------------------------
def launches(max_patches=4):
    """[(conf, nms, P, max_out, [case, ...])]: every case once, grouped by its thresholds, at most `max_patches` to a
    launch.  stack() pads the patches of a launch to the largest A with anchors that do not pass."""
    groups = {}
    for c in CASES:
        groups.setdefault((c.conf, c.nms, c.P, c.max_out), []).append(c)
    out = []
    for key, cs in groups.items():
        for i in range(0, len(cs), max_patches):
            out.append((*key, cs[i:i + max_patches]))
    return out


def stack(cases):
    A = max(c.A for c in cases)
    raw = np.zeros((len(cases), A, 6), F)
    for n, c in enumerate(cases):
        raw[n] = pc._background(A, c.P)
        raw[n, :c.A] = build(c)
    return raw
