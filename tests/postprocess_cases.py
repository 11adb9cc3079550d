"""Committed inputs for the detector's threshold / sort / NMS stage (`postprocess_kernel` through `jn_postprocess`) and
their exact reference.

Shared by the CPU test that shows the cases mean something (tests/test_postprocess_cases_cpu.py: the reference equals
the oracle, every case is admissible, every case reaches its branch) and the GPU test that holds the kernel to them
(tests/test_gpu_postprocess.py).  Nothing is drawn at test time: a case is (name, A, P, conf, nms, max_out, kind, args)
and `build(case)` is a pure function of it (seeded generators only).

Inputs.  raw [A, 6] fp32 = decoded rows (cx, cy, w, h, obj, cls) of ONE patch; a launch stacks patches.  Every anchor a
case does not set is background: a box somewhere in the patch with obj * cls <= 0.087, below every threshold used.

The reference (`reference(case)`) restates the stage in NumPy with every operation rounded to fp32 on its own:
x1 = cx - w * 0.5f ..., score = obj * cls, keep score >= fp32(conf), the first 2048 passing anchors in index order enter
the sort (DET_CAP), a stable order by (score descending, anchor index ascending), the greedy loop with the IoU formula
of oracle/yolox_ref.py::box_iou_xyxy suppressing on IoU > fp32(nms), the clamp to [0, P - 1] AFTER the loop, the first
max_out survivors written.  It returns the rows, the count and the two counters (passing anchors before the 2048 cap,
survivors before max_out).  It is exact, not within a bar: w * 0.5f is exact, so the edges are the same bits with or
without FMA contraction; the score is one IEEE multiply; the division is correctly rounded.  The only place the kernel
may differ is the last bits of the IoU denominator, where aa + dx * dy - inter may contract; hence

margins(case), fp64, over every pair the greedy loop actually compares (a kept box against a later, still live one;
pairs whose IoU is 0 / 0 = NaN, two zero-area boxes, compare false in any precision and are left out):
 (a) the smallest |iou64 - fp32(nms)|, iou64 computed in fp64 FROM THE fp32 EDGES, over the pairs whose fp64 and fp32
     IoU are not both exactly the threshold (integer boxes with IoU 1/2 against 0.5: every intermediate is an exact small
     integer in any contraction, the quotient exact);
 (b) the largest |iou32 - iou64|.
Admissible: (a) > MARGIN_BAR = 16 x the largest (b) over all cases (16 x: the allowance the SimOTA cases give fp32
conditioning; the contracted denominator is within a couple of ulp of the reference's).  Measured by
tests/test_postprocess_cases_cpu.py, which prints both: largest (b) = 1.64e-07 (MARGIN_BAR = 2.62e-06), smallest (a)
over all cases = 5.42e-05.  Random boxes are used up to 300 candidates only (seeds chosen so that the reference
alone is admissible); every larger case is built from integer-lattice boxes whose IoUs are 0, 1/2, 3/4 or 1.

Kinds (the cases and what each is for):
- empty: nothing passes; count 0, the output buffer untouched.
- last: the only candidate is anchor A - 1, A no multiple of 256.
- conf-exact: obj = cls = 0.5 against conf 0.25 is kept, score nextafter(0.25, 0) is dropped, nextafter(0.25, 1) kept;
  against conf 0.3 (not representable) score fp32(0.3) is kept and its predecessor dropped.
- clusters: k groups of m jittered copies of a box, at random anchors, random scores; 20 to 300 candidates; the P = 448
  version spreads them over the 17 chunks of 256 anchors.
- ties: two groups of nine anchors with bit-identical scores on overlapping boxes, one straddling anchor 64 (a wave
  boundary), one anchor 256 (a chunk boundary), among 40 other candidates; only the anchor index says who survives.  A
  third group: two anchors whose fp32 score products are equal while the fp64 products differ, the larger fp64 product
  at the HIGHER index.
- iou-exact: integer boxes with IoU exactly 1/2 (kept at 0.5, suppressed at 0.45), 3/4 (suppressed) and 1/4 (kept).
- chain: X suppresses Y; Y overlaps Z above the threshold, X does not; Z survives.
- degenerate: two identical zero-area boxes (IoU NaN, both kept), a zero-area box and a zero-height box inside a large
  box (IoU 0, kept).
- clamp: boxes over all four sides of [0, P - 1]; pairs with IoU 1/4 unclamped and 1 once clamped: both kept, both
  written clamped.
- max-out: 100 disjoint boxes with max_out 4 and 64.
- lattice: n candidates on a 64 x 32 lattice of disjoint 4 x 12 boxes in a 448 patch; with shadows, every third
  candidate is a box inside a lattice box with IoU 3/4 or 1/2.  n = 1, 2, 3, 255, 256, 257, 1023, 1025, 2047, 2048 (the
  sort's padding); n = 2049 and 3000 at A = 4116 (the candidate cap: the highest score of the patch sits on the last
  passing anchor and is dropped); 2048 without shadows (2048 greedy rounds).
- copies: 2048 copies of one box with distinct scores: one survives.
- negative: scores below zero against conf -1 (the entry takes any finite input): the sort's padding must rank below
  them.
"""
import functools
from typing import NamedTuple

import numpy as np

DET_CAP = 2048                   # candidates postprocess_kernel holds in LDS
MARGIN_BAR = 2.62e-06            # 16 x the largest |iou32 - iou64| over all cases (see the docstring)
F = np.float32


class Case(NamedTuple):
    name: str
    A: int
    P: int
    conf: float
    nms: float
    max_out: int
    kind: str
    args: tuple = ()


def _lattice_cases():
    out = []
    for n, A in ((1, 1), (2, 63), (3, 65), (255, 255), (256, 257), (257, 525), (1023, 4116), (1025, 4116), (2047, 4116),
                 (2048, 4116)):
        nms = 0.45 if n in (3, 256, 1025, 2048) else 0.5
        out.append(Case(f"count-{n}", A, 448, 0.25, nms, 2048, "lattice", (n, 1, n)))
    return out


CASES = [
    Case("empty-1", 1, 64, 0.25, 0.45, 100, "empty"),
    Case("empty-84", 84, 64, 0.25, 0.45, 100, "empty"),
    Case("empty-257", 257, 160, 0.3, 0.5, 100, "empty"),
    Case("last-63", 63, 64, 0.25, 0.45, 100, "last"),
    Case("last-65", 65, 64, 0.3, 0.5, 100, "last"),
    Case("last-257", 257, 160, 0.25, 0.45, 100, "last"),
    Case("last-525", 525, 160, 0.25, 0.5, 100, "last"),
    Case("last-4116", 4116, 448, 0.3, 0.45, 100, "last"),
    Case("conf-exact-0.25", 84, 64, 0.25, 0.45, 100, "conf-exact"),
    Case("conf-exact-0.3", 189, 96, 0.3, 0.5, 100, "conf-exact"),
    Case("clusters-84", 84, 64, 0.25, 0.45, 100, "clusters", (1, 2, 10)),
    Case("clusters-189", 189, 96, 0.3, 0.5, 100, "clusters", (1, 4, 15)),
    Case("clusters-255", 255, 160, 0.25, 0.45, 100, "clusters", (3, 5, 24)),
    Case("clusters-525", 525, 160, 0.25, 0.45, 100, "clusters", (1, 6, 50)),
    Case("clusters-4116", 4116, 448, 0.25, 0.45, 100, "clusters", (1, 8, 30)),
    Case("clusters-4116-0.5", 4116, 448, 0.3, 0.5, 100, "clusters", (2, 12, 16)),
    Case("ties-525", 525, 160, 0.25, 0.45, 100, "ties"),
    Case("ties-525-0.5", 525, 160, 0.3, 0.5, 100, "ties"),
    Case("iou-exact-0.5", 84, 64, 0.25, 0.5, 100, "iou-exact"),
    Case("iou-exact-0.45", 84, 64, 0.25, 0.45, 100, "iou-exact"),
    Case("chain-0.45", 65, 96, 0.25, 0.45, 100, "chain"),
    Case("chain-0.5", 189, 96, 0.3, 0.5, 100, "chain"),
    Case("degenerate", 84, 64, 0.25, 0.45, 100, "degenerate"),
    Case("clamp-0.45", 84, 64, 0.25, 0.45, 100, "clamp"),
    Case("clamp-0.5", 84, 64, 0.3, 0.5, 100, "clamp"),
    Case("max-out-4", 525, 160, 0.25, 0.45, 4, "max-out"),
    Case("max-out-64", 525, 160, 0.25, 0.45, 64, "max-out"),
    *_lattice_cases(),
    Case("cap-2049", 4116, 448, 0.25, 0.5, 2048, "lattice", (2049, 1, 2049)),
    Case("cap-3000", 4116, 448, 0.25, 0.45, 2048, "lattice", (3000, 1, 3000)),
    Case("heavy-disjoint", 4116, 448, 0.25, 0.45, 2048, "lattice", (2048, 0, 4)),
    Case("heavy-copies", 2048, 448, 0.25, 0.45, 100, "copies"),
    Case("negative-3", 3, 64, -1.0, 0.45, 100, "negative"),
    Case("negative-5", 5, 64, -1.0, 0.5, 100, "negative"),
]
BY_NAME = {c.name: c for c in CASES}
GUARD_ROWS = 8                   # rows behind the last patch's rows that a launch must leave untouched


# ---- builders ---------------------------------------------------------------------------------------------------------
def _background(A, P):
    a = np.arange(A)
    raw = np.zeros((A, 6), F)
    raw[:, 0] = (a * 37) % P
    raw[:, 1] = (a * 53) % P
    raw[:, 2] = raw[:, 3] = 10 + a % 7
    raw[:, 4] = F(0.2) + F(0.01) * (a % 10).astype(F)
    raw[:, 5] = F(0.3)
    return raw


def _put(raw, a, x1, y1, x2, y2, obj, cls):
    """Anchor a := the box with these edges (exact when the edges are integers or halves) and these two factors."""
    raw[a] = (F(0.5) * (F(x1) + F(x2)), F(0.5) * (F(y1) + F(y2)), F(x2) - F(x1), F(y2) - F(y1), F(obj), F(cls))


def _scores(rng, n, lo):
    """n distinct scores in (lo, 0.98) split into (obj, cls), both below 1: the order is a random permutation."""
    s = lo + 0.02 + (0.96 - lo) * (rng.permutation(n) + 1.0) / (n + 1.0)
    u = 0.2 + 0.6 * rng.random_sample(n)
    return (s ** u).astype(F), (s ** (1.0 - u)).astype(F)


def _lattice_box(cell):
    i, j = cell % 64, cell // 64
    return 7 * i + 1, 14 * j + 1, 7 * i + 5, 14 * j + 13


def _build_lattice(case):
    n, shadows, seed = case.args
    rng = np.random.RandomState(seed)
    raw = _background(case.A, case.P)
    n_sh = n // 3 if shadows else 0
    n_main = n - n_sh
    assert n_main <= 2048 and n <= case.A
    cells = rng.permutation(2048)[:n_main]
    where = np.sort(rng.permutation(case.A)[:n])
    slot = rng.permutation(n)                                      # candidate k sits on anchor where[slot[k]]
    obj, cls = _scores(rng, n, max(case.conf, 0.0))
    if n > DET_CAP:                                                # the best score of the patch on the last passing anchor
        k_last, k_best = int(np.argmax(slot)), int(np.argmax(obj * cls))
        obj[[k_last, k_best]], cls[[k_last, k_best]] = obj[[k_best, k_last]], cls[[k_best, k_last]]
    for k in range(n):
        if k < n_main:
            x1, y1, x2, y2 = _lattice_box(cells[k])
        else:                                                      # a shadow of main box k - n_main: IoU 3/4 or 1/2 with it
            x1, y1, x2, y2 = _lattice_box(cells[k - n_main])
            y2 = y1 + (9 if (k - n_main) % 2 == 0 else 6)
        _put(raw, where[slot[k]], x1, y1, x2, y2, obj[k], cls[k])
    return raw


def _build_clusters(case):
    seed, k, m = case.args
    rng = np.random.RandomState(1000 * seed + case.A)
    raw = _background(case.A, case.P)
    P = case.P
    where = rng.permutation(case.A)[:k * m]
    obj, cls = _scores(rng, k * m, case.conf)
    for g in range(k):
        w, h = rng.uniform(0.15 * P, 0.4 * P, 2)
        cx, cy = rng.uniform(0.2 * P, 0.8 * P, 2)
        for c in range(m):
            q = g * m + c
            jit = rng.normal(0.0, 0.04 * P, 4)
            raw[where[q]] = (cx + jit[0], cy + jit[1], max(w + jit[2], 1.0), max(h + jit[3], 1.0), obj[q], cls[q])
    return raw


def _equal_fp32_products():
    """(obj, cls), (obj', cls') with fp32(obj * cls) == fp32(obj' * cls') and obj * cls < obj' * cls' in fp64."""
    a, b = F(0.7), F(0.6)
    a2 = np.nextafter(a, F(1))
    b2 = b
    for _ in range(8):
        if F(a * b) == F(a2 * b2) and float(a) * float(b) != float(a2) * float(b2):
            lo, hi = sorted([(float(a) * float(b), a, b), (float(a2) * float(b2), a2, b2)])
            return (lo[1], lo[2]), (hi[1], hi[2])
        b2 = np.nextafter(b2, F(0))
    raise AssertionError("no pair found")


TIE_GROUPS = ((60, 9, 0.8, 0.7), (252, 9, 0.6, 0.9))             # first anchor, anchors, obj, cls


def _build_ties(case):
    rng = np.random.RandomState(7)
    raw = _background(case.A, case.P)
    # 40 disjoint others on a 16 px grid along the top rows, distinct scores around the tied ones
    obj, cls = _scores(rng, 40, case.conf)
    others = [a for a in rng.permutation(case.A) if not (56 <= a < 72 or 248 <= a < 264 or 400 <= a < 402)][:40]
    for q, a in enumerate(others):
        _put(raw, a, 16 * (q % 10) + 1, 16 * (q // 10) + 1, 16 * (q % 10) + 9, 16 * (q // 10) + 9, obj[q], cls[q])
    for g, (a0, cnt, o, c) in enumerate(TIE_GROUPS):               # nested boxes growing with the index: IoU >= 0.70
        for t in range(cnt):
            _put(raw, a0 + t, 10 + 70 * g, 80, 50 + 70 * g + t, 130 + t, o, c)
    (o1, c1), (o2, c2) = _equal_fp32_products()
    _put(raw, 400, 10, 140, 40, 158, o1, c1)
    _put(raw, 401, 10, 140, 41, 158, o2, c2)
    return raw


def _build(case):
    A, P = case.A, case.P
    raw = _background(A, P)
    kind = case.kind
    if kind == "empty":
        pass
    elif kind == "last":
        _put(raw, A - 1, 5, 6, 25, 30, 0.9, 0.8)
    elif kind == "conf-exact":
        if case.conf == 0.25:
            _put(raw, 10, 1, 1, 9, 9, 0.5, 0.5)
            _put(raw, 11, 11, 1, 19, 9, np.nextafter(F(0.25), F(0)), 1.0)
            _put(raw, 12, 21, 1, 29, 9, np.nextafter(F(0.25), F(1)), 1.0)
            _put(raw, 70, 31, 1, 39, 9, 0.5, np.nextafter(F(0.5), F(0)))
        else:
            _put(raw, 10, 1, 1, 9, 9, F(case.conf), 1.0)
            _put(raw, 11, 11, 1, 19, 9, np.nextafter(F(case.conf), F(0)), 1.0)
            _put(raw, 12, 21, 1, 29, 9, 1.0, np.nextafter(F(case.conf), F(1)))
    elif kind == "iou-exact":
        _put(raw, 3, 10, 10, 30, 20, 0.9, 0.9)                     # 1/2 with anchor 40
        _put(raw, 40, 10, 10, 20, 20, 0.9, 0.8)
        _put(raw, 5, 10, 30, 50, 40, 0.9, 0.7)                     # 3/4 with anchor 41
        _put(raw, 41, 10, 30, 40, 40, 0.9, 0.6)
        _put(raw, 83, 10, 50, 50, 60, 0.9, 0.5)                    # 1/4 with anchor 0
        _put(raw, 0, 10, 50, 20, 60, 0.9, 0.4)
    elif kind == "chain":
        _put(raw, 20, 10, 10, 50, 50, 0.9, 0.9)                    # X
        _put(raw, 7, 20, 10, 60, 50, 0.9, 0.8)                     # Y: IoU 0.6 with X
        _put(raw, 64, 30, 10, 70, 50, 0.9, 0.7)                    # Z: IoU 0.6 with Y, 1/3 with X
    elif kind == "degenerate":
        _put(raw, 8, 30, 30, 30, 30, 0.9, 0.9)                     # twice the same point
        _put(raw, 9, 30, 30, 30, 30, 0.9, 0.8)
        _put(raw, 50, 2, 2, 20, 20, 0.9, 0.7)                      # a large box, then a point and a line inside it
        _put(raw, 51, 10, 10, 10, 10, 0.9, 0.6)
        _put(raw, 52, 5, 12, 15, 12, 0.9, 0.5)
    elif kind == "clamp":
        m = P - 1
        _put(raw, 1, -10, 20, 15, 40, 0.9, 0.95)                   # over the left, right, top, bottom edge
        _put(raw, 2, m - 13, 20, m + 17, 40, 0.9, 0.94)
        _put(raw, 3, 20, -10, 40, 15, 0.9, 0.93)
        _put(raw, 4, 20, m - 13, 40, m + 17, 0.9, 0.92)
        _put(raw, 5, -30, 0, 10, 10, 0.9, 0.91)                    # IoU 1/4 with the next; both clamp to (0, 0, 10, 10)
        _put(raw, 6, 0, 0, 10, 10, 0.9, 0.90)
        _put(raw, 80, m - 10, m - 10, m + 30, m, 0.9, 0.89)        # the same at the right edge
        _put(raw, 81, m - 10, m - 10, m, m, 0.9, 0.88)
        _put(raw, 82, -5, -5, m + 5, m + 5, 0.9, 0.5)              # over all four; IoU with every box above is small
    elif kind == "max-out":
        rng = np.random.RandomState(5)
        obj, cls = _scores(rng, 100, case.conf)
        where = rng.permutation(A)[:100]
        for q in range(100):
            _put(raw, where[q], 16 * (q % 10) + 1, 16 * (q // 10) + 1, 16 * (q % 10) + 11, 16 * (q // 10) + 11, obj[q], cls[q])
    elif kind == "copies":
        obj, cls = _scores(np.random.RandomState(6), A, case.conf)
        for a in range(A):
            _put(raw, a, 100, 120, 180, 240, obj[a], cls[a])
    elif kind == "negative":
        _put(raw, 0, 1, 1, 9, 9, -0.5, 0.5)
        _put(raw, 1, 11, 1, 19, 9, 0.5, -0.2)
        _put(raw, 2, 21, 1, 29, 9, 0.5, 0.4)
        for a in range(3, A):
            _put(raw, a, 1, 11 + 10 * (a - 3), 9, 19 + 10 * (a - 3), -0.3 - 0.1 * a, 0.9)
    else:
        raise KeyError(kind)
    return raw


@functools.lru_cache(maxsize=None)
def _build_cached(case):
    raw = {"lattice": _build_lattice, "clusters": _build_clusters, "ties": _build_ties}.get(case.kind, _build)(case)
    assert raw.dtype == F and raw.shape == (case.A, 6) and bool(np.isfinite(raw).all()) and bool((raw[:, 2:4] >= 0).all())
    raw.setflags(write=False)
    return raw


def build(case):
    """raw [A, 6] fp32 of the case's patch (read-only, shared)."""
    return _build_cached(case)


# ---- the reference ----------------------------------------------------------------------------------------------------
def xyxy(raw):
    half = F(0.5)
    return np.stack((raw[:, 0] - raw[:, 2] * half, raw[:, 1] - raw[:, 3] * half, raw[:, 0] + raw[:, 2] * half,
                     raw[:, 1] + raw[:, 3] * half), 1)


def _iou_row(b, i, js, dtype):
    """IoU of box i against boxes js, every operation in `dtype` (box_iou_xyxy's formula)."""
    b = b.astype(dtype)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    zero = dtype(0)
    iw = np.maximum(np.minimum(b[i, 2], b[js, 2]) - np.maximum(b[i, 0], b[js, 0]), zero)
    ih = np.maximum(np.minimum(b[i, 3], b[js, 3]) - np.maximum(b[i, 1], b[js, 1]), zero)
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[i] + area[js] - inter)


def run(raw, conf, nms, P, max_out, *, conf_strict=False, iou_ge=False, tie_high_index=False, dead_suppress=False,
        clamp_first=False, trace=None):
    """The stage on one patch.  Returns (rows [count, 7] fp32, count, (passing, survivors)).  The keyword flags switch on
    one deliberate mistake each; the CPU test uses them to show that a case reaches its branch.  `trace`, a list, receives
    (iou32, iou64) of every pair the greedy loop compares."""
    raw = np.asarray(raw, F)
    conf, nms, hi = F(conf), F(nms), F(P - 1)
    score = raw[:, 4] * raw[:, 5]
    passing = np.nonzero(score > conf if conf_strict else score >= conf)[0]
    cand = passing[:DET_CAP]
    order = cand[np.lexsort((-cand if tie_high_index else cand, -score[cand]))]
    edges = xyxy(raw)
    clamped = np.minimum(np.maximum(edges, F(0)), hi)
    b = (clamped if clamp_first else edges)[order]
    n = len(order)
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i] and not dead_suppress:
            continue
        if not dead[i]:
            keep.append(i)
        js = np.arange(i + 1, n)
        js = js[~dead[js]]
        if len(js) == 0:
            continue
        iou = _iou_row(b, i, js, F)
        if trace is not None:
            trace.append((iou, _iou_row(b, i, js, np.float64)))
        dead[js[iou >= nms if iou_ge else iou > nms]] = True
    kept = order[keep[:max_out]]
    rows = np.concatenate((clamped[kept], raw[kept, 4:6], np.zeros((len(kept), 1), F)), 1).astype(F)
    return rows, len(kept), (len(passing), len(keep))


@functools.lru_cache(maxsize=None)
def reference(case):
    rows, count, stats = run(build(case), case.conf, case.nms, case.P, case.max_out)
    rows.setflags(write=False)
    return rows, count, stats


@functools.lru_cache(maxsize=None)
def margins(case):
    """{"a": smallest |iou64 - fp32(nms)| off the exact ties, "b": largest |iou32 - iou64|, "exact": pairs whose fp32 and
    fp64 IoU both equal the threshold, "nan": pairs with a NaN IoU, "pairs": compared pairs}."""
    trace = []
    run(build(case), case.conf, case.nms, case.P, case.max_out, trace=trace)
    thr = float(F(case.nms))
    out = dict(a=float("inf"), b=0.0, exact=0, nan=0, pairs=0)
    for i32, i64 in trace:
        nan = np.isnan(i64)
        assert bool((np.isnan(i32) == nan).all())
        i32, i64 = i32[~nan].astype(np.float64), i64[~nan]
        exact = (i32 == thr) & (i64 == thr)
        out["nan"] += int(nan.sum())
        out["exact"] += int(exact.sum())
        out["pairs"] += len(nan)
        if len(i64):
            out["b"] = max(out["b"], float(np.abs(i32 - i64).max()))
        if (~exact).any():
            out["a"] = min(out["a"], float(np.abs(i64[~exact] - thr).min()))
    return out


# ---- launches: patches of one (conf, nms, max_out), padded with background to a common A ------------------------------
def launches(max_patches=7):
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
        raw[n] = _background(A, c.P)
        raw[n, :c.A] = build(c)
    return raw
