"""Committed inputs for the SimOTA detector loss (`yolox_loss_kernel` through `jn_yolox_loss`) and their fp64 oracle.

Shared by the CPU test that shows the cases mean something (tests/test_simota_cases_cpu.py: every case is admissible,
the list walks every branch of the assignment, an fp32 evaluation assigns as fp64 does) and the GPU test that holds the
kernel to them (tests/test_gpu_simota_loss.py).  Nothing is drawn at test time: a case is (P, N, nb, seed, layout, use_l1)
and `build(case)` is a pure function of it.

Inputs.  raw [N, A, 6] fp32: objectness and class logits N(0, 2) clipped to |o| <= 8 (sigmoid(o) - 1 is never 0 in fp32,
so the foreground set is the sign of d_raw[..., 4]); regression outputs N(0, 0.5), except at the anchors within 1.5
strides of a real box's centre, which encode a copy of that box jittered by sigma = 0.25 in raw units: that puts the
top-10 IoU sums at 3 to 8, where dynamic k and contention exist.  targets [N, nb, 5] fp32 = (class, x1, y1, x2, y2), the
public layout; the fp64 oracle converts them to cxcywh as the kernel's conversion does.

Layouts, one per patch; a case's layout is a "+"-joined cycle over its patches ("clustered+empty": patch 0 clustered,
patch 1 empty, patch 2 clustered ...).  Patch 0 holds nb real boxes, a later patch 1..nb of them:
- clustered: centres within 40 px of each other, the boxes contend for anchors;
- spread: centres anywhere in the patch;
- stray: as spread, but no anchor predicts the boxes (an untrained head): top-10 IoU sums below 1, k = 1 by the clamp;
- corner: centres within 8 px (one stride) of a patch corner: 12 candidates per box;
- empty: zero rows only;
- outside: one box whose centre lies 60 px or more beyond the right or bottom edge: ng > 0 with zero candidates;
- zero-row-first: a zero row, then a real box: the published head takes the FIRST ng rows, here the zero row.

margins(case), fp64: the distance of every discrete decision of the assignment from flipping,
 (a) smallest |centre-radius delta| over box x anchor, px.  The all-zero box of zero-row-first is left out: its deltas
     are differences of integers below 2^8 (0 +- 1.5 * stride against anchor centres), exact in fp32 and fp64 alike, zeros
     included;
 (b) smallest |top-10 IoU sum - nearest integer| over the boxes.  A sum of exact zeros is left out: every IoU of a box
     disjoint from all its candidates (the zero row of zero-row-first) is +0 in any precision (`en` = 0), int(0) = 0;
 (c) smallest gap between the k-th and (k+1)-th cheapest cost of a box, relative to max(1, |cost|);
 (d) the same gap between the two cheapest boxes of every contested anchor;
 (e) smallest |p - q| over the max / min operand pairs of the IoU loss at foreground anchors, px.
Admissible: (a) > 1e-3, (b) > 1e-2, (c), (d) > 1e-3, (e) > 1e-4.  Costs are fp32 sums of two logs of magnitude 1 to 60
computed with accurate logf / expf, error about 1e-5: the gaps sit ten to a hundred times above it.  TIE_CASE is exempt
from (e) and has (e) = 0: a stride-8 anchor with raw (0.5, 0.5, 0, 0) decodes to an exact 8 x 8 box whose left and top
edges equal those of its ground-truth box bit for bit, so torch's max / min backward splits the gradient 0.5 / 0.5.

"k clamped to nc" cannot be reached with finite inputs: the sum of min(10, nc) IoUs, each < 1 unless a prediction equals
its box exactly, truncates to at most nc - 1, and clamp(min=1) gives 1 <= nc.  No case covers it.

Tolerances.  Each bar is 8 x the worst distance from fp64 of the fp32 CPU evaluation of the same oracle over CASES +
[TIE_CASE] (8 x: the factor test_detector_training_step_vs_oracle grants over fp32 conditioning; the kernel's float
atomics sum in another order than torch).  Measured by tests/test_simota_cases_cpu.py (single-threaded torch), which
prints them; never derived from the kernel's output.  Measured fp32 distances:
- the five losses (total, 5 * iou, obj, cls, l1), relative: 1.19e-7, 8.64e-7, 1.57e-7, 4.73e-7, 7.91e-8;
- scale, relative: 3.73e-8;
- LOSS_SCALE * d total / d raw per column, max-norm over max |ref|: 6.27e-6, 3.46e-6, 6.89e-6, 8.90e-6, 4.28e-7, 4.73e-6 (the
  regression columns carry the IoU gradient, a quotient of differences of box edges: fp32 itself is good to 1e-5 there);
- the same gradient over the foreground rows of columns 0-3 and 5, relative L2: 2.63e-6.
All bars are far below 1e-4 relative: the inputs are well conditioned.
"""
import functools
from typing import NamedTuple

import torch

from oracle import yolox_ref

STRIDES = (8, 16, 32)
LOSS_SCALE = 0.5                 # the 1 / gradient_accumulation of the training step


class Case(NamedTuple):
    P: int
    N: int
    nb: int
    seed: int
    layout: str
    use_l1: bool = True


# ---- the fixed bars: 8 x the fp32 CPU oracle's distance from fp64 (see the docstring) ---------------------------------
METRIC_RTOL = (9.5e-7, 6.9e-6, 1.25e-6, 3.8e-6, 6.3e-7)      # total, 5 * iou, obj, cls, l1: |got - ref| / |ref|
SCALE_RTOL = 3.0e-7
GRAD_MAX = (5.0e-5, 2.8e-5, 5.5e-5, 7.1e-5, 3.4e-6, 3.8e-5)    # per column of d total / d raw: max |got - ref| / max |ref|
GRAD_FG_L2 = 2.1e-5                           # relative L2 over the foreground rows of columns 0-3 and 5

CASES = [
    Case(64, 1, 1, 1, "spread", False),
    Case(64, 1, 2, 1, "clustered"),
    Case(64, 3, 1, 1, "corner+spread+empty", False),
    Case(64, 2, 8, 20, "clustered"),
    Case(64, 2, 1, 1, "empty", False),
    Case(64, 2, 2, 8, "stray"),
    Case(160, 1, 8, 2, "spread"),
    Case(160, 4, 5, 1, "clustered+empty", False),
    Case(160, 2, 2, 1, "zero-row-first+outside"),
    Case(160, 3, 3, 1, "empty"),
    Case(160, 2, 4, 1, "outside+corner", False),
    Case(160, 3, 8, 11, "clustered", False),
    Case(160, 5, 8, 1, "clustered"),
    Case(160, 3, 3, 9, "stray+clustered", False),
    Case(448, 1, 8, 1, "spread", False),
    Case(448, 8, 8, 1, "spread+clustered+empty", False),
    Case(448, 2, 3, 1, "spread"),
    Case(448, 3, 6, 6, "clustered+corner+zero-row-first"),
    Case(448, 2, 8, 12, "clustered+spread"),
    Case(448, 1, 4, 7, "stray"),
]
TIE_CASE = Case(64, 1, 1, 0, "tie")
BOX_CAP_CASE = Case(160, 2, 12, 0, "eleven")       # eleven real boxes in patch 0: beyond the kernel's 8


def geometry(P, dtype=torch.float64):
    """(grid [A, 2] (x, y) cell of every anchor, stride [A], hw of the three levels), level by level, row-major."""
    grids, sv, hw = [], [], []
    for s in STRIDES:
        h = w = P // s
        yv, xv = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grids.append(torch.stack((xv, yv), 2).view(-1, 2))
        sv.append(torch.full((h * w,), float(s)))
        hw.append((h, w))
    return torch.cat(grids).to(dtype), torch.cat(sv).to(dtype), hw


def n_anchors(P):
    return sum((P // s) ** 2 for s in STRIDES)


def to_cxcywh(targets):
    """(class, x1, y1, x2, y2) -> (class, cx, cy, w, h) with the kernel's expressions, in the dtype of `targets`."""
    t = targets
    return torch.stack([t[..., 0], 0.5 * (t[..., 1] + t[..., 3]), 0.5 * (t[..., 2] + t[..., 4]), t[..., 3] - t[..., 1],
                        t[..., 4] - t[..., 2]], -1)


def _patch_boxes(layout, P, nb, first, g):
    """cxcywh boxes [n, 4] fp64 of one patch and the row each goes to."""
    def rand(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)
    if layout == "empty":
        return torch.zeros((0, 4), dtype=torch.float64), []
    if layout == "outside":                       # beyond the right or the bottom edge: the row's sum stays positive
        far, along = 60.0 + 40.0 * float(rand(1)), float(rand(1)) * P
        c = (P + far, along) if int(torch.randint(0, 2, (1,), generator=g)) else (along, P + far)
        wh = rand(2) * 16 + 8
        return torch.tensor([[c[0], c[1], float(wh[0]), float(wh[1])]], dtype=torch.float64), [0]
    if layout == "zero-row-first":
        assert nb >= 2
        cxy = rand(1, 2) * (P - 16) + 8
        wh = rand(1, 2) * (P / 2 - 8) + 8
        return torch.cat([cxy, wh], 1), [1]
    n = nb if first else int(torch.randint(1, nb + 1, (1,), generator=g))
    if layout in ("clustered", "eleven"):
        c0 = rand(2) * (P - 64) + 32
        cxy = c0 + (rand(n, 2) - 0.5) * 40
    elif layout in ("spread", "stray"):
        cxy = rand(n, 2) * (P - 16) + 8
    elif layout == "corner":
        corner = torch.randint(0, 2, (n, 2), generator=g).double()
        off = rand(n, 2) * 8
        cxy = corner * P + (1 - 2 * corner) * off
    else:
        raise ValueError(layout)
    wh = rand(n, 2) * (P / 2 - 8) + 8
    return torch.cat([cxy, wh], 1), list(range(n))


@functools.lru_cache(maxsize=None)
def build(case):
    """(raw [N, A, 6] fp32, targets [N, nb, 5] fp32 xyxy) of a case.  Treat both as read-only."""
    if case.layout == "tie":
        return _build_tie(case)
    P, N, nb = case.P, case.N, case.nb
    grid, stride, _ = geometry(P)
    A = grid.shape[0]
    xc, yc = (grid[:, 0] + 0.5) * stride, (grid[:, 1] + 0.5) * stride
    layouts = case.layout.split("+")
    raws, tgs = [], []
    for n in range(N):
        g = torch.Generator().manual_seed(case.seed * 1000 + n)
        lay = layouts[n % len(layouts)]
        n_real = 11 if lay == "eleven" else nb
        boxes, rows = _patch_boxes(lay, P, n_real, n == 0, g)
        tg = torch.zeros((nb, 5), dtype=torch.float64)
        for b, r in zip(boxes, rows):
            tg[r, 1:] = torch.stack([b[0] - b[2] / 2, b[1] - b[3] / 2, b[0] + b[2] / 2, b[1] + b[3] / 2])
        tg = tg.float()
        gt = to_cxcywh(tg.double())[:, 1:]                          # the boxes as the kernel will see them
        raw = torch.randn((A, 6), generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.5, 0.5, 0.5, 2.0, 2.0], dtype=torch.float64)
        raw[:, 4:].clamp_(-8.0, 8.0)
        for r in rows if lay != "stray" else []:                    # anchors near a real box predict a jittered copy of it
            near = ((xc - gt[r, 0]).abs() < 1.5 * stride) & ((yc - gt[r, 1]).abs() < 1.5 * stride)
            idx = near.nonzero().squeeze(1)
            j = torch.randn((len(idx), 4), generator=g, dtype=torch.float64) * 0.25
            raw[idx, 0] = gt[r, 0] / stride[idx] - grid[idx, 0] + j[:, 0]
            raw[idx, 1] = gt[r, 1] / stride[idx] - grid[idx, 1] + j[:, 1]
            raw[idx, 2] = torch.log(gt[r, 2] / stride[idx]) + j[:, 2]
            raw[idx, 3] = torch.log(gt[r, 3] / stride[idx]) + j[:, 3]
        raws.append(raw.float())
        tgs.append(tg)
    return torch.stack(raws), torch.stack(tgs)


def _build_tie(case):
    P = case.P
    grid, stride, _ = geometry(P)
    A = grid.shape[0]
    g = torch.Generator().manual_seed(77)
    raw = torch.randn((A, 6), generator=g, dtype=torch.float64) * 0.5
    raw[:, 4:] = -4.0 + 0.25 * torch.randn((A, 2), generator=g, dtype=torch.float64)
    gx, gy = 3, 2
    a = gy * (P // 8) + gx                                          # a stride-8 anchor: decodes to [24, 32] x [16, 24] exactly
    raw[a] = torch.tensor([0.5, 0.5, 0.0, 0.0, 8.0, 8.0], dtype=torch.float64)
    tg = torch.zeros((1, case.nb, 5))
    tg[0, 0] = torch.tensor([0.0, 8.0 * gx, 8.0 * gy, 8.0 * gx + 13.0, 8.0 * gy + 11.0])   # same left and top edge
    return raw.float()[None], tg


def _trace_patch(gt, raw, grid, stride):
    """The fp64 assignment of one patch, restated step by step so that every decision's margin can be read off.
    gt [ng, 4] cxcywh (the first ng rows), raw [A, 6]."""
    inf = float("inf")
    ng, A = gt.shape[0], raw.shape[0]
    out = dict(ng=ng, nc=0, ks=[], sums=[], a=inf, b=inf, c=inf, d=inf, e=inf, contested=0, contested_not_first=0,
               boxes_left_empty=0, chunks=0, levels=0, nfg=0, fg=torch.zeros(A, dtype=torch.bool))
    if ng == 0:
        return out
    boxes = torch.cat([(raw[:, :2] + grid) * stride[:, None], torch.exp(raw[:, 2:4]) * stride[:, None]], 1)
    xc, yc, r = (grid[:, 0] + 0.5) * stride, (grid[:, 1] + 0.5) * stride, 1.5 * stride
    d = torch.stack([xc[None] - (gt[:, 0:1] - r[None]), yc[None] - (gt[:, 1:2] - r[None]),
                     (gt[:, 0:1] + r[None]) - xc[None], (gt[:, 1:2] + r[None]) - yc[None]], 2).min(-1).values
    real = gt.abs().sum(1) != 0                                     # (the zero box: small integers, exact in any precision)
    if real.any():
        out["a"] = d[real].abs().min().item()
    inc = d > 0
    cand = inc.sum(0) > 0
    nc = out["nc"] = int(cand.sum())
    if nc == 0:
        return out
    cidx = cand.nonzero().squeeze(1)
    out["chunks"] = len(set((cidx // 256).tolist()))
    out["levels"] = len(set(stride[cidx].tolist()))
    ious = yolox_ref.pairwise_iou_cxcywh(gt, boxes[cand])
    p = (raw[cand, 5].sigmoid() * raw[cand, 4].sigmoid()).sqrt()
    cost = (-torch.log(p)).clamp(max=100.0)[None] + 3.0 * -torch.log(ious + 1e-8) + 1e6 * (~inc[:, cand]).double()
    sums = torch.topk(ious, min(10, nc), dim=1).values.sum(1)
    ks = sums.int().clamp(min=1)
    out["sums"], out["ks"] = sums.tolist(), ks.tolist()
    live = sums[sums != 0.0]
    if len(live):
        out["b"] = (live - live.round()).abs().min().item()
    match = torch.zeros_like(cost, dtype=torch.bool)
    for gi in range(ng):
        v, i = torch.sort(cost[gi])
        k = int(ks[gi])
        if k < nc:
            out["c"] = min(out["c"], ((v[k] - v[k - 1]) / v[k - 1].abs().clamp(min=1)).item())
        match[gi, i[:k]] = True
    claims = match.sum(0)
    multi = claims > 1
    out["contested"] = int(multi.sum())
    final = match.clone()
    if multi.any():
        v, i = torch.sort(cost[:, multi], dim=0)
        out["d"] = ((v[1] - v[0]) / v[0].abs().clamp(min=1)).min().item()
        first = match[:, multi].int().argmax(0)
        out["contested_not_first"] = int((i[0] != first).sum())
        final[:, multi] = False
        final[i[0], multi.nonzero().squeeze(1)] = True
    out["boxes_left_empty"] = int((final.sum(1) == 0).sum())
    sel = claims > 0
    out["nfg"] = int(sel.sum())
    out["fg"][cidx[sel]] = True
    mg = final[:, sel].int().argmax(0)
    pb, tb = boxes[cidx[sel]], gt[mg]
    pairs = torch.cat([(pb[:, :2] - pb[:, 2:] / 2) - (tb[:, :2] - tb[:, 2:] / 2), (pb[:, :2] + pb[:, 2:] / 2) - (tb[:, :2] + tb[:, 2:] / 2)], 1)
    out["e"] = pairs.abs().min().item()
    return out


@functools.lru_cache(maxsize=None)
def margins(case):
    """{"a".."e": the case's margins (inf where a decision does not occur), "patches": the per-patch traces}."""
    raw, tg = build(case)
    grid, stride, _ = geometry(case.P)
    lab = to_cxcywh(tg.double())
    traces = []
    for n in range(raw.shape[0]):
        ng = int((lab[n].sum(1) > 0).sum())
        traces.append(_trace_patch(lab[n, :ng, 1:], raw[n].double(), grid, stride))
    res = {k: min(t[k] for t in traces) for k in "abcde"}
    res["patches"] = traces
    return res


def admissible(m, tie=False):
    return (m["a"] > 1e-3 and m["b"] > 1e-2 and m["c"] > 1e-3 and m["d"] > 1e-3 and (m["e"] == 0.0 if tie else m["e"] > 1e-4))


def evaluate(case, dtype):
    """The oracle on a case in `dtype`: {"metrics": the five losses, "num_fg", "num_gt" (ints), "scale", "grad": LOSS_SCALE *
    d total_loss / d raw [N, A, 6], "fg": [N, A] bool}, values as fp64 / python numbers."""
    raw, tg = build(case)
    _, _, hw = geometry(case.P)
    x = raw.to(dtype).clone().requires_grad_(True)
    lab = to_cxcywh(tg.to(dtype))
    out, assign = yolox_ref.losses_from_raw(x, hw, lab, case.use_l1, STRIDES)
    (out[0] * LOSS_SCALE).backward()
    fg = torch.stack([a[0] if a is not None else torch.zeros(x.shape[1], dtype=torch.bool) for a in assign])
    num_fg = int(fg.sum())
    num_gt = int((lab.sum(2) > 0).sum())
    assert abs(float(out[5]) - num_fg / max(num_gt, 1)) < 1e-6
    scale = (torch.tensor(LOSS_SCALE, dtype=dtype) / max(num_fg, 1)).double().item()
    return dict(metrics=[float(v.detach()) for v in out[:5]], num_fg=num_fg, num_gt=num_gt, scale=scale, grad=x.grad.double(), fg=fg)


@functools.lru_cache(maxsize=None)
def reference(case):
    """evaluate(case, fp64), computed once and shared.  Treat as read-only."""
    return evaluate(case, torch.float64)


def distances(got, ref):
    """Distance of an evaluation `got` (metrics, scale, grad as in evaluate()) from `ref`: {"metrics": 5 relative errors
    (0 where both are exactly 0, inf where only the reference is), "scale": relative, "grad_max": per column max-norm over
    max |ref|, "grad_fg_l2": relative L2 over the foreground rows of columns 0-3 and 5 (0 without foreground)}."""
    mets = []
    for g, r in zip(got["metrics"], ref["metrics"]):
        mets.append((0.0 if g == 0.0 else float("inf")) if r == 0.0 else abs(g - r) / abs(r))
    G, R = got["grad"].double(), ref["grad"]
    gmax = []
    for c in range(6):
        den = R[..., c].abs().max().item()
        err = (G[..., c] - R[..., c]).abs().max().item()
        gmax.append((0.0 if err == 0.0 else float("inf")) if den == 0.0 else err / den)
    fg = ref["fg"]
    cols = [0, 1, 2, 3, 5]
    l2 = 0.0
    if fg.any():
        l2 = ((G[fg][:, cols] - R[fg][:, cols]).norm() / R[fg][:, cols].norm()).item()
    return dict(metrics=mets, scale=abs(got["scale"] - ref["scale"]) / ref["scale"], grad_max=gmax, grad_fg_l2=l2)


def check_bars(dist, tag=""):
    """Holds distances() to the fixed bars; raises AssertionError naming every quantity over its bar."""
    over = []
    for i, (v, bar) in enumerate(zip(dist["metrics"], METRIC_RTOL)):
        if not v <= bar:
            over.append((f"metric {i}", v, bar))
    if not dist["scale"] <= SCALE_RTOL:
        over.append(("scale", dist["scale"], SCALE_RTOL))
    for c, (v, bar) in enumerate(zip(dist["grad_max"], GRAD_MAX)):
        if not v <= bar:
            over.append((f"grad column {c} max-norm", v, bar))
    if not dist["grad_fg_l2"] <= GRAD_FG_L2:
        over.append(("grad foreground L2", dist["grad_fg_l2"], GRAD_FG_L2))
    assert not over, (tag, over)
