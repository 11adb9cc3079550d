"""Committed inputs for the SimOTA detector loss over EVERY box of a patch (`yolox_loss_wide_kernel` through
`jn_yolox_loss_wide`): patches with 9 to 64 ground-truth boxes, which the default kernel cuts to eight.

Everything comes from tests/simota_cases.py: the same `Case`, the same generator (`build`: patch 0 of a case holds nb real
boxes), the same fp64 oracle, margins, admissibility thresholds and bars.  tests/test_simota_wide_cases_cpu.py shows on the
CPU that every case here is admissible under those margins, that an fp32 evaluation of the oracle assigns as fp64 does and
that it stays inside the EXISTING bars (8 x the fp32 oracle's distance from fp64 on the narrow list), so the bars apply
unchanged; it prints the fp32 distances of this list.  tests/test_gpu_simota_wide.py holds the kernel to them.

One layout of this file's own, "zero-row-then-wide": a zero row followed by nb - 1 real boxes ("spread").  ng counts the
real rows, nb - 1; the published head takes the FIRST ng rows, so the zero row is a box and the last real row is not.

No case puts a box without an in-radius candidate beside candidates of other boxes: its choice among costs of 1e6 + x
is not decidable in fp32.
"""
import functools

import torch

from oracle import yolox_ref
from tests import simota_cases as sc
from tests.simota_cases import Case

WIDE_CASES = [
    Case(64, 2, 9, 1, "clustered"),
    Case(64, 1, 16, 1, "spread", False),
    Case(160, 2, 12, 1, "clustered"),
    Case(160, 2, 24, 4, "spread"),
    Case(160, 3, 16, 3, "clustered+empty+spread", False),
    Case(448, 1, 40, 10, "spread"),
    Case(448, 2, 24, 6, "clustered+spread", False),
    Case(160, 1, 64, 3, "spread"),
    Case(160, 2, 12, 2, "stray+zero-row-first"),
]
ZERO_FIRST_WIDE = Case(160, 1, 11, 1, "zero-row-then-wide")       # a zero row, then ten real boxes: ng = 10
ALL = WIDE_CASES + [ZERO_FIRST_WIDE]
DETERMINISM_CASE = Case(448, 1, 40, 10, "spread")                 # the 40-box patch


@functools.lru_cache(maxsize=None)
def build(case):
    """(raw [N, A, 6] fp32, targets [N, nb, 5] fp32 xyxy) of a case.  Treat both as read-only."""
    if case.layout != "zero-row-then-wide":
        return sc.build(case)
    assert case.N == 1
    raw, tg = sc.build(Case(case.P, 1, case.nb - 1, case.seed, "spread", case.use_l1))
    return raw, torch.cat([torch.zeros((1, 1, 5)), tg], 1)


@functools.lru_cache(maxsize=None)
def margins(case):
    """simota_cases.margins for any case of this file."""
    if case.layout != "zero-row-then-wide":
        return sc.margins(case)
    raw, tg = build(case)
    grid, stride, _ = sc.geometry(case.P)
    lab = sc.to_cxcywh(tg.double())
    traces = []
    for n in range(raw.shape[0]):
        ng = int((lab[n].sum(1) > 0).sum())
        traces.append(sc._trace_patch(lab[n, :ng, 1:], raw[n].double(), grid, stride))
    res = {k: min(t[k] for t in traces) for k in "abcde"}
    res["patches"] = traces
    return res


def evaluate(case, dtype):
    """simota_cases.evaluate for any case of this file."""
    if case.layout != "zero-row-then-wide":
        return sc.evaluate(case, dtype)
    raw, tg = build(case)
    _, _, hw = sc.geometry(case.P)
    x = raw.to(dtype).clone().requires_grad_(True)
    lab = sc.to_cxcywh(tg.to(dtype))
    out, assign = yolox_ref.losses_from_raw(x, hw, lab, case.use_l1, sc.STRIDES)
    (out[0] * sc.LOSS_SCALE).backward()
    fg = torch.stack([a[0] if a is not None else torch.zeros(x.shape[1], dtype=torch.bool) for a in assign])
    num_fg = int(fg.sum())
    num_gt = int((lab.sum(2) > 0).sum())
    scale = (torch.tensor(sc.LOSS_SCALE, dtype=dtype) / max(num_fg, 1)).double().item()
    return dict(metrics=[float(v.detach()) for v in out[:5]], num_fg=num_fg, num_gt=num_gt, scale=scale, grad=x.grad.double(), fg=fg)


@functools.lru_cache(maxsize=None)
def reference(case):
    """evaluate(case, fp64), computed once and shared.  Treat as read-only."""
    return evaluate(case, torch.float64)


@functools.lru_cache(maxsize=None)
def assignment(case):
    """The fp64 oracle's assignment, per patch None (no box, or no candidate) or a dict: matched [nfg] = the box of every
    foreground anchor in anchor order, claims [nfg] = how many boxes chose that anchor before the conflict was resolved."""
    raw, tg = build(case)
    grid, stride, _ = sc.geometry(case.P)
    lab = sc.to_cxcywh(tg.double())
    res = []
    for n in range(raw.shape[0]):
        ng = int((lab[n].sum(1) > 0).sum())
        r = raw[n].double()
        boxes = torch.cat([(r[:, :2] + grid) * stride[:, None], torch.exp(r[:, 2:4]) * stride[:, None]], 1)
        if ng == 0:
            res.append(None)
            continue
        fg, matched, _ = yolox_ref.simota_assign(lab[n, :ng, 1:], boxes, r[:, 4], r[:, 5], grid, stride)
        # claims: the oracle's matching restated up to, not including, its conflict step (as simota_cases._trace_patch does)
        gt = lab[n, :ng, 1:]
        xc, yc, rad = (grid[:, 0] + 0.5) * stride, (grid[:, 1] + 0.5) * stride, 1.5 * stride
        d = torch.stack([xc[None] - (gt[:, 0:1] - rad[None]), yc[None] - (gt[:, 1:2] - rad[None]),
                         (gt[:, 0:1] + rad[None]) - xc[None], (gt[:, 1:2] + rad[None]) - yc[None]], 2).min(-1).values
        inc = d > 0
        cand = inc.sum(0) > 0
        if int(cand.sum()) == 0:
            res.append(None)
            continue
        ious = yolox_ref.pairwise_iou_cxcywh(gt, boxes[cand])
        p = (r[cand, 5].sigmoid() * r[cand, 4].sigmoid()).sqrt()
        cost = (-torch.log(p)).clamp(max=100.0)[None] + 3.0 * -torch.log(ious + 1e-8) + 1e6 * (~inc[:, cand]).double()
        ks = torch.topk(ious, min(10, ious.shape[1]), dim=1).values.sum(1).int().clamp(min=1)
        match = torch.zeros_like(cost, dtype=torch.bool)
        for g in range(ng):
            match[g, torch.topk(cost[g], int(ks[g]), largest=False).indices] = True
        claims = match.sum(0)
        assert torch.equal(cand.nonzero().squeeze(1)[claims > 0], fg.nonzero().squeeze(1))
        res.append(dict(matched=matched, claims=claims[claims > 0]))
    return res
