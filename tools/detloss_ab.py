#!/usr/bin/env python3
"""Device time of the detector's SimOTA loss under its two box policies, on one GPU, in one process: ``jn_yolox_loss``
(`yolox_loss_kernel`, at most 8 boxes per patch) against ``jn_yolox_loss_wide`` (`yolox_loss_wide_kernel`, every box), on
64 patches of 448 px (A = 4116) built from the committed case generators of tests/simota_cases.py:

  (a) cap8 on the committed nb = 8 case Case(448, 8, 8, 1, "spread+clustered+empty"), tiled to 64 patches;
  (b) the wide kernel on the same input;
  (c) the wide kernel at 24 boxes per patch: Case(448, 2, 24, 6, "clustered+spread") of tests/simota_wide_cases.py, tiled;
  (d) the wide kernel at 64 boxes per patch: Case(448, 1, 64, 3, "spread"), tiled;
  (floor) cap8 on 64 patches without a box: the objectness loop and what the entry itself costs.

Both entries allocate their scratch and wait for the stream on every call, so a figure is the kernel pair (loss +
finalize) PLUS that per-call cost, which is the same for every variant: read the differences, and the floor.  Each
sample is `--inner` back-to-back calls between two HIP events, divided by `--inner`; after one warm-up of every variant
the variants alternate, `--repeats` samples each; the figure is the median with (max - min).  Prints ONE JSON line and
writes it to `--out`.  Every GPU step runs under a hard time limit.

    python tools/detloss_ab.py [--patches 64] [--repeats 7] [--inner 20] [--out profiles/detloss_ab.json]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from infer_ab import Limit  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "detloss_ab.json"))
    args = ap.parse_args()

    from jolineedle_amd import yolox
    from tests import simota_cases as sc

    assert torch.cuda.is_available(), "detloss_ab needs the GPU"
    dev = torch.device("cuda:0")
    N, P, lim = args.patches, 448, args.step_timeout

    def tiled(case):
        raw, tg = sc.build(case)
        reps = (N + case.N - 1) // case.N
        return raw.repeat(reps, 1, 1)[:N].contiguous().to(dev), tg.repeat(reps, 1, 1)[:N].contiguous().to(dev)

    eight = tiled(sc.Case(448, 8, 8, 1, "spread+clustered+empty", False))
    empty = (eight[0], torch.zeros((N, 1, 5), device=dev))
    variants = [("a_cap8_nb8", "cap8", eight), ("b_all_nb8", "all", eight),
                ("c_all_nb24", "all", tiled(sc.Case(448, 2, 24, 6, "clustered+spread", False))),
                ("d_all_nb64", "all", tiled(sc.Case(448, 1, 64, 3, "spread"))),
                ("floor_cap8_no_box", "cap8", empty)]

    def sample(policy, raw, tg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            res = yolox.yolox_loss(raw, tg, P, sc.STRIDES, True, sc.LOSS_SCALE, boxes=policy)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.inner, res

    out = {"tool": "detloss_ab", "patches": N, "patch_size": P, "repeats": args.repeats, "calls_per_sample": args.inner,
           "note": "ms per call of N patches under HIP events, median and (max - min); a call = loss + finalize kernels plus "
                   "the entry's own scratch allocation and stream wait, equal for every variant (see floor)"}
    ms, last = {name: [] for name, _, _ in variants}, {}
    for name, policy, (raw, tg) in variants:                       # warm-up, and the outputs
        with Limit(lim):
            _, last[name] = sample(policy, raw, tg)
    for r in range(args.repeats):
        for name, policy, (raw, tg) in (variants if r % 2 == 0 else variants[::-1]):
            with Limit(lim):
                ms[name].append(sample(policy, raw, tg)[0])
    for name, policy, (raw, tg) in variants:
        lab = sc.to_cxcywh(tg)
        boxes = (lab.sum(2) > 0).sum(1)
        num_fg = round(sc.LOSS_SCALE / float(last[name][2]))
        out[name] = {"policy": policy, "nb": tg.shape[1], "boxes_per_patch_max": int(boxes.max()),
                     "boxes_per_patch_mean": round(float(boxes.float().mean()), 1), "num_fg": num_fg,
                     "ms": round(statistics.median(ms[name]), 4), "ms_spread": round(max(ms[name]) - min(ms[name]), 4)}
        print(f"{name}: {out[name]['ms']} ms (spread {out[name]['ms_spread']}), num_fg {num_fg}", file=sys.stderr, flush=True)
    out["b_over_a"] = round(out["b_all_nb8"]["ms"] / out["a_cap8_nb8"]["ms"], 3)
    out["same_bits_a_b"] = all(bool(torch.equal(x, y)) for x, y in zip(last["a_cap8_nb8"], last["b_all_nb8"]))

    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
