#!/usr/bin/env python3
"""Device time of the detector's threshold / sort / NMS stage under its two candidate policies, on one GPU, in one
process: ``jn_postprocess`` (the first 2048 passing anchors enter the sort) against ``jn_postprocess_all`` (every passing
anchor does), called as the hot path calls them (no stats buffer).  Two inputs:

  (a) the raw head output of the tools/eval_ab.py model (configs[2] topology, yolox-s detector, fresh weights) on 64
      random patches of 448 px (A = 4116), at the config's threshold 0.5 (few or no candidates) and at 1e-5 (every
      anchor passes), max_out = max_det_per_patch = 64;
  (b) the committed 8400-candidate lattice at 640 px (tests/postprocess_all_cases.py, case count-8400), 64 copies, with
      max_out = 64 and with max_out = 8400 (every greedy round runs).

Each sample is `--inner` back-to-back launches between two HIP events, divided by `--inner`; after one warm-up of every
setting the two policies alternate, `--repeats` samples each; the figure is the median with the spread (min, max).  For
(a) at 1e-5 it also counts the written rows and the patches that differ between the policies.  Prints ONE JSON line and
writes it to `--out`.  Every GPU step runs under a hard time limit.

    python tools/postprocess_ab.py [--patches 64] [--repeats 7] [--inner 20] [--out profiles/postprocess_ab.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from infer_ab import Limit  # noqa: E402

POLICIES = (("first2048", "jn_postprocess"), ("all", "jn_postprocess_all"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "postprocess_ab.json"))
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import _lib
    from jolineedle_amd._lib import check, ptr
    from jolineedle_amd.config import model_config
    from tests import postprocess_all_cases as pa

    assert torch.cuda.is_available(), "postprocess_ab needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    N, P, lim = args.patches, 448, args.step_timeout
    out = {"tool": "postprocess_ab", "patches": N, "repeats": args.repeats, "launches_per_sample": args.inner,
           "note": "ms per launch of N patches under HIP events, median [min, max]; stats buffer NULL as on the hot path"}

    def run(entry, raw, conf, nms, clamp_max, K, boxes, counts):
        check(getattr(lib, entry)(ptr(raw), raw.shape[0], raw.shape[1], C.c_float(conf), C.c_float(nms), C.c_float(clamp_max), K,
                                  ptr(boxes), ptr(counts), None, _lib.current_stream(dev)), entry)

    def sample(entry, raw, conf, nms, clamp_max, K, boxes, counts):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            run(entry, raw, conf, nms, clamp_max, K, boxes, counts)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.inner

    def ab(name, raw, conf, nms, clamp_max, K):
        """Both policies on one input, interleaved.  Returns the outputs of either for the comparison."""
        res, ms = {}, {p: [] for p, _ in POLICIES}
        for p, entry in POLICIES:                  # warm-up, and the outputs
            boxes = torch.zeros((raw.shape[0], K, 7), device=dev)
            counts = torch.zeros((raw.shape[0],), device=dev, dtype=torch.int32)
            with Limit(lim):
                sample(entry, raw, conf, nms, clamp_max, K, boxes, counts)
            res[p] = (boxes, counts)
        for r in range(args.repeats):
            for p, entry in (POLICIES if r % 2 == 0 else POLICIES[::-1]):
                with Limit(lim):
                    ms[p].append(sample(entry, raw, conf, nms, clamp_max, K, *res[p]))
        score = raw[..., 4] * raw[..., 5]
        passing = (score >= conf).sum(1)
        rec = {"A": raw.shape[1], "conf": conf, "max_out": K,
               "passing_per_patch": {"min": int(passing.min()), "mean": round(float(passing.float().mean()), 1), "max": int(passing.max())}}
        for p, _ in POLICIES:
            rec[f"{p}_ms"] = round(statistics.median(ms[p]), 4)
            rec[f"{p}_ms_spread"] = [round(min(ms[p]), 4), round(max(ms[p]), 4)]
            rec[f"{p}_boxes_per_patch_mean"] = round(float(res[p][1].float().mean()), 1)
        rec["all_over_first2048"] = round(rec["all_ms"] / rec["first2048_ms"], 3)
        (b0, c0), (b1, c1) = res["first2048"], res["all"]
        rows = (b0 != b1).any(2)
        rec["rows_that_differ"] = int(rows.sum())
        rec["patches_that_differ"] = int((rows.any(1) | (c0 != c1)).sum())
        out[name] = rec
        print(f"{name}: first2048 {rec['first2048_ms']} ms, all {rec['all_ms']} ms, rows that differ {rec['rows_that_differ']}",
              file=sys.stderr, flush=True)

    # (a) the eval_ab model's own head output
    with Limit(lim):
        torch.manual_seed(args.seed)
        model = ja.GPT(model_config(patch_size=P, block_size=20), max_batch=N, device=dev)
        model.eval()
        model.sync_weights()
        eng = model.engine()
        A = sum((P // s) ** 2 for s in (8, 16, 32))
        x = torch.randint(0, 256, (N, 3, P, P), generator=torch.Generator().manual_seed(args.seed), dtype=torch.uint8).to(dev).float().div(255)
        raw = torch.empty((N, A, 6), device=dev)
        check(lib.jn_detect(eng.handle, ptr(x), N, None, None, ptr(raw), _lib.current_stream(dev)), "jn_detect")
        torch.cuda.synchronize()
    K, nms = eng.cfg.max_det_per_patch, eng.cfg.det_nms_threshold
    ab("model_448_conf0.5", raw, 0.5, nms, float(P - 1), K)
    ab("model_448_conf1e-5", raw, 1e-5, nms, float(P - 1), K)

    # (b) the committed lattice: 8400 candidates per patch at 640 px
    case = pa.BY_NAME["count-8400"]
    lattice = torch.from_numpy(np.array(pa.build(case)))[None].repeat(N, 1, 1).contiguous().to(dev)
    ab("lattice_640_max_out64", lattice, case.conf, case.nms, float(case.P - 1), 64)
    ab("lattice_640_max_out8400", lattice, case.conf, case.nms, float(case.P - 1), pa.POST_ALL_MAX_A)

    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
