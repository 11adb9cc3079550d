#!/usr/bin/env python3
"""A/B of the two routes of ``NeedleGeneralEnv.get_detection_batch`` at the headline workload (B = 64, 4480 x 4480 px,
448 px patches, 1..3 boxes per image, sample_neg = 1) on one GPU, in one process, for fp32 and uint8 images.

Prints ONE JSON line (and writes it to --out), per element type:
  host_ms / device_ms     wall time of one call, the device idle before and after (a synchronisation on both sides), the
                          two routes interleaved and the first of each pair alternating: median of --iters (7) calls
  host_ms_spread / ...    max - min of those calls
  cells_kernel_ms         device time of the three launches of jn_detection_cells (HIP events, no readback), median
  gather_kernel_ms        device time of the one indexed gather of the n patches, median
  n_patches               rows of the batch (the routes agree on the positives; the negatives are other draws)

Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/detbatch_ab.py [--iters 7] [--warmup 2] [--out profiles/detbatch_ab.json] [--step-timeout 300]
"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


class Limit:
    """Hard per-step time limit: faulthandler's watchdog thread exits the process even when a GPU call never returns."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--sample-neg", type=int, default=1)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="fp32,uint8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import _lib
    from jolineedle_amd._lib import check, ptr
    from jolineedle_amd.detection import detection_cells_device
    from jolineedle_amd.trajectory import gather_indexed

    assert torch.cuda.is_available(), "detbatch_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, P, G, sn, lim = args.batch, args.patch_size, args.grid, args.sample_neg, args.step_timeout
    out = {"tool": "detbatch_ab", "batch": B, "patch_size": P, "grid": G, "sample_neg": sn, "iters": args.iters}
    lib = _lib.load_library()

    for kind in args.dtypes.split(","):
        with Limit(lim):
            batch = ja.synthetic_batch(B, G, P, seed=12345, device=dev, dtype=torch.uint8 if kind == "uint8" else torch.float32)
            env = ja.NeedleGeneralEnv(batch["image"], batch["bboxes"], P, 20, 1, True, uint8_images=kind == "uint8")
            torch.cuda.synchronize()

        def one(route, i):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            patches, boxes = env.get_detection_batch(sn, device=True, seed=i) if route == "device" else env.get_detection_batch(sn)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, int(patches.shape[0]), boxes

        times = {"host": [], "device": []}
        rows = {}
        for i in range(args.warmup + args.iters):
            for route in (("host", "device") if i % 2 == 0 else ("device", "host")):
                with Limit(lim):
                    ms, rows[route], boxes = one(route, i)
                if i >= args.warmup:
                    times[route].append(ms)
        assert rows["host"] == rows["device"], rows
        with Limit(lim):
            hp, hb = env.get_detection_batch(0)
            dp, db = env.get_detection_batch(0, device=True)
            assert torch.equal(hp, dp) and torch.equal(hb, db), "the routes disagree on the positive rows"

        # the device route's two stages on their own
        bb = env._bboxes_dev
        nb, cap = int(bb.shape[1]), B * G * G
        cells = torch.empty((cap, 3), device=dev, dtype=torch.int64)
        targets = torch.empty((cap, nb, 5), device=dev, dtype=torch.int64)
        offsets = torch.empty((B + 1,), device=dev, dtype=torch.int32)
        n_pos = torch.empty((B,), device=dev, dtype=torch.int32)
        stream = _lib.current_stream(dev)
        k_ms, g_ms = [], []
        for i in range(args.warmup + args.iters):
            with Limit(lim):
                ms, _ = _event_ms(lambda: check(lib.jn_detection_cells(ptr(bb), None, B, nb, G, G, P, sn, i, cap, ptr(cells), ptr(targets),
                                                                       ptr(offsets), ptr(n_pos), stream), "jn_detection_cells"))
                c, _, _, _ = detection_cells_device(bb, G, G, P, sn, i)
                ii, pos = c[:, 0].contiguous(), c[:, 1:].contiguous()
                gms, _ = _event_ms(lambda: gather_indexed(env._images, ii, pos, P, _check_positions=False))
            if i >= args.warmup:
                k_ms.append(ms)
                g_ms.append(gms)
        res = {"n_patches": rows["device"], "cells_kernel_ms": round(statistics.median(k_ms), 4),
               "gather_kernel_ms": round(statistics.median(g_ms), 4)}
        for route in ("host", "device"):
            res[f"{route}_ms"] = round(statistics.median(times[route]), 3)
            res[f"{route}_ms_spread"] = round(max(times[route]) - min(times[route]), 3)
            res[f"{route}_ms_all"] = [round(t, 3) for t in times[route]]
        res["device_vs_host"] = round(res["device_ms"] / res["host_ms"], 4)
        out[kind] = res
        del env, batch, hp, dp, cells, targets
        torch.cuda.empty_cache()

    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
