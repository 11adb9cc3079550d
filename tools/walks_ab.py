#!/usr/bin/env python3
"""A/B of the two routes of ``SupervisedTrainer.generate_trajectories`` at the headline workload (B = 64, 4480 x 4480 px,
448 px patches: a 10 x 10 grid, T = 20, 1..3 boxes per image, max_keypoints = 2) on one GPU, in one process.

Prints ONE JSON line (and writes it to --out):
  host_ms / device_ms       wall time of one call (walks, upload, both gathers), the device idle before and after (a
                            synchronisation on both sides), the two routes interleaved and the first of each pair
                            alternating: median of --iters (7) calls
  host_ms_spread / ...      max - min of those calls
  host_walks_ms             wall time of the host route's walk loop alone (one NeedleSimpleEnv per image, no gather), median
  device_walks_ms           wall time of ``teacher_walks_device`` alone (three launches + the readback of the offsets), median
  walks_kernel_ms           device time of the three launches of jn_teacher_walks (HIP events, no readback), median
  steps_mean                mean walk length of the device route's walks (before the cut to T)

Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/walks_ab.py [--iters 7] [--warmup 2] [--out profiles/walks_ab.json] [--step-timeout 300]
"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

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


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--max-keypoints", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import _lib
    from jolineedle_amd._lib import check, ptr
    from jolineedle_amd.trajectory import NeedleSimpleEnv, teacher_walks_device

    assert torch.cuda.is_available(), "walks_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, P, G, T, K, lim = args.batch, args.patch_size, args.grid, args.seq_len, args.max_keypoints, args.step_timeout
    out = {"tool": "walks_ab", "batch": B, "patch_size": P, "grid": G, "seq_len": T, "max_keypoints": K, "iters": args.iters}
    lib = _lib.load_library()
    cfg = ja.CfgNode(patch_size=P, max_seq_len=T, min_keypoints=0, max_keypoints=K, binomial_keypoints=False, seed=1)
    trainer = ja.SupervisedTrainer(cfg, SimpleNamespace(device=dev))       # generate_trajectories needs the device only

    with Limit(lim):
        batch = ja.synthetic_batch(B, G, P, seed=12345, device=dev, dtype=torch.float32)
        batch = {"image": batch["image"], "bboxes": batch["bboxes"].cpu()}                   # boxes as a loader hands them over
        torch.cuda.synchronize()

    times = {"host": [], "device": []}
    for i in range(args.warmup + args.iters):
        for route in (("host", "device") if i % 2 == 0 else ("device", "host")):
            with Limit(lim):
                ms, tr = _wall_ms(lambda: trainer.generate_trajectories(batch, seed=1000 + i, device=route == "device"))
                assert tr["patches"].shape[:2] == (B, T)
                del tr
            if i >= args.warmup:
                times[route].append(ms)

    # the walks on their own: the host loop, the device call, the three launches
    boxes = batch["bboxes"]

    def host_walks(seed):
        for b in range(B):
            bb = boxes[b]
            env = NeedleSimpleEnv(None, P, bb[(bb != 0).any(dim=-1)], seed=seed + b, height=G * P, width=G * P)
            env.generate_sample_indices(T, 0, K, False, None)

    bb_dev = boxes.to(dev)
    nb, cap = int(bb_dev.shape[1]), B * G * G
    i64 = lambda *s: torch.empty(s, device=dev, dtype=torch.int64)
    f32 = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    bufs = [i64(B, T, 2), i64(B, T), i64(B, T), i64(B, T), f32(B, T), f32(B, T, nb, 6),
            torch.empty((B,), device=dev, dtype=torch.int32), torch.empty((B, G, G), device=dev, dtype=torch.uint8),
            i64(cap, 3), f32(cap, nb, 6), torch.empty((B + 1,), device=dev, dtype=torch.int32)]
    stream = _lib.current_stream(dev)
    h_ms, d_ms, k_ms, steps = [], [], [], []
    for i in range(args.warmup + args.iters):
        with Limit(lim):
            hms, _ = _wall_ms(lambda: host_walks(1000 + i))
            dms, w = _wall_ms(lambda: teacher_walks_device(bb_dev, G, G, P, T, 0, K, False, 1000 + i))
            kms, _ = _event_ms(lambda: check(lib.jn_teacher_walks(ptr(bb_dev), None, B, nb, G, G, P, T, 0, K, 0, 1000 + i, cap,
                                                                  *(ptr(t) for t in bufs), stream), "jn_teacher_walks"))
        if i >= args.warmup:
            h_ms.append(hms)
            d_ms.append(dms)
            k_ms.append(kms)
            steps.append(float(w["n_steps"].float().mean()))
    for route in ("host", "device"):
        out[f"{route}_ms"] = round(statistics.median(times[route]), 3)
        out[f"{route}_ms_spread"] = round(max(times[route]) - min(times[route]), 3)
        out[f"{route}_ms_all"] = [round(t, 3) for t in times[route]]
    out["device_vs_host"] = round(out["device_ms"] / out["host_ms"], 4)
    out["host_walks_ms"] = round(statistics.median(h_ms), 3)
    out["host_walks_ms_spread"] = round(max(h_ms) - min(h_ms), 3)
    out["device_walks_ms"] = round(statistics.median(d_ms), 3)
    out["device_walks_ms_spread"] = round(max(d_ms) - min(d_ms), 3)
    out["walks_kernel_ms"] = round(statistics.median(k_ms), 4)
    out["walks_kernel_ms_spread"] = round(max(k_ms) - min(k_ms), 4)
    out["steps_mean"] = round(statistics.mean(steps), 2)

    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
