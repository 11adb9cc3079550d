#!/usr/bin/env python3
"""A/B of uint8 against fp32 images at the c3 shapes (B = 64, T = 20, 448 px, 10 x 10 grid) on one GPU, in one process.

Prints ONE JSON line:
  upload_ms_{fp32,u8}       median time of one batch's host-to-device copy from pinned memory (CUDA events)
  train_iter_ms_{fp32,u8}   median time of one REINFORCE train_iteration (env build included, as in bench.py) on an fp32
                            env and on a uint8 env (uint8_images=True) of the same images, with the same weights (every
                            iteration starts from the seeded parameters and a fresh AdamW) and the same seed, the two
                            kinds interleaved, the first of each pair alternating
  u8_vs_fp32                train_iter_ms_u8 / train_iter_ms_fp32 - 1

The fp32 images are the bytes / 255 computed exactly (a 256-entry table of ToTensor's values), so both envs see the same
pixel values.  Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/uint8_ab.py [--iters 10] [--warmup 2] [--uploads 5] [--step-timeout 300]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--uploads", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    from bench import TrainingStart

    assert torch.cuda.is_available(), "uint8_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, T, P, G = args.batch, args.seq_len, args.patch_size, args.grid
    lim = args.step_timeout
    out = {"tool": "uint8_ab", "batch": B, "seq_len": T, "patch_size": P, "grid": G, "iters": args.iters}

    # ---- inputs: uint8 bytes and the exact fp32 image they stand for -----------------------------------------------
    with Limit(lim):
        batch = ja.synthetic_batch(B, G, P, seed=12345, device=dev, dtype=torch.uint8)
        u8, bboxes, start = batch["image"], batch["bboxes"], batch["start_positions"]
        lut = torch.arange(256, dtype=torch.uint8).float().div(255).to(dev)
        f32 = torch.empty(u8.shape, dtype=torch.float32, device=dev)
        for b in range(B):
            f32[b] = lut[u8[b].long()]
        torch.cuda.synchronize()
    out["image_bytes_fp32"], out["image_bytes_u8"] = f32.numel() * 4, u8.numel()

    # ---- upload of one batch from pinned host memory ---------------------------------------------------------------
    for name, src in (("fp32", f32), ("u8", u8)):
        with Limit(lim):
            host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
            dst = torch.empty_like(src)
            times = []
            for _ in range(args.uploads + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(host, non_blocking=True)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            med = statistics.median(times[1:])
            out[f"upload_ms_{name}"] = round(med, 2)
            out[f"upload_GBps_{name}"] = round(src.numel() * src.element_size() / med / 1e6, 1)
            del host, dst
            torch.cuda.empty_cache()

    # ---- train_iteration, interleaved ------------------------------------------------------------------------------
    with Limit(lim):
        model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None),
                       max_batch=B, device=dev)
        model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345,
                         learning_rate=1e-4, gradient_accumulation=1)
        trainer = ja.ReinforceTrainer(cfg, model)
        initial = TrainingStart(model)
        forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(777)).to(dev)
        eng = model.engine()
        torch.cuda.synchronize()

    def one(kind):
        initial.restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env = ja.NeedleGeneralEnv(u8 if kind == "u8" else f32, bboxes, P, T, 1, True, engine=eng,
                                  uint8_images=kind == "u8")
        m = trainer.train_iteration(env, forced_actions=forced, start_positions=start, sample_actions=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(m["loss"]), int(m["steps"])

    times = {"fp32": [], "u8": []}
    loss = {}
    for i in range(args.warmup + args.iters):
        for kind in (("fp32", "u8") if i % 2 == 0 else ("u8", "fp32")):
            with Limit(lim):
                ms, loss[kind], steps = one(kind)
            assert steps == T
            if i >= args.warmup:
                times[kind].append(ms)
    for kind in ("fp32", "u8"):
        out[f"train_iter_ms_{kind}"] = round(statistics.median(times[kind]), 3)
        out[f"train_iter_ms_{kind}_all"] = [round(t, 2) for t in times[kind]]
        out[f"loss_{kind}"] = loss[kind]
    out["u8_vs_fp32"] = round(out["train_iter_ms_u8"] / out["train_iter_ms_fp32"] - 1.0, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
