#!/usr/bin/env python3
"""What image views cost and what they save, at the c3 shapes (B = 64, T = 20, 448 px, 10 x 10 grid) on one GPU, in one
process, for uint8 and for fp32 sources.  Three kinds of REINFORCE ``train_iteration`` (env build included, as in
bench.py), interleaved, the order rotating from round to round:

  plain        an env on the stored images, no augmentation — the floor
  materialize  what a user could do before: ``ImageViews.materialize()`` (torch transpose / flip / shifted copy into a
               zero canvas) every iteration, then a plain env on the canvas with the transformed boxes
  views        ``NeedleGeneralEnv(None, boxes, ..., views=...)``: the transform applied inside the patch reads

The views are drawn once (``ImageViews.sample`` with rotations and translations) and reused, so that every iteration of a
kind does the same work; building the ``ImageViews`` object and transforming the boxes is inside the timed region of
both kinds that use it.  Prints ONE JSON line: median ms per kind and dtype, all samples, views - plain and
views / materialize - 1.  Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/views_ab.py [--iters 6] [--warmup 2] [--dtypes uint8 fp32] [--step-timeout 300]
"""
import argparse
import faulthandler
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
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
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", nargs="+", default=["uint8", "fp32"])
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    from jolineedle_amd.views import ImageViews
    from bench import TrainingStart

    assert torch.cuda.is_available(), "views_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, T, P, G = args.batch, args.seq_len, args.patch_size, args.grid
    lim = args.step_timeout
    out = {"tool": "views_ab", "batch": B, "seq_len": T, "patch_size": P, "grid": G, "iters": args.iters}

    with Limit(lim):
        batch = ja.synthetic_batch(B, G, P, seed=12345, device=dev, dtype=torch.uint8)
        u8, bboxes, start = batch["image"], batch["bboxes"], batch["start_positions"]
        model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None),
                       max_batch=B, device=dev)
        model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345,
                         learning_rate=1e-4, gradient_accumulation=1)
        trainer = ja.ReinforceTrainer(cfg, model)
        initial = TrainingStart(model)
        forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(777)).to(dev)
        eng = model.engine()
        drawn = ImageViews.sample(u8, bboxes, True, True, np.random.default_rng(12345), P)
        rot, ty, tx = drawn.rot.copy(), drawn.ty.copy(), drawn.tx.copy()
        out["rotations_drawn"] = {str(k): int((rot == k).sum()) for k in (0, 90, 180, 270)}
        del drawn
        torch.cuda.synchronize()

    for dt in args.dtypes:
        with Limit(lim):
            if dt == "uint8":
                src = u8
            else:
                lut = torch.arange(256, dtype=torch.uint8).float().div(255).to(dev)
                src = torch.empty(u8.shape, dtype=torch.float32, device=dev)
                for b in range(B):
                    src[b] = lut[u8[b].long()]
            torch.cuda.synchronize()

        def one(kind):
            initial.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "plain":
                env = ja.NeedleGeneralEnv(src, bboxes, P, T, 1, True, engine=eng, uint8_images=dt == "uint8")
            else:
                views = ImageViews(src, rot, ty, tx, patch_size=P)
                tb = views.transform_bboxes(bboxes)
                if kind == "views":
                    env = ja.NeedleGeneralEnv(None, tb, P, T, 1, True, engine=eng, views=views)
                else:
                    env = ja.NeedleGeneralEnv(views.materialize(), tb, P, T, 1, True, engine=eng, uint8_images=dt == "uint8")
            m = trainer.train_iteration(env, forced_actions=forced, start_positions=start, sample_actions=True)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            del env
            return ms, float(m["loss"]), int(m["steps"])

        kinds = ["plain", "materialize", "views"]
        times = {k: [] for k in kinds}
        loss = {}
        for i in range(args.warmup + args.iters):
            order = kinds[i % 3:] + kinds[:i % 3]
            for kind in order:
                with Limit(lim):
                    ms, loss[kind], steps = one(kind)
                assert steps == T
                if i >= args.warmup:
                    times[kind].append(ms)
            torch.cuda.empty_cache()
        for k in kinds:
            out[f"{dt}_{k}_ms"] = round(statistics.median(times[k]), 2)
            out[f"{dt}_{k}_ms_all"] = [round(t, 1) for t in times[k]]
            out[f"{dt}_{k}_loss"] = loss[k]
        out[f"{dt}_views_minus_plain_ms"] = round(out[f"{dt}_views_ms"] - out[f"{dt}_plain_ms"], 2)
        out[f"{dt}_views_vs_materialize"] = round(out[f"{dt}_views_ms"] / out[f"{dt}_materialize_ms"] - 1.0, 4)
        del src
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
