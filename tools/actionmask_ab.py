#!/usr/bin/env python3
"""What invalid-action masking (``rollout(action_mask=...)``) changes on the workload of ``bench.py --mode rollout`` (B = 64, 448 px
patches on a 10 x 10 grid, T = 20, the benchmark's model, images and start positions), on one GPU, in one process: sampled and greedy
walks under the three policies (none, "grid", "unvisited"), the six variants interleaved and their order rotated from round to round.

Prints ONE JSON line (and writes it to --out), per variant "<mode>/<policy>":
  clamped_share     share of the executed steps of live agents whose move was altered by the env's clamp (a non-STOP action whose
                    position change is not its delta)
  revisit_share     share of those steps that landed on a cell the walk had already visited (STOP steps count as landing where they
                    stand)
  steps             executed glimpse steps S of the batch (median)
  device_ms         device time of one rollout (the engine's own events around it, ``jn_last_timing``): median of --iters (7) runs
  device_ms_spread  max - min of those runs
The shares of a sampled variant are means over the runs (every run draws other walks); a greedy variant walks the same way every run.

Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/actionmask_ab.py [--iters 7] [--warmup 2] [--out profiles/actionmask_ab.json] [--step-timeout 300]
"""
import argparse
import ctypes as C
import faulthandler
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DY = (0, 0, -1, 1, -1, -1, 1, 1, 0)
DX = (-1, 1, 0, 0, -1, 1, -1, 1, 0)
POLICIES = (None, "grid", "unvisited")


class Limit:
    """Hard per-step time limit: faulthandler's watchdog thread exits the process even when a GPU call never returns."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def walk_shares(ro, G):
    """(clamped steps, revisiting steps, counted steps) of a rollout, on the device: the steps of agents still alive when they
    decide (logit_masks)."""
    pos, act, live = ro["positions"], ro["actions"], ro["logit_masks"]
    B, S = act.shape
    dy, dx = torch.tensor(DY, device=act.device)[act], torch.tensor(DX, device=act.device)[act]
    moved = pos[:, 1:] - pos[:, :-1]
    clamped = ((moved[..., 0] != dy) | (moved[..., 1] != dx)) & live
    cell = pos[..., 0] * G + pos[..., 1]                                              # [B, S + 1]
    earlier = torch.ones((S + 1, S + 1), device=act.device, dtype=torch.bool).tril(-1)      # [t, k]: k < t
    seen = ((cell[:, :, None] == cell[:, None, :]) & earlier[None]).any(-1)           # cell t was visited at some k < t
    revisit = seen[:, 1:] & live
    return int(clamped.sum()), int(revisit.sum()), int(live.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "actionmask_ab.json"))
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()

    import jolineedle_amd as ja
    from bench import synth_inputs
    from jolineedle_amd.config import model_config

    assert torch.cuda.is_available(), "actionmask_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, P, G, T, lim = args.batch, args.patch_size, args.grid, args.seq_len, args.step_timeout
    out = {"tool": "actionmask_ab", "batch": B, "patch_size": P, "grid": G, "seq_len": T, "iters": args.iters}
    torch.manual_seed(12345)
    with Limit(lim):
        model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None), max_batch=B, device="cuda:0")
        model.sync_weights()
        model.eval()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345)
        trainer = ja.ReinforceTrainer(cfg, model)
        images, bboxes, start = synth_inputs(B, G, P, 12345, dev)
        eng = model.engine()
        torch.cuda.synchronize()

    variants = [(mode, pol) for mode in ("sample", "greedy") for pol in POLICIES]
    runs = {v: [] for v in variants}

    @torch.no_grad()
    def one(mode, pol):
        env = ja.NeedleGeneralEnv(images, bboxes, P, T, 1, True, engine=eng)
        ro = trainer.rollout(env, sample_actions=mode == "sample", start_positions=start, keep_patches=False, action_mask=pol)
        ms = C.c_float()
        eng.lib.jn_last_timing(eng.handle, 0, C.byref(ms))
        return (ms.value, int(ro["actions"].shape[1])) + walk_shares(ro, G)

    for i in range(args.warmup + args.iters):
        k = i % len(variants)
        for v in variants[k:] + variants[:k]:
            with Limit(lim):
                r = one(*v)
            if i >= args.warmup:
                runs[v].append(r)

    for (mode, pol), rs in runs.items():
        ms = [r[0] for r in rs]
        counted = sum(r[4] for r in rs)
        out[f"{mode}/{pol or 'none'}"] = {
            "clamped_share": round(sum(r[2] for r in rs) / counted, 4), "revisit_share": round(sum(r[3] for r in rs) / counted, 4),
            "steps": statistics.median(r[1] for r in rs), "device_ms": round(statistics.median(ms), 3),
            "device_ms_spread": round(max(ms) - min(ms), 3), "device_ms_all": [round(m, 3) for m in ms]}

    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
