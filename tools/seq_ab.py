#!/usr/bin/env python3
"""What sequence token positions and the in-rollout teacher cost, at the inference workload of ``bench.py --mode rollout``
(B = 64, T = 20, 448 px, 10 x 10 grid, forced actions, no detector) on one GPU, in one process.

Three kinds of the same rollout, interleaved (the order rotates from round to round):
  recurrent          every token at 1-D position 0 (the default; neither new engine call is made)
  sequence           token_positions="sequence" (jn_set_rollout_positions)
  sequence_teacher   the same with teacher=True (jn_set_rollout_teacher: one small launch per step)

Prints ONE JSON line: per kind the device time of the rollout from ``jn_last_timing(0)`` (HIP events on the rollout's
stream, env reset to epilogue) of every run, its median and spread (max - min), and the teacher sets' checksum.
Every GPU step runs under a hard time limit: past it the process dumps its stacks and exits.

    python tools/seq_ab.py [--runs 7] [--warmup 2] [--step-timeout 300]
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

KINDS = {"recurrent": dict(token_positions="recurrent"), "sequence": dict(token_positions="sequence"),
         "sequence_teacher": dict(token_positions="sequence", teacher=True)}


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
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs of each kind"

    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    from bench import synth_inputs

    assert torch.cuda.is_available(), "seq_ab needs the GPU"
    dev = torch.device("cuda:0")
    B, T, P, G = args.batch, args.seq_len, args.patch_size, args.grid
    lim = args.step_timeout
    out = {"tool": "seq_ab", "batch": B, "seq_len": T, "patch_size": P, "grid": G, "runs": args.runs}
    with Limit(lim):
        torch.manual_seed(12345)
        model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None), max_batch=B,
                       device=dev)
        model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345)
        trainer = ja.ReinforceTrainer(cfg, model)
        images, bboxes, start = synth_inputs(B, G, P, 12345, dev)
        forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(777)).to(dev)
        eng = model.engine()
        torch.cuda.synchronize()

    def one(kind):
        env = ja.NeedleGeneralEnv(images, bboxes, P, T, 1, True, engine=eng)
        ro = trainer.rollout(env, forced_actions=forced, start_positions=start, keep_patches=False, **KINDS[kind])
        ms = C.c_float()
        assert eng.lib.jn_last_timing(eng.handle, 0, C.byref(ms)) == 0       # synchronises
        assert ro["rewards"].shape[1] == T
        return ms.value, ro

    times = {k: [] for k in KINDS}
    names = list(KINDS)
    for i in range(args.warmup + args.runs):
        for kind in names[i % 3:] + names[:i % 3]:
            with Limit(lim):
                ms, ro = one(kind)
            if i >= args.warmup:
                times[kind].append(ms)
            if kind == "sequence_teacher":
                out["teacher_sets_nonzero"] = int((ro["teacher_sets"] != 0).sum())
                out["teacher_sets_sum"] = int(ro["teacher_sets"].sum(dtype=torch.int64))
    for kind, v in times.items():
        out[f"rollout_ms_{kind}"] = round(statistics.median(v), 3)
        out[f"rollout_ms_{kind}_spread"] = round(max(v) - min(v), 3)
        out[f"rollout_ms_{kind}_all"] = [round(t, 3) for t in v]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
