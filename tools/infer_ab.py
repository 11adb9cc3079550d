#!/usr/bin/env python3
"""What batching buys ``infer_images`` on a test set of unequal sizes, at the configs[2] topology (gpt-nano, yolox-nano
patch encoder, yolox-s detector, 448 px patches) on one GPU, in one process.  The workload: 64 seeded uint8 images whose
sides are drawn between 3 and 10 patches (not all equal), a few boxes each, T = 20, greedy, detection on.  Three
settings of the same call, every shape warmed up once, then three repeats that alternate between them:

  loop       ``infer_images(batch_size=None)``: one B = 1 env and rollout per image, fp32 copy padded with F.pad
  batch16    ``infer_images(batch_size=16)``: chunks of 16 through image views, bytes read in place
  batch64    ``infer_images(batch_size=64)``: one chunk

Prints ONE JSON line: images / s of every run and their medians — WHOLE-CALL rates (env construction, rollout, box
assembly and the host-side bookkeeping of the call), not kernel figures; whether the three settings visited the same
positions; and for one 64-image chunk the split of its time into the rollout, the device box assembly
(``rollout_boxes_to_image``) and the Python list assembly it replaces (the B x (S+1) clone lists of ``rollout`` plus
``patch_bboxes2full_image`` on the same rollout outputs).  Every GPU step runs under a hard time limit: past it the
process dumps its stacks and exits.

    python tools/infer_ab.py [--images 64] [--min-side 3] [--max-side 10] [--repeats 3] [--step-timeout 300]
                             [--conf-threshold 0.5]
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


def make_workload(n_images: int, patch_size: int, min_side: int, max_side: int, seed: int, max_boxes: int = 3):
    """([uint8 [3, h, w]], [[n, 4] int64 xyxy]) on the CPU: h and w drawn independently in
    [min_side, max_side] * patch_size minus up to a patch (so that the padding differs from image to image), the first
    two images pinned to the smallest and the largest side so that the sizes are never all equal."""
    g = torch.Generator().manual_seed(seed)
    P = int(patch_size)
    images, boxes = [], []
    for i in range(n_images):
        sides = torch.randint(min_side, max_side + 1, (2,), generator=g).tolist()
        if i == 0:
            sides = [min_side, min_side]
        elif i == 1:
            sides = [max_side, max_side]
        h, w = (s * P - int(torch.randint(0, P, (1,), generator=g)) for s in sides)
        images.append(torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8))
        rows = []
        for _ in range(int(torch.randint(1, max_boxes + 1, (1,), generator=g))):
            bw, bh = (int(torch.randint(max(2, P // 8), P, (1,), generator=g)) for _ in range(2))
            x, y = int(torch.randint(0, max(1, w - bw), (1,), generator=g)), int(torch.randint(0, max(1, h - bh), (1,), generator=g))
            rows.append([x, y, min(x + bw, w - 1), min(y + bh, h - 1)])
        boxes.append(torch.tensor(rows, dtype=torch.int64))
    return images, boxes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--min-side", type=int, default=3, help="smallest image side in patches")
    ap.add_argument("--max-side", type=int, default=10, help="largest image side in patches")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--conf-threshold", type=float, default=0.5,
                    help="detector confidence threshold (0.5 is the config's; seeded weights clear it nowhere, so a "
                         "lower one puts boxes into the assembly that the split times)")
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import detection, ragged
    from jolineedle_amd.config import model_config

    assert torch.cuda.is_available(), "infer_ab needs the GPU"
    dev = torch.device("cuda:0")
    N, P, T, lim = args.images, args.patch_size, args.seq_len, args.step_timeout
    settings = [("loop", None), ("batch16", min(16, N)), ("batch64", min(64, N))]
    out = {"tool": "infer_ab", "images": N, "patch_size": P, "seq_len": T, "sides": [args.min_side, args.max_side],
           "conf_threshold": args.conf_threshold,
           "note": "images_per_s are whole-call rates of infer_images, not kernel figures"}

    with Limit(lim):
        images, boxes = make_workload(N, P, args.min_side, args.max_side, args.seed)
        images = [im.to(dev) for im in images]
        out["distinct_sizes"] = len({tuple(im.shape[1:]) for im in images})
        model = ja.GPT(model_config(patch_size=P, block_size=T, detector_conf_threshold=args.conf_threshold), max_batch=max(64, N), device=dev)
        model.eval()
        model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=False, seed=args.seed,
                         patch_size=P, detection_enabled=True)
        trainer = ja.ReinforceTrainer(cfg, model)
        torch.cuda.synchronize()

    def one(batch_size):
        trainer._rollouts = 0                      # every call draws the same start positions
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ja.infer_images(trainer, images, boxes, sample_actions=False, do_detection=True, batch_size=batch_size)
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0), res

    positions = {}
    for name, bs in settings:                      # warm-up: every shape once (allocations, first launches)
        with Limit(lim):
            _, res = one(bs)
        positions[name] = res["positions"]
    rates = {name: [] for name, _ in settings}
    for r in range(args.repeats):
        order = settings[r % 3:] + settings[:r % 3]
        for name, bs in order:
            with Limit(lim):
                rate, res = one(bs)
            rates[name].append(rate)
            same = all(torch.equal(a, b) for a, b in zip(res["positions"], positions[name]))
            assert same, f"{name}: two runs of one setting visited different positions"
    for name, _ in settings:
        out[f"{name}_images_per_s"] = round(statistics.median(rates[name]), 2)
        out[f"{name}_images_per_s_all"] = [round(v, 2) for v in rates[name]]
    out["same_positions"] = all(torch.equal(a, b) for name, _ in settings[1:]
                                for a, b in zip(positions[name], positions["loop"]))
    out["slowest_batch64_over_fastest_loop"] = round(min(rates["batch64"]) / max(rates["loop"]), 2)
    out["steps_total"] = int(sum(res["steps"]))

    # the split of one chunk: the first min(64, N) images as infer_images runs them
    with Limit(lim):
        n = min(64, N)
        rows = boxes[:n]
        split = {"rollout_ms": [], "device_boxes_ms": [], "python_boxes_ms": []}
        for _ in range(1 + args.repeats):
            env = ragged.image_env(trainer, images[:n], rows)
            start = ragged.loop_start_positions(trainer, 1, list(range(n)), env.grid_extents.tolist())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ro = trainer.rollout(env, do_detection=True, sample_actions=False, start_positions=start, bbox_lists=False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            full = detection.rollout_boxes_to_image(ro, P)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            cnt = ro["det_counts"].tolist()          # what rollout(bbox_lists=True) builds, then the reference's loop
            S1 = ro["det_counts"].shape[1]
            lists = [[ro["det_boxes"][b, t, :cnt[b][t]].clone() if cnt[b][t] > 0 else None for t in range(S1)] for b in range(n)]
            ref = detection.patch_bboxes2full_image(lists, ro["positions"][:, :, [1, 0]] * P, ro["masks"])
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for a, b in zip(full, ref):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
            for k, v in zip(split, (t1 - t0, t2 - t1, t3 - t2)):
                split[k].append(v * 1e3)
        for k, v in split.items():
            out["chunk_" + k] = round(statistics.median(v[1:]), 3)
        out["chunk_boxes"] = int(sum(0 if a is None else len(a) for a in full))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
