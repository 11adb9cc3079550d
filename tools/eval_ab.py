#!/usr/bin/env python3
"""What evaluating the detections on the device buys ``eval_on_images``, on the 64-image workload of tools/infer_ab.py
(configs[2] topology, uint8 images with sides of 3 - 10 patches of 448 px, T = 20, greedy, detection on,
``merge_bboxes=True``, one chunk of 64) on one GPU, in one process.  Two settings of the same call, each warmed up once,
then repeats that alternate between them:

  host      ``eval_on_images(device_metrics=False)``: merge_boxes and map_50 per image in Python
  device    ``eval_on_images(device_metrics=True)``:  jn_merge_boxes, jn_match_detections, jn_average_precision per chunk

Prints ONE JSON line: images / s of every run and their medians — WHOLE-CALL rates (env construction, rollout, box
assembly, the per-image detector pass of the `yolo_*` keys and the bookkeeping), not kernel figures; whether the two
settings report the same metrics (`map` within 1e-6, every other key identical); and for the chunk, under device
events, the merge launches (predictions and targets) and the match + average-precision launches, with the boxes per
image and the relaxation rounds the merge took.  With many boxes per image (``--conf-threshold 1e-5``) the host path
takes minutes per chunk: ``--host-images K`` times BOTH settings on the first K images and the device setting on all
of them as well; rates are per image either way.  Every GPU step runs under a hard time limit.

    python tools/eval_ab.py [--images 64] [--conf-threshold 0.5] [--host-images K] [--host-repeats R] [--repeats 3]
                            [--step-timeout 300]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from infer_ab import Limit, make_workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--min-side", type=int, default=3)
    ap.add_argument("--max-side", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--conf-threshold", type=float, default=0.5, help="detector confidence threshold (0.5 is the config's)")
    ap.add_argument("--host-images", type=int, default=None, help="time the host setting on the first K images only")
    ap.add_argument("--host-repeats", type=int, default=None, help="timed runs of the host setting (default: --repeats)")
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import detection, ragged
    from jolineedle_amd.config import model_config

    assert torch.cuda.is_available(), "eval_ab needs the GPU"
    dev = torch.device("cuda:0")
    N, P, T, lim = args.images, args.patch_size, args.seq_len, args.step_timeout
    K = N if args.host_images is None else min(N, args.host_images)
    out = {"tool": "eval_ab", "images": N, "host_images": K, "patch_size": P, "seq_len": T, "conf_threshold": args.conf_threshold,
           "note": "images_per_s are whole-call rates of eval_on_images, not kernel figures"}

    with Limit(lim):
        images, boxes = make_workload(N, P, args.min_side, args.max_side, args.seed)
        images = [im.to(dev) for im in images]
        model = ja.GPT(model_config(patch_size=P, block_size=T, detector_conf_threshold=args.conf_threshold), max_batch=max(64, N), device=dev)
        model.eval()
        model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=False, seed=args.seed,
                         patch_size=P, detection_enabled=True, merge_bboxes=True)
        trainer = ja.ReinforceTrainer(cfg, model)
        torch.cuda.synchronize()

    def one(device_metrics, n):
        trainer._rollouts = 0                      # every call draws the same start positions
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = trainer.eval_on_images(images[:n], boxes[:n], batch_size=min(64, n), do_detection=True, merge_bboxes=True,
                                   device_metrics=device_metrics)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), m

    settings = [("host", False, K), ("device", True, K)] + ([("device_all", True, N)] if K < N else [])
    metrics, rates = {}, {name: [] for name, _, _ in settings}
    host_repeats = args.repeats if args.host_repeats is None else args.host_repeats
    out["host_repeats"] = host_repeats
    for name, dm, n in settings:                   # warm-up: every setting once
        with Limit(lim):
            rate, metrics[name] = one(dm, n)
        print(f"warm-up {name}: {rate:.3f} images/s", file=sys.stderr, flush=True)
    for r in range(args.repeats):
        for name, dm, n in (settings if r % 2 == 0 else settings[::-1]):
            if name == "host" and r >= host_repeats:
                continue
            with Limit(lim):
                rate, _ = one(dm, n)
            rates[name].append(rate)
            print(f"run {r} {name}: {rate:.3f} images/s", file=sys.stderr, flush=True)
    for name, _, _ in settings:
        out[f"{name}_images_per_s"] = round(statistics.median(rates[name]), 3)
        out[f"{name}_images_per_s_all"] = [round(v, 3) for v in rates[name]]
    out["slowest_device_over_fastest_host"] = round(min(rates["device"]) / max(rates["host"]), 2)
    h, d = metrics["host"], metrics["device"]
    out["same_keys"] = list(h) == list(d)
    out["map_max_difference"] = max(abs(a - b) for a, b in zip(h["map"], d["map"]))
    out["other_keys_identical"] = all(a == b or (a != a and b != b) for k in h if k != "map" for a, b in zip(h[k], d[k]))
    out["metrics_agree"] = bool(out["same_keys"] and out["map_max_difference"] <= 1e-6 and out["other_keys_identical"])
    out["map_mean_host"], out["map_mean_device"] = sum(h["map"]) / len(h["map"]), sum(d["map"]) / len(d["map"])

    # the chunk's evaluation launches under device events: the first min(64, N) images as eval_on_images runs them
    with Limit(lim):
        n = min(64, N)
        env = ragged.image_env(trainer, images[:n], boxes[:n])
        extents = env.grid_extents.tolist()
        ro = trainer.rollout(env, do_detection=True, sample_actions=False, bbox_lists=False,
                             start_positions=ragged.loop_start_positions(trainer, 1, list(range(n)), extents))
        packed = detection.rollout_boxes_packed(ro, P)
        tg = detection.pack_boxes([detection.detection_targets(boxes[b].unsqueeze(0), *extents[b], P)[0] for b in range(n)], 5, dev)
        merge_ms, match_ms = [], []
        for _ in range(1 + args.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            pm, pc, rounds = detection.merge_boxes_device(*packed, return_rounds=True)
            tm = detection.merge_boxes_device(*tg, target=True)
            ev[1].record()
            ap = detection.average_precision_device(detection.match_detections_device((pm, pc), tm), pooled=False)
            ev[2].record()
            torch.cuda.synchronize()
            merge_ms.append(ev[0].elapsed_time(ev[1]))
            match_ms.append(ev[1].elapsed_time(ev[2]))
        counts = packed[1].tolist()
        out["chunk_boxes_per_image"] = {"min": min(counts), "mean": round(sum(counts) / n, 1), "max": max(counts)}
        out["chunk_merged_per_image_mean"] = round(float(pc.float().mean()), 1)
        out["chunk_relaxation_rounds"] = {"max": int(rounds.max()), "mean": round(float(rounds.float().mean()), 2)}
        out["chunk_merge_ms"] = round(statistics.median(merge_ms[1:]), 4)
        out["chunk_match_ap_ms"] = round(statistics.median(match_ms[1:]), 4)
        out["chunk_map_mean"] = float(ap.mean())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
