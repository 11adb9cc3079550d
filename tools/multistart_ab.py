#!/usr/bin/env python3
"""What running the multistart evaluation as one ragged batch with device metrics buys
``SupervisedTrainer.eval_envs_on_images``, on the 64-image workload of tools/eval_ab.py (configs[2] topology, uint8 images
with sides of 3 - 10 patches of 448 px, T = 20, greedy, detection on, K = 2 starts) on one GPU, in one process.  Two
settings of the same call, each warmed up once, then repeats that alternate between them:

  loop      ``eval_envs_on_images(batch_size=1, device_metrics=False)``: one image at a time (its K walks as 2 agents),
            the pooling, NMS and mAP per image in Python — the form of the reference's ``eval_envs``
  batch     ``eval_envs_on_images(batch_size=64 // K, device_metrics=True)``: 32 images x K walks per rollout,
            jn_pool_walk_detections, jn_match_detections, jn_average_precision_segments per chunk

Prints ONE JSON line: images / s of every run and their medians — WHOLE-CALL rates (env construction, rollouts, teacher
grids, metrics), not kernel figures; whether both settings visited the same positions and reported the same values
(`map*` within 1e-6, every other key identical); and for one chunk, under device events, the K pool launches and the
match + segmented-AP launches, with the pool sizes they met.  With many boxes per patch (``--conf-threshold 1e-5``) the
loop takes long: ``--loop-images N`` times BOTH settings on the first N images.  Every GPU step runs under a hard time
limit.

    python tools/multistart_ab.py [--images 64] [--starts 2] [--conf-threshold 0.5] [--loop-images N] [--repeats 3]
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
    ap.add_argument("--starts", type=int, default=2)
    ap.add_argument("--patch-size", type=int, default=448)
    ap.add_argument("--seq-len", type=int, default=20)
    ap.add_argument("--min-side", type=int, default=3)
    ap.add_argument("--max-side", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--conf-threshold", type=float, default=0.5, help="detector confidence threshold (0.5 is the config's)")
    ap.add_argument("--loop-images", type=int, default=None, help="time both settings on the first N images only")
    args = ap.parse_args()

    import jolineedle_amd as ja
    from jolineedle_amd import detection
    from jolineedle_amd.config import model_config

    assert torch.cuda.is_available(), "multistart_ab needs the GPU"
    dev = torch.device("cuda:0")
    P, T, K, lim = args.patch_size, args.seq_len, args.starts, args.step_timeout
    N = args.images if args.loop_images is None else min(args.images, args.loop_images)
    out = {"tool": "multistart_ab", "images": N, "starts": K, "patch_size": P, "seq_len": T, "conf_threshold": args.conf_threshold,
           "note": "images_per_s are whole-call rates of eval_envs_on_images, not kernel figures"}

    with Limit(lim):
        images, boxes = make_workload(args.images, P, args.min_side, args.max_side, args.seed)
        images, boxes = [im.to(dev) for im in images[:N]], boxes[:N]
        model = ja.GPT(model_config(patch_size=P, block_size=T, detector_conf_threshold=args.conf_threshold), max_batch=64, device=dev)
        model.eval()
        model.sync_weights()
        cfg = ja.CfgNode(patch_size=P, max_seq_len=T, test_max_seq_len=T, stop_enabled=True, seed=args.seed, detection_enabled=True)
        trainer = ja.SupervisedTrainer(cfg, model)
        torch.cuda.synchronize()
    bs = max(1, min(64 // K, N))
    out["batch_size"] = bs

    def one(batched):
        trainer._eval_runner()._rollouts = 0               # every call draws the same start positions
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = trainer.eval_envs_on_images(images, boxes, batch_size=bs if batched else 1, n_starts=K, device_metrics=batched)
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0), m, [w["positions"] for w in trainer.last_eval_rollouts], trainer.last_eval_pool_stats

    settings = [("loop", False), ("batch", True)]
    metrics, walks, stats, rates = {}, {}, {}, {name: [] for name, _ in settings}
    for name, b in settings:                               # warm-up: every setting once
        with Limit(lim):
            rate, metrics[name], walks[name], stats[name] = one(b)
        print(f"warm-up {name}: {rate:.3f} images/s", file=sys.stderr, flush=True)
    for r in range(args.repeats):
        for name, b in (settings if r % 2 == 0 else settings[::-1]):
            with Limit(lim):
                rate = one(b)[0]
            rates[name].append(rate)
            print(f"run {r} {name}: {rate:.3f} images/s", file=sys.stderr, flush=True)
    for name, _ in settings:
        out[f"{name}_images_per_s"] = round(statistics.median(rates[name]), 3)
        out[f"{name}_images_per_s_all"] = [round(v, 3) for v in rates[name]]
    out["slowest_batch_over_fastest_loop"] = round(min(rates["batch"]) / max(rates["loop"]), 2)
    h, d = metrics["loop"], metrics["batch"]
    out["same_positions"] = len(walks["loop"]) == len(walks["batch"]) and all(torch.equal(a, b) for a, b in zip(walks["loop"], walks["batch"]))
    out["same_keys"] = list(h) == list(d)
    maps = [k for k in h if k.startswith("map")]
    out["map_max_difference"] = max(abs(a - b) for k in maps for a, b in zip(h[k], d[k]))
    out["other_keys_identical"] = all(a == b for k in h if k not in maps for a, b in zip(h[k], d[k]))
    out["values_agree"] = bool(out["same_keys"] and out["map_max_difference"] <= 1e-6 and out["other_keys_identical"])
    out["map_mean"] = {k: round(sum(d[k]) / len(d[k]), 6) for k in maps}
    pools = torch.cat([s[-1, ..., 0].flatten() for s in stats["batch"]])                # k = K: pool sizes per (image, cell)
    surv = torch.cat([s[-1, ..., 1].flatten() for s in stats["batch"]])
    out["pool_boxes_per_visited_cell"] = {"max": int(pools.max()), "sum": int(pools.sum()), "survivors_max": int(surv.max()),
                                           "survivors_sum": int(surv.sum())}

    # one chunk's evaluation launches under device events, as eval_envs_on_images issues them
    with Limit(lim):
        trainer._eval_runner()._rollouts = 0
        seen = list(trainer._eval_walks(images[:bs], boxes[:bs], bs, True, walks=K))[-1]
        ro, env = seen["rollout"], seen["env"]
        grid = (env.n_vertical_patches, env.n_horizontal_patches)
        tokens = torch.tensor([s + 1 for s in seen["steps"]], dtype=torch.int32, device=dev)
        first = torch.arange(bs, dtype=torch.int32, device=dev) * K
        counts = [torch.full((bs,), k, dtype=torch.int32, device=dev) for k in range(1, K + 1)]
        tg, tc = detection.cell_targets(boxes[:bs], seen["extents"][::K], grid, P, device=dev)
        tcells = seen["targets"][::K].reshape(bs, -1).bool()
        M = int(getattr(cfg, "eval_max_per_cell", 64))
        n_tok = max(seen["steps"]) + 1
        det = [ro[name][:, :n_tok] for name in ("det_boxes", "det_counts", "positions")]      # in place, as the method reads them
        pool_ms, score_ms = [], []
        for _ in range(1 + args.repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            pools_k = [detection.pool_walk_detections_device(*det, tokens, first, c, k + 1, grid, M) for k, c in enumerate(counts)]
            ev[1].record()
            maps_k = [detection.walk_cell_maps_device(p, tg, tc, tcells) for p in pools_k]
            ev[2].record()
            torch.cuda.synchronize()
            pool_ms.append(ev[0].elapsed_time(ev[1]))
            score_ms.append(ev[1].elapsed_time(ev[2]))
        out["chunk"] = {"images": bs, "walks": bs * K, "canvas_grid": list(grid), "pool_launches": K,
                        "pool_ms": round(statistics.median(pool_ms[1:]), 4),
                        "match_ap_launches": 4 * K, "match_ap_ms": round(statistics.median(score_ms[1:]), 4),
                        "map_traj_mean": float(maps_k[-1][0].mean()), "map_mean": float(maps_k[-1][1].mean())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
