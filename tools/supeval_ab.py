#!/usr/bin/env python3
"""What the teacher-forced validation costs on one GPU.  Three measurements, each in a child process of its own under a
time limit (the parent never opens the GPU; after a child that did not end cleanly nothing more is started):

  supervised   ``SupervisedTrainer.eval_step`` (jn_supervised_eval: the B*T patches in chunks of max_batch, loss and
               accuracy in one kernel) against the path the package offered before for the same numbers — ``GPT.forward``
               in eval mode (T conv-stack passes of B patches) followed by ``compute_metrics`` in torch — interleaved,
               device events, at B = 4, T = 8 (BASELINE configs[0]; max_batch 32, what its training step needs) and at
               B = 16, T = 20, max_batch 64; 448 px, gpt-nano + yolox-nano encoder, synthetic patches.  The logits of
               the two paths are compared (bar 2e-4).
  detector     ``NeedleYOLOX.validation_loss`` (jn_detector_eval_loss: eval-mode PAFPN, train-mode head, SimOTA loss,
               eval head + NMS) on 18 and on 64 patches of 448 px, yolox-s, max_batch 64; beside it the train-mode loss
               branch under no_grad (what the same call cost before, with the numbers of another route).
  end_to_end   ``eval_supervised_on_images`` on 16 synthetic images of 4 x 4 patches, batches of 8, T = 20: images / s of
               the WHOLE call (teacher walks on the host, gathers, both engines, one readback per batch).

Prints ONE JSON line with the medians and spreads (max - min) of at least five runs after warm-up.

    python tools/supeval_ab.py [--runs 7] [--warmup 2] [--step-timeout 240] [--out profiles/supeval_ab.json]
"""
import argparse
import faulthandler
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SECTIONS = ("supervised", "detector", "end_to_end")
P = 448


class Limit:
    """Hard per-step time limit: faulthandler's watchdog thread exits the process even when a GPU call never returns."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def _summary(out, key, values):
    out[key] = round(statistics.median(values), 3)
    out[key + "_spread"] = round(max(values) - min(values), 3)
    out[key + "_all"] = [round(v, 3) for v in values]


def _timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), res


def section_supervised(args, torch, ja, model_config):
    dev = torch.device("cuda:0")
    out = {}
    for B, T, MB in ((4, 8, 32), (16, 20, 64)):
        tag = f"B{B}_T{T}"
        with Limit(args.step_timeout):
            torch.manual_seed(12345)
            model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None), max_batch=MB, device=dev)
            model.eval()
            model.sync_weights()
            trainer = ja.SupervisedTrainer(ja.CfgNode(stop_enabled=True, stop_weight=2.0, loss_mode="best-action"), model)
            g = torch.Generator().manual_seed(7)
            patches = torch.rand((B, T, 3, P, P), generator=g).to(dev)
            cur, nxt = (torch.randint(0, 9, (B, T), generator=g).to(dev) for _ in range(2))
            positions = torch.randint(0, 5, (B, T, 2), generator=g).to(dev)
            masks = (torch.arange(T)[None] < torch.randint(1, T + 1, (B, 1), generator=g)).float().to(dev)
            classes = torch.zeros(B, dtype=torch.long, device=dev)
            torch.cuda.synchronize()

        def new():
            return trainer.eval_step(patches, cur, nxt, positions, masks, classes=classes)

        def old():
            with torch.no_grad():
                logits, _ = model(patches, cur, classes, positions)
                return trainer.compute_metrics(logits, nxt, masks), logits

        times = {"new": [], "old": []}
        for i in range(args.warmup + args.runs):
            for name, fn in ((("new", new), ("old", old)) if i % 2 == 0 else (("old", old), ("new", new))):
                with Limit(args.step_timeout):
                    ms, res = _timed(torch, fn)
                print(f"supervised {tag} run {i} {name}: {ms:.3f} ms", file=sys.stderr, flush=True)
                if i >= args.warmup:
                    times[name].append(ms)
                if name == "new":
                    got = res
                else:
                    ref_metrics, ref_logits = res
        out[tag] = {"B": B, "T": T, "max_batch": MB, "conv_stack_passes_new": -(-B * T // MB), "conv_stack_passes_old": T}
        _summary(out[tag], "eval_step_ms", times["new"])
        _summary(out[tag], "forward_plus_torch_metrics_ms", times["old"])
        out[tag]["logits_max_difference"] = float((got["logits"] - ref_logits).abs().max())
        out[tag]["logits_agree"] = out[tag]["logits_max_difference"] < 2e-4
        out[tag]["action_loss"] = [float(got["metrics"][0]), float(ref_metrics["action_loss"])]
        out[tag]["action_accuracy"] = [float(got["metrics"][1]), float(ref_metrics["action_accuracy"])]
        out[tag]["faster"] = out[tag]["eval_step_ms"] < out[tag]["forward_plus_torch_metrics_ms"]
        del model, trainer, patches
        torch.cuda.empty_cache()
    return out


def section_detector(args, torch, ja, model_config):
    dev = torch.device("cuda:0")
    out = {}
    with Limit(args.step_timeout):
        torch.manual_seed(12345)
        model = ja.GPT(model_config(patch_size=P, block_size=4), max_batch=64, device=dev)
        model.eval()
        model.sync_weights()
    for N in (18, 64):
        g = torch.Generator().manual_seed(N)
        x = torch.rand((N, 3, P, P), generator=g).to(dev)
        tg = torch.zeros((N, 3, 5), device=dev)
        tg[::2, 0] = torch.tensor([0, 40., 60., 200., 260.], device=dev)
        tg[::3, 1] = torch.tensor([0, 250., 100., 400., 300.], device=dev)

        def new():
            with torch.no_grad():
                return model.yolox.validation_loss(x, tg, packed=True)[2]

        def old():
            model.train()
            with torch.no_grad():
                losses = model.yolox(x, tg)[2]
            model.eval()
            return losses

        times = {"new": [], "old": []}
        for i in range(args.warmup + args.runs):
            for name, fn in ((("new", new), ("old", old)) if i % 2 == 0 else (("old", old), ("new", new))):
                with Limit(args.step_timeout):
                    ms, res = _timed(torch, fn)
                print(f"detector N={N} run {i} {name}: {ms:.3f} ms", file=sys.stderr, flush=True)
                if i >= args.warmup:
                    times[name].append(ms)
                if name == "new":
                    total_new = float(res["total_loss"])
                else:
                    total_old = float(res["total_loss"])
        out[f"N{N}"] = {"patches": N, "total_loss_validation_route": total_new, "total_loss_train_mode_backbone": total_old}
        _summary(out[f"N{N}"], "validation_loss_ms", times["new"])
        _summary(out[f"N{N}"], "train_mode_loss_branch_ms", times["old"])
    return out


def section_end_to_end(args, torch, ja, model_config):
    import time
    dev = torch.device("cuda:0")
    n_img, G, T, bs = 16, 4, 20, 8
    with Limit(args.step_timeout):
        torch.manual_seed(12345)
        model = ja.GPT(model_config(patch_size=P, block_size=T), max_batch=64, device=dev)
        model.eval()
        model.sync_weights()
        cfg = ja.CfgNode(patch_size=P, max_seq_len=T, stop_enabled=True, stop_weight=2.0, seed=0, detection_enabled=True,
                         loss_mode="best-action")
        trainer = ja.SupervisedTrainer(cfg, model)
        g = torch.Generator().manual_seed(5)
        images = torch.rand((n_img, 3, G * P, G * P), generator=g).to(dev)
        bboxes = torch.zeros((n_img, 2, 4), dtype=torch.long)
        for i in range(n_img):
            for k in range(2):
                x0, y0 = (int(v) for v in torch.randint(0, G * P - 300, (2,), generator=g))
                w, h = (int(v) for v in torch.randint(60, 300, (2,), generator=g))
                bboxes[i, k] = torch.tensor([x0, y0, x0 + w, y0 + h])
        torch.cuda.synchronize()
    rates = []
    for i in range(args.warmup + args.runs):
        with Limit(args.step_timeout):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = trainer.eval_supervised_on_images(images, bboxes, bs, seed=100)
            torch.cuda.synchronize()
            rate = n_img / (time.perf_counter() - t0)
            print(f"end_to_end run {i}: {rate:.3f} images/s", file=sys.stderr, flush=True)
            if i >= args.warmup:
                rates.append(rate)
    out = {"images": n_img, "grid": G, "seq_len": T, "batch_size": bs, "note": "whole-call rate, host walks included",
           "detector_patches_per_batch": [int(k["trajectories"]["patches_yolox"].shape[0]) for k in trainer.last_eval_supervised],
           "action_loss": m["action_loss"], "yolo_total_loss": m["yolo_total_loss"], "map": m["map"]}
    _summary(out, "images_per_s", rates)
    return out


def child(args):
    import torch
    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    assert torch.cuda.is_available(), "supeval_ab needs the GPU"
    fn = {"supervised": section_supervised, "detector": section_detector, "end_to_end": section_end_to_end}[args.section]
    print("RESULT " + json.dumps(fn(args, torch, ja, model_config)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--section-timeout", type=float, default=360.0, help="time limit of one child process")
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=SECTIONS)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    ap.add_argument("--section", type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs of each kind"
    if args.section:
        return child(args)
    out = {"tool": "supeval_ab", "patch_size": P, "runs": args.runs, "warmup": args.warmup}
    for name in args.sections:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--section", name, "--runs", str(args.runs), "--warmup", str(args.warmup),
               "--step-timeout", str(args.step_timeout)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.section_timeout)     # stderr: passed on
            rc, text, err = res.returncode, res.stdout, ""
        except subprocess.TimeoutExpired as e:
            rc, text, err = 124, "", str(e)
        print(f"section {name}: exit code {rc}", file=sys.stderr, flush=True)
        line = next((ln for ln in text.splitlines() if ln.startswith("RESULT ")), None)
        if rc != 0 or line is None:
            out[name] = {"failed": True, "exit_code": rc, "note": err[-500:]}
            out["stopped_after"] = name                     # nothing more is started on the GPU after a child that failed
            break
        out[name] = json.loads(line[len("RESULT "):])
    text = json.dumps(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)
    return 1 if "stopped_after" in out else 0


if __name__ == "__main__":
    sys.exit(main())
