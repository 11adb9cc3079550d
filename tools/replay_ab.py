#!/usr/bin/env python3
"""What activation replay (jn_set_activation_slots) costs on one GPU.  Two measurements, each in a child
process of its own under a time limit (the parent never opens the GPU; after a child that did not end cleanly nothing
more is started):

  headline   the headline workload (B = 64, T = 20, 448 px, gpt-nano + yolox-nano encoder, fp32, forced non-STOP actions)
             under n = 0 (every step resident), n = 5 and n = 1: one model per setting, the same images, iterations
             interleaved; a whole iteration = train-mode rollout + loss + backward (``train_iteration`` without the
             optimiser step) between two device events.  Beside each: what the encoder's workspace holds
             (``GPT.activation_slots_info``) and the bytes of its activation slots.
  long_walk  T = 128 at B = 64 under n = 8, the ring only: the default would need 129 activation slots and as many
             gradient mirrors (about 490 GB) and is not attempted.

Prints ONE JSON line: medians of the runs after warm-up with their spread (max - min).

    python tools/replay_ab.py [--runs 7] [--warmup 2] [--out profiles/replay_ab.json]
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

SECTIONS = ("headline", "long_walk")
P, B = 448, 64


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


class Setting:
    """One model under activation_slots = n with its trainer; ``iteration`` returns device ms of a whole iteration."""

    def __init__(self, torch, ja, model_config, n, T, images, bboxes, start, forced):
        self.torch, self.ja, self.n, self.T = torch, ja, n, T
        self.inputs = (images, bboxes, start, forced)
        torch.manual_seed(12345)
        self.model = ja.GPT(model_config(patch_size=P, block_size=T, with_detector=False, image_processor=None, activation_slots=n),
                            max_batch=B, device="cuda:0")
        self.model.sync_weights()
        cfg = ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345, learning_rate=1e-4,
                         gradient_accumulation=1)
        self.trainer = ja.ReinforceTrainer(cfg, self.model)

    def iteration(self):
        torch, ja = self.torch, self.ja
        images, bboxes, start, forced = self.inputs
        eng = self.model.engine()
        env = ja.NeedleGeneralEnv(images, bboxes, P, self.T, 1, True, engine=eng)
        eng.lib.jn_zero_grad(eng.handle, None)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m = self.trainer.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
        b.record()
        torch.cuda.synchronize()
        assert m["steps"] == self.T and float(m["loss"]) == float(m["loss"]), m
        return a.elapsed_time(b), float(m["loss"])

    def report(self, times, loss):
        info = self.model.activation_slots_info()
        out = {"activation_slots": self.n, "T": self.T, "B": B, "loss": loss, **info,
               "activation_bytes": info["act_slots"] * info["slot_bytes"]}
        _summary(out, "iteration_ms", times)
        return out


def _inputs(torch, T, G):
    dev = torch.device("cuda:0")
    images = torch.rand((B, 3, G * P, G * P), device=dev, generator=torch.Generator(device=dev).manual_seed(12345))
    g = torch.Generator().manual_seed(12345)
    bboxes = torch.zeros((B, 3, 4), dtype=torch.long)
    for b in range(B):
        for k in range(int(torch.randint(1, 4, (1,), generator=g))):
            w, h = (int(torch.randint(32, P, (1,), generator=g)) for _ in range(2))
            x, y = int(torch.randint(0, G * P - w, (1,), generator=g)), int(torch.randint(0, G * P - h, (1,), generator=g))
            bboxes[b, k] = torch.tensor([x, y, x + w, y + h])
    start = torch.randint(0, G, (B, 2), generator=g)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(777)).to(dev)
    return images, bboxes, start, forced


def section_headline(args, torch, ja, model_config):
    T = 20
    with Limit(args.step_timeout):
        inputs = _inputs(torch, T, args.grid)
        settings = [Setting(torch, ja, model_config, n, T, *inputs) for n in (0, 5, 1)]
    times, loss = {s.n: [] for s in settings}, {}
    for i in range(args.warmup + args.runs):
        for s in settings[i % 3:] + settings[:i % 3]:          # interleaved, the order rotating
            with Limit(args.step_timeout):
                ms, loss[s.n] = s.iteration()
            print(f"headline run {i} n={s.n}: {ms:.3f} ms", file=sys.stderr, flush=True)
            if i >= args.warmup:
                times[s.n].append(ms)
    out = {f"n{s.n}": s.report(times[s.n], loss[s.n]) for s in settings}
    base = out["n0"]["iteration_ms"]
    for s in settings[1:]:
        r = out[f"n{s.n}"]
        r["over_n0_ms"] = round(r["iteration_ms"] - base, 3)
        r["over_n0_ms_per_replayed_step"] = round((r["iteration_ms"] - base) / max(r["replayed_steps"], 1), 3)
    return out


def section_long_walk(args, torch, ja, model_config):
    T, n = 128, 8
    with Limit(args.step_timeout):
        s = Setting(torch, ja, model_config, n, T, *_inputs(torch, T, args.grid))
    times, loss = [], None
    for i in range(1 + args.long_runs):
        with Limit(args.step_timeout):
            ms, loss = s.iteration()
        print(f"long_walk run {i} n={n}: {ms:.3f} ms", file=sys.stderr, flush=True)
        if i >= 1:
            times.append(ms)
    out = s.report(times, loss)
    out["all_resident_would_hold_bytes"] = (T + 1) * out["slot_bytes"]
    out["ms_per_glimpse_step"] = round(out["iteration_ms"] / T, 3)
    return out


def child(args):
    import torch
    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    assert torch.cuda.is_available(), "replay_ab needs the GPU"
    fn = {"headline": section_headline, "long_walk": section_long_walk}[args.section]
    print("RESULT " + json.dumps(fn(args, torch, ja, model_config)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long-runs", type=int, default=3, help="timed iterations of the T = 128 walk (after one warm-up)")
    ap.add_argument("--grid", type=int, default=10, help="patches per image side (10: the headline's 4480 x 4480 images)")
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--section-timeout", type=float, default=300.0, help="time limit of one child process")
    ap.add_argument("--sections", nargs="+", default=list(SECTIONS), choices=SECTIONS)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    ap.add_argument("--section", type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs of each kind"
    if args.section:
        return child(args)
    out = {"tool": "replay_ab", "patch_size": P, "batch": B, "runs": args.runs, "warmup": args.warmup,
           "iteration": "train-mode rollout + loss + backward, no optimiser step, device events"}
    for name in args.sections:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--section", name, "--runs", str(args.runs), "--warmup", str(args.warmup),
               "--long-runs", str(args.long_runs), "--grid", str(args.grid), "--step-timeout", str(args.step_timeout)]
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
