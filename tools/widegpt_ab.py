#!/usr/bin/env python3
"""What a decision step costs on the wide route (kernels_gptwide.hip: every Linear one skinny GEMM over all agents) on one
GPU.  Each model in a child process of its own under a time limit (the parent never opens the GPU; after a child that did
not end cleanly nothing more is started):

  gpt-mini      both routes, interleaved: the per-agent gpt_step_kernel (the default below n_embd 257) and the wide route
                (a second context created under JN_GPT_WIDE=1) on the same weights; their logits are compared (bar 1e-4).
  gopher-44m    wide route only, against the weight-stream floor: the block weights (12 L C^2 floats) read once per
  gpt2          step at the one-read-stream rate tools/streambench reports in the same session (its "1R1W" column at
                411 MB, in TB/s; build it first, see its head, or pass --stream-tbps).

Conditions: B = 64, T = 20, 64-px patches, yolox-nano encoder, eval mode; device events around one recurrent
``GPT.forward`` with 20 previous embeddings — a full-sequence decode of 21 tokens (20 given, 1 new) behind ONE encoder pass
of B patches.  That pass (``GPT.embed_patches`` on the same B patches: the same engine call sequence) is timed by itself
right after every forward and subtracted, run by run: ``*_us_per_step`` is the decode alone per decision step
((forward - encoder) / 21), ``*_forward_us_per_step`` the whole forward / 21, ``*_encoder_us`` the encoder pass; medians of
seven with (max - min).  The floor and the route-to-route ratio are taken on the decode alone.

Prints ONE JSON line.

    python tools/widegpt_ab.py [--runs 7] [--warmup 2] [--step-timeout 240] [--out profiles/widegpt_ab.json]
"""
import argparse
import faulthandler
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODELS = ("gpt-mini", "gopher-44m", "gpt2")
P, B, T = 64, 64, 20


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


def child(args):
    import torch
    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    from jolineedle_amd.engine import GPT_ZOO
    assert torch.cuda.is_available(), "widegpt_ab needs the GPU"
    dev = torch.device("cuda:0")
    name = args.model
    n_layer, n_head, n_embd = GPT_ZOO[name]
    routes = ("per_agent", "wide") if n_embd <= 256 else ("wide",)
    models = {}
    with Limit(args.step_timeout):
        torch.manual_seed(12345)
        cfg = dict(model_type=name, patch_size=P, block_size=T, with_detector=False, image_processor=None)
        for r in routes:
            if r == "wide":
                os.environ["JN_GPT_WIDE"] = "1"
            else:
                os.environ.pop("JN_GPT_WIDE", None)
            m = ja.GPT(model_config(**cfg), max_batch=B, device=dev)
            os.environ.pop("JN_GPT_WIDE", None)
            if models:
                m.load_state_dict(next(iter(models.values())).state_dict())
            m.eval()
            m.sync_weights()
            eng = m.engine()
            assert eng.lib.jn_debug_decision_route(eng.handle) == (1 if r == "wide" else 0), r
            models[r] = m
        g = torch.Generator().manual_seed(7)
        patches = torch.rand((B, T, 3, P, P), generator=g).to(dev)
        actions = torch.randint(0, 9, (B, T), generator=g).to(dev)
        positions = torch.randint(0, 5, (B, T, 2), generator=g).to(dev)
        classes = torch.zeros(B, dtype=torch.long, device=dev)
        prev = (torch.randn((B, T, n_embd), generator=g) * 0.5).to(dev)
        torch.cuda.synchronize()
    times = {r: [] for r in routes}
    fwd_times = {r: [] for r in routes}
    enc_times = {r: [] for r in routes}
    logits = {}
    last = patches[:, -1:].contiguous()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0, res
    for i in range(args.warmup + args.runs):
        for r in (routes if i % 2 == 0 else routes[::-1]):
            with Limit(args.step_timeout):
                fwd_us, (lg, _) = timed(lambda: models[r](patches, actions, classes, positions, prev))
                enc_us, _ = timed(lambda: models[r].embed_patches(last))
                us = (fwd_us - enc_us) / (T + 1)
            print(f"{name} run {i} {r}: forward {fwd_us:.1f} us, encoder pass {enc_us:.1f} us, decode {us:.1f} us per decision step",
                  file=sys.stderr, flush=True)
            logits[r] = lg
            if i >= args.warmup:
                times[r].append(us)
                fwd_times[r].append(fwd_us / (T + 1))
                enc_times[r].append(enc_us)
    out = {"n_layer": n_layer, "n_head": n_head, "n_embd": n_embd, "tokens": T + 1,
           "launches_per_token_wide": 7 * n_layer + 2,
           "block_weight_bytes": 12 * n_layer * n_embd * n_embd * 4}
    for r in routes:
        _summary(out, f"{r}_us_per_step", times[r])
        _summary(out, f"{r}_forward_us_per_step", fwd_times[r])
        _summary(out, f"{r}_encoder_us", enc_times[r])
    if len(routes) == 2:
        out["logits_max_difference"] = float((logits["wide"] - logits["per_agent"]).abs().max())
        out["logits_agree"] = out["logits_max_difference"] < 1e-4
        out["wide_over_per_agent"] = round(out["wide_us_per_step"] / out["per_agent_us_per_step"], 3)
    print("RESULT " + json.dumps(out), flush=True)


def stream_rate(args):
    """TB/s of one read stream beside one write stream (tools/streambench, the 411 MB row's first figure)."""
    if args.stream_tbps:
        return args.stream_tbps, "--stream-tbps"
    exe = ROOT / "tools" / "streambench"
    if not exe.exists():
        return None, "tools/streambench is not built"
    try:
        res = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=args.section_timeout)
    except subprocess.TimeoutExpired:
        return None, "tools/streambench ran into its time limit"
    if res.returncode != 0:
        return None, f"tools/streambench: exit code {res.returncode}"
    m = re.search(r"^\s*411 MB per stream:\s+1R1W ([0-9.]+)", res.stdout, re.M)
    return (float(m.group(1)), "tools/streambench, 1R1W at 411 MB per stream") if m else (None, "no 1R1W figure in its output")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--section-timeout", type=float, default=360.0, help="time limit of one child process")
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=MODELS)
    ap.add_argument("--stream-tbps", type=float, default=None, help="one-read-stream rate, instead of running tools/streambench")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    ap.add_argument("--model", type=str, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs of each kind"
    if args.model:
        return child(args)
    out = {"tool": "widegpt_ab", "patch_size": P, "B": B, "T": T, "runs": args.runs, "warmup": args.warmup,
           "note": "us_per_step = (one recurrent GPT.forward of 21 tokens - the encoder pass of its B patches, timed by itself) / 21"}
    tbps, src = stream_rate(args)
    out["stream_tbps"], out["stream_source"] = tbps, src
    if tbps is None and src != "tools/streambench is not built":
        out["stopped_after"] = "streambench"                # nothing more is started on the GPU after a child that failed
    for name in ([] if "stopped_after" in out else args.models):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--model", name, "--runs", str(args.runs), "--warmup", str(args.warmup),
               "--step-timeout", str(args.step_timeout)]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.section_timeout)     # stderr: passed on
            rc, text, err = res.returncode, res.stdout, ""
        except subprocess.TimeoutExpired as e:
            rc, text, err = 124, "", str(e)
        print(f"model {name}: exit code {rc}", file=sys.stderr, flush=True)
        line = next((ln for ln in text.splitlines() if ln.startswith("RESULT ")), None)
        if rc != 0 or line is None:
            out[name] = {"failed": True, "exit_code": rc, "note": err[-500:]}
            out["stopped_after"] = name
            break
        out[name] = json.loads(line[len("RESULT "):])
        if tbps:
            floor = out[name]["block_weight_bytes"] / (tbps * 1e12) * 1e6
            out[name]["weight_stream_floor_us"] = round(floor, 1)
            out[name]["wide_over_floor"] = round(out[name]["wide_us_per_step"] / floor, 2)
    text = json.dumps(out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)
    return 1 if "stopped_after" in out else 0


if __name__ == "__main__":
    sys.exit(main())
