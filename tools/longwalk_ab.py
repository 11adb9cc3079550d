#!/usr/bin/env python3
"""What the attention of the batched GPT backward costs in its two forms (kernels_gptbwd.hip) on one GPU: the LDS form (a
head's q, k, v, dY and two score tiles in 64 KB) and the tiled form (LDS that does not grow with the sequence; the only
form past T = 74 for gpt-nano and T = 63 for gpt-mini).  Everything else of the backward — the GEMMs, the LayerNorms, the
token embeddings — is the same launches under either form, so the difference of the two forms is the difference here.

Device events around ``jn_gpt_attention_backward`` (context-free: ONE layer's recompute + backward on N(0, 1) tensors, the
launches alone: its workspace is kept between calls), B = 64:

  (a) gpt-nano (3 heads of 16), T = 20 and T = 62: LDS against tiled, interleaved;
  (b) gpt-mini (6 heads of 32), T = 62: the same;
  (c) tiled alone at T = 128 and T = 255, both models.

Medians of seven with (max - min), in microseconds per layer; ``*_per_backward_us`` multiplies by the model's layer count.
Nothing is gated on these numbers.  Prints ONE JSON line.

    python tools/longwalk_ab.py [--runs 7] [--warmup 3] [--step-timeout 120] [--out profiles/longwalk_ab.json]
"""
import argparse
import faulthandler
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODELS = {"gpt-nano": (3, 3, 48), "gpt-mini": (6, 6, 192)}          # n_layer, n_head, n_embd
CASES = [("gpt-nano", 20, True), ("gpt-nano", 62, True), ("gpt-mini", 62, True),
         ("gpt-nano", 128, False), ("gpt-nano", 255, False), ("gpt-mini", 128, False), ("gpt-mini", 255, False)]
B = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from jolineedle_amd import _lib
    from jolineedle_amd._lib import check, ptr
    assert torch.cuda.is_available(), "longwalk_ab needs the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    stream = _lib.current_stream(dev)
    out = {"tool": "longwalk_ab", "B": B, "runs": args.runs, "unit": "us per layer (attention recompute + backward)", "cases": []}
    for name, T, both in CASES:
        n_layer, nh, C = MODELS[name]
        Lm = T + 1
        faulthandler.dump_traceback_later(args.step_timeout, exit=True)      # a call that never returns ends the process
        g = torch.Generator(device="cpu").manual_seed(7)
        qkv = torch.randn((B, Lm, 3 * C), generator=g).to(dev)
        dy = torch.randn((B, Lm, C), generator=g).to(dev)
        att = torch.empty((B * nh, Lm, Lm), device=dev)
        y = torch.empty((B, Lm, C), device=dev)
        dqkv = torch.empty((B, Lm, 3 * C), device=dev)
        forms = (("lds", 0), ("tiled", 1)) if both else (("tiled", 1),)

        def run(form):
            check(lib.jn_gpt_attention_backward(form, ptr(qkv), ptr(dy), B, nh, C, Lm, Lm, 0.0, 0, 0, Lm, ptr(att), ptr(y), ptr(dqkv),
                                                stream), "jn_gpt_attention_backward")
        for _ in range(args.warmup):
            for _, f in forms:
                run(f)
        torch.cuda.synchronize()
        times = {k: [] for k, _ in forms}
        for _ in range(args.runs):                                           # interleaved: one run of each form in turn
            for k, f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(f)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        faulthandler.cancel_dump_traceback_later()
        row = {"model": name, "T": T, "route_rule": {1: "lds", 2: "per_agent", 3: "tiled"}.get(lib.jn_gpt_backward_route(C, nh, T, 0))}
        for k, v in times.items():
            row[k + "_us"] = round(statistics.median(v), 2)
            row[k + "_us_spread"] = round(max(v) - min(v), 2)
            row[k + "_per_backward_us"] = round(statistics.median(v) * n_layer, 1)
        if both:
            row["tiled_over_lds"] = round(row["tiled_us"] / row["lds_us"], 3)
        out["cases"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
