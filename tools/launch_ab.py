#!/usr/bin/env python3
"""Do two builds of libjnroll.so enqueue the same kernels and compute the same numbers?  For changes to the host side of
the library that are meant to move code and nothing else.

``run`` calls once, at small shapes (gpt-nano, yolox-nano encoder and detector, 64 px patches, block size 4,
max_batch 4), every entry point that embeds patches or decodes teacher-forced tokens, and saves what they wrote:

  embed              jn_embed_patches, N = 3
  forward            jn_gpt_forward, B = 2, T = 3
  forward_prev       jn_gpt_forward with prev_embeddings, Tp = 2
  supervised_step    jn_supervised_step, B = 2, T = 2 (B * T = max_batch), with the gradient arena it leaves
  supervised_eval    jn_supervised_eval, B = 3, T = 3 (B * T = 9: encoder chunks of 4 + 4 + 1 patches)
  reinforce          a train-mode rollout (jn_reinforce_forward) and jn_reinforce_backward, B = 2, T = 3, with the gradients
  rollout_detect     an eval-mode rollout with the detector, B = 2, T = 3

Run it once per library under a kernel trace (tracing alone, the program after ``--``), and plainly as often as the
spread of a library against itself is wanted:

    rocprofv3 --kernel-trace --output-format csv -d OUT/a -- python tools/launch_ab.py run --lib A/libjnroll.so --out OUT/a
    rocprofv3 --kernel-trace --output-format csv -d OUT/b -- python tools/launch_ab.py run --lib B/libjnroll.so --out OUT/b
    python tools/launch_ab.py run --lib A/libjnroll.so --out OUT/a2        # ... a3, a4, a5

``compare`` needs no GPU.  It prints ONE JSON line: the dispatch counts of the two traces and the first dispatch whose
kernel name, grid or workgroup size differs (none: ``launches_identical``); per saved tensor whether A reproduces
itself bit for bit over its runs, else its largest difference between any two of them, and the largest difference of B
from any run of A.  Exit status 1 if the launches differ, a tensor that A reproduces differs in B, or B is further from
A than A from itself.

    python tools/launch_ab.py compare --a OUT/a OUT/a2 OUT/a3 OUT/a4 OUT/a5 --b OUT/b
"""
import argparse
import csv
import faulthandler
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

P, BLOCK, MAX_BATCH, GRID = 64, 4, 4, 4


def run(args):
    if args.lib:
        os.environ["JNROLL_LIB"] = str(Path(args.lib).resolve())
    faulthandler.dump_traceback_later(args.timeout, exit=True)      # a GPU call that never returns ends the process
    import torch
    import jolineedle_amd as ja
    from jolineedle_amd.config import model_config
    from bench import synth_inputs

    assert torch.cuda.is_available(), "launch_ab run needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(12345)
    model = ja.GPT(model_config(patch_size=P, block_size=BLOCK, image_processor="yolox-nano", detector_conf_threshold=1e-5),
                   max_batch=MAX_BATCH, device=dev)
    model.eval()
    model.sync_weights()
    g = torch.Generator().manual_seed(7)
    rand = lambda *shape: torch.rand(shape, generator=g).to(dev)
    ints = lambda hi, *shape: torch.randint(0, hi, shape, generator=g).to(dev)
    out = {}
    keep = lambda name, t: out.__setitem__(name, t.detach().cpu().clone())

    keep("embed", model.embed_patches(rand(1, 3, 3, P, P)))

    patches, actions, positions = rand(2, 3, 3, P, P), ints(9, 2, 3), ints(GRID, 2, 3, 2)
    classes = torch.tensor([3, 99], device=dev)
    with torch.no_grad():
        logits, final_emb = model(patches, actions, classes, positions)
        keep("forward.logits", logits)
        keep("forward.final_emb", final_emb)
        logits, final_emb2 = model(patches, actions, classes, positions, prev_embeddings=final_emb[:, :2])
        keep("forward_prev.logits", logits)
        keep("forward_prev.final_emb", final_emb2)

    sup = ja.SupervisedTrainer(ja.CfgNode(stop_enabled=True, stop_weight=2.0, loss_mode="best-action"), model)
    res = sup.train_step(rand(2, 2, 3, P, P), ints(9, 2, 2), ints(9, 2, 2), ints(GRID, 2, 2, 2), torch.ones((2, 2)),
                         optimizer_step=False, classes=classes)
    keep("supervised_step.logits", res["logits"])
    keep("supervised_step.loss", res["loss"])
    keep("supervised_step.grads", sup._grad_arena())
    sup._grad_arena().zero_()

    masks = (torch.arange(3)[None] < torch.tensor([3, 2, 1])[:, None]).float()
    res = sup.eval_step(rand(3, 3, 3, P, P), ints(9, 3, 3), ints(9, 3, 3), ints(GRID, 3, 3, 2), masks,
                        classes=torch.tensor([3, 99, 0]))
    for k in ("logits", "metrics", "token_loss", "predicted"):
        keep("supervised_eval." + k, res[k])

    T = 3
    images, bboxes, start = synth_inputs(2, GRID, P, 12345, dev)
    forced = ints(8, 2, T)
    rl = ja.ReinforceTrainer(ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=12345), model)
    env = ja.NeedleGeneralEnv(images, bboxes, P, T, 1, True, engine=model.engine())
    names = ("rewards", "returns", "logprobs", "entropies", "positions", "actions", "logits", "final_emb")
    model.train()
    ro = rl.rollout(env, forced_actions=forced, start_positions=start, keep_patches=False)
    for k in names:
        keep("reinforce." + k, ro[k])
    (ro["logprobs"].sum() + 0.5 * ro["entropies"].sum()).backward()
    keep("reinforce.grads", model._flat_grads)
    model.eval()
    with torch.no_grad():
        ro = rl.rollout(env, do_detection=True, forced_actions=forced, start_positions=start, keep_patches=False, bbox_lists=False)
    for k in names + ("det_boxes", "det_counts"):
        keep("rollout_detect." + k, ro[k])
    torch.cuda.synchronize()
    Path(args.out).mkdir(parents=True, exist_ok=True)
    torch.save(out, str(Path(args.out) / "outputs.pt"))
    print(json.dumps({"tool": "launch_ab", "saved": len(out), "lib": os.environ.get("JNROLL_LIB", "in-tree")}))
    return 0


def dispatches(folder):
    """[(kernel name, grid xyz, workgroup xyz)] of the one kernel trace under `folder`, in dispatch order."""
    files = sorted(Path(folder).rglob("*kernel_trace.csv"))
    assert len(files) == 1, f"{folder}: expected one *kernel_trace.csv, found {len(files)}"
    with open(files[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"))
            for r in rows]


def compare(args):
    import torch
    res = {"tool": "launch_ab"}
    a, b = dispatches(args.a[0]), dispatches(args.b)
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    res["dispatches"] = [len(a), len(b)]
    res["launches_identical"] = len(a) == len(b) and first is None
    if first is not None:
        res["first_difference"] = {"dispatch": first, "a": a[first], "b": b[first]}
    runs = [torch.load(str(Path(d) / "outputs.pt")) for d in args.a]
    other = torch.load(str(Path(args.b) / "outputs.pt"))
    diff = lambda x, y: float((x.double() - y.double()).abs().max()) if x.numel() else 0.0
    ok = res["launches_identical"] and runs[0].keys() == other.keys()
    res["tensors"] = {}
    for k, t in runs[0].items():
        same = all(torch.equal(t, r[k]) for r in runs[1:])
        spread = max([diff(x[k], y[k]) for i, x in enumerate(runs) for y in runs[i + 1:]], default=0.0)
        to_b = max(diff(r[k], other[k]) for r in runs)
        res["tensors"][k] = {"a_reproduces": same, "a_spread": spread, "b_equals_a": torch.equal(t, other[k]), "b_from_a": to_b}
        ok = ok and (torch.equal(t, other[k]) if same else to_b <= spread)
    res["a_runs"] = len(runs)
    res["ok"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", type=str, default=None, help="the libjnroll.so to load (default: the in-tree build)")
    r.add_argument("--out", type=str, required=True)
    r.add_argument("--timeout", type=float, default=240.0)
    c = sub.add_parser("compare")
    c.add_argument("--a", nargs="+", required=True, help="output folders of library A; the first one holds its kernel trace")
    c.add_argument("--b", required=True, help="output folder of library B, with its kernel trace")
    args = ap.parse_args()
    return run(args) if args.cmd == "run" else compare(args)


if __name__ == "__main__":
    sys.exit(main())
