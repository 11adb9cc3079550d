"""Records tests/golden/gpt_step_bits.npz: logits and final embeddings of decision-only models (no patch encoder, so
no atomics anywhere) out of gpt_step_kernel, as the library of ONE NAMED COMMIT computes them.  The test
tests/test_gpu_gpt_step_bits.py holds every later form of the kernel to these bits: changes to the kernel's scheduling
and data movement must leave each floating-point operation, its operands and its order alone.

    JNROLL_LIB=/path/to/that/commit/libjnroll.so python tests/golden/make_gpt_step_bits.py --commit <hash>

The library is taken from JNROLL_LIB and nowhere else: build the named commit, point JNROLL_LIB at its libjnroll.so.
Every case is recorded twice from scratch and the two must agree bit for bit before anything is written.
gpt_step_bits_long.npz (--which long) holds the case whose K / V rows do not fit the workgroup's LDS: there the kernel
reads them from the cache in global memory, and must give the same bits.
gpt_wide_bits.npz (--which wide) holds the agents-batched route (kernels_gptwide.hip, contexts created under
JN_GPT_WIDE=1) on the same kind of forward cases, and whole rollouts — sampled, forced, greedy — on both routes: the
decision behind the head (argmax, draw, forced id, env step, bookkeeping) is one function that both routes call, and
these rollouts hold it to what each route's own copy computed in the named commit.
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "gpt_step_bits.npz"
OUT_LONG = Path(__file__).resolve().parent / "gpt_step_bits_long.npz"
OUT_WIDE = Path(__file__).resolve().parent / "gpt_wide_bits.npz"
B = 3
CLASSES = (37, 0, 99)
N_ACTIONS = 9
GRID = 5
# (model, block size, use_pos_emb, concat_emb): both thread counts of the kernel (n_embd 48 -> 256 threads, 192 -> 1024),
# both block sizes with all embeddings on, the two switches at block size 20 (K of the embedding projection = 3C, 2C)
CASES = [(m, bs, True, True) for m in ("gpt-nano", "gpt-mini") for bs in (20, 32)] + \
        [(m, 20, pos, cat) for m in ("gpt-nano", "gpt-mini") for pos, cat in ((False, True), (True, False))]


# n_embd 192 at block size 100: 2 x 101 x 192 floats of K / V rows (155 KB) beside the kernel's 26 KB pass a CU's 160 KB of
# LDS, so the rows stay in global memory.  Two agents, the full-sequence call only (cache lengths 0 .. 100): a small file.
LONG_CASES = [("gpt-mini", 100, True, True)]
LONG_B = 2


# The wide route, forward: gpt-mini (admitted by both routes) with all embeddings on and the two switches, and an odd-sized
# model past the per-agent envelope (K = 320 is no power of two, five column tiles of 64), all at block size 20
WIDE_DIMS = {"wide-320": (2, 5, 320)}             # (n_layer, n_head, n_embd) of the models the zoo does not hold
WIDE_CASES = [("gpt-mini", 20, True, True), ("gpt-mini", 20, False, True), ("gpt-mini", 20, True, False),
              ("wide-320", 20, True, True)]
# Rollouts of gpt-mini on either route: 3 agents, 4 steps on a 3 x 4 grid of 64-px patches.  The forced one stops every
# agent at step 2 (step 3 takes the skip path of every launch) and holds one id above and one below the action range
# (the clamp of a forced id); the sampled one draws with trainer seed 1.
ROLL_T, ROLL_P, ROLL_GRID, ROLL_SEED = 4, 64, (3, 4), 1
ROLLOUT_CASES = [(route, kind) for route in ("per_agent", "wide") for kind in ("sampled", "forced", "greedy")]


def case_name(model, bs, pos, cat):
    return f"{model}_T{bs}_pos{int(pos)}_cat{int(cat)}"


def build(model, bs, pos, cat, wide=False, patch_size=16):
    """A seeded decision-only model on the engine; wide: its context takes the agents-batched route."""
    sys.path.insert(0, str(ROOT))
    import jolineedle_amd as ja
    from oracle import gpt_ref
    from jolineedle_amd.config import model_config
    kw = dict(model_type=model, block_size=bs, patch_size=patch_size, use_pos_emb=pos, concat_emb=cat, no_patch_emb=True,
              with_detector=False, gpt_backbone=None, image_processor=None, nclasses=N_ACTIONS)
    if model in WIDE_DIMS:
        gpt_ref.GPT_ZOO[model] = WIDE_DIMS[model]
    oracle = gpt_ref.build_gpt_ref(1234 + bs, **kw)
    oracle.eval()
    if model in WIDE_DIMS:                                # the engine takes such a model by its dimensions
        kw.update(model_type=None, **dict(zip(("n_layer", "n_head", "n_embd"), WIDE_DIMS[model])))
    before = os.environ.get("JN_GPT_WIDE")
    try:
        if wide:
            os.environ["JN_GPT_WIDE"] = "1"
        else:
            os.environ.pop("JN_GPT_WIDE", None)
        product = ja.GPT(model_config(**kw), max_batch=8)
    finally:
        os.environ.pop("JN_GPT_WIDE", None)
        if before is not None:
            os.environ["JN_GPT_WIDE"] = before
    eng = product.engine()
    assert eng.lib.jn_debug_decision_route(eng.handle) == int(wide), (model, wide)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product


def run_case(model, bs, pos, cat, nb=B, recurrent=True, wide=False):
    """{name: array} of one case: the full-sequence call (cache lengths 0 .. T, class token first) and the recurrent
    calls t = 0 .. T - 1 (prev_embeddings; every new token at 1-D position 0, the two-token first call)."""
    product = build(model, bs, pos, cat, wide=wide)
    g = torch.Generator().manual_seed(99 + bs)
    actions = torch.randint(0, N_ACTIONS, (nb, bs), generator=g)
    positions = torch.randint(0, GRID, (nb, bs, 2), generator=g)
    classes = torch.tensor(CLASSES[:nb], dtype=torch.long)
    n = case_name(model, bs, pos, cat)
    with torch.no_grad():
        lg, emb = product(None, actions, classes, positions if pos else None)
        if not recurrent:
            torch.cuda.synchronize()
            return {f"{n}.full_logits": lg.cpu().numpy(), f"{n}.full_emb": emb.cpu().numpy()}
        e, rec = None, []
        for t in range(bs):
            l, e = product(None, actions[:, :t + 1], classes, positions[:, :t + 1] if pos else None, e)
            rec.append(l[:, -1])
        torch.cuda.synchronize()
    return {f"{n}.full_logits": lg.cpu().numpy(), f"{n}.full_emb": emb.cpu().numpy(),
            f"{n}.rec_logits": torch.stack(rec, 1).cpu().numpy(), f"{n}.rec_emb": e.cpu().numpy()}


def rollout_name(route, kind):
    return f"rollout_{route}_{kind}"


def run_rollout(route, kind):
    """{name: array} of one rollout of gpt-mini on `route`: what the decision wrote (actions, positions, masks, rewards)
    and what it left in the env (positions, visited grid) as integers, log-probs / entropies / logits as their bits."""
    product = build("gpt-mini", ROLL_T, True, True, wide=route == "wide", patch_size=ROLL_P)
    import jolineedle_amd as ja
    from tests.helpers import synth_batch
    images, bboxes, start = synth_batch(B, *ROLL_GRID, ROLL_P, seed=31)
    cfg = ja.CfgNode(max_seq_len=ROLL_T, entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=ROLL_SEED)
    kw = dict(start_positions=start, keep_patches=False)
    if kind == "forced":
        forced = torch.randint(0, 8, (B, ROLL_T), generator=torch.Generator().manual_seed(9))
        forced[:, 2] = 8
        forced[0, 1], forced[1, 1] = 11, -3               # clamped to 8 (STOP) and 0
        kw["forced_actions"] = forced
    else:
        kw["sample_actions"] = kind == "sampled"
    env = ja.NeedleGeneralEnv(images.to("cuda:0"), bboxes, ROLL_P, ROLL_T, 1, True)
    with torch.no_grad():
        ro = ja.ReinforceTrainer(cfg, product).rollout(env, **kw)
    torch.cuda.synchronize()
    n = rollout_name(route, kind)
    got = {f"{n}.{k}": ro[k].cpu().to(torch.int64).numpy() for k in ("actions", "positions", "masks")}
    got[f"{n}.env_positions"] = env.positions.cpu().to(torch.int64).numpy()
    got[f"{n}.env_visited"] = env.visited_patches.cpu().to(torch.int64).numpy()
    for k in ("rewards", "logprobs", "entropies", "logits"):
        got[f"{n}.{k}_bits"] = ro[k].cpu().contiguous().numpy().view(np.int32)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library JNROLL_LIB points at")
    ap.add_argument("--which", choices=["short", "long", "wide"], default="short")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = os.environ.get("JNROLL_LIB")
    assert lib and Path(lib).is_file(), "JNROLL_LIB must point at the libjnroll.so built from the named commit"
    long_, wide = a.which == "long", a.which == "wide"
    a.out = a.out or str(OUT_LONG if long_ else OUT_WIDE if wide else OUT)
    kw = dict(nb=LONG_B, recurrent=False) if long_ else dict(wide=True) if wide else {}
    jobs = [(run_case, c, kw) for c in (LONG_CASES if long_ else WIDE_CASES if wide else CASES)]
    if wide:
        jobs += [(run_rollout, c, {}) for c in ROLLOUT_CASES]
    rec = {}
    for fn, c, kw in jobs:
        one, two = fn(*c, **kw), fn(*c, **kw)
        for k in one:
            assert one[k].tobytes() == two[k].tobytes(), f"{k}: the recording library is not bit-reproducible"
            assert np.isfinite(one[k]).all(), k
        rec.update(one)
    rec["commit"] = np.array(a.commit)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes,", len(rec) - 1, "arrays, library of commit", a.commit)


if __name__ == "__main__":
    main()
