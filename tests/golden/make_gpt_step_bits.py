"""Records tests/golden/gpt_step_bits.npz: logits and final embeddings of decision-only models (no patch encoder, so
no atomics anywhere) out of gpt_step_kernel, as the library of ONE NAMED COMMIT computes them.  The test
tests/test_gpu_gpt_step_bits.py holds every later form of the kernel to these bits: changes to the kernel's scheduling
and data movement must leave each floating-point operation, its operands and its order alone.

    JNROLL_LIB=/path/to/that/commit/libjnroll.so python tests/golden/make_gpt_step_bits.py --commit <hash>

The library is taken from JNROLL_LIB and nowhere else: build the named commit, point JNROLL_LIB at its libjnroll.so.
Every case is recorded twice from scratch and the two must agree bit for bit before anything is written.
gpt_step_bits_long.npz (--which long) holds the case whose K / V rows do not fit the workgroup's LDS: there the kernel
reads them from the cache in global memory, and must give the same bits.
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


def case_name(model, bs, pos, cat):
    return f"{model}_T{bs}_pos{int(pos)}_cat{int(cat)}"


def build(model, bs, pos, cat):
    """A seeded decision-only model on the engine."""
    sys.path.insert(0, str(ROOT))
    import jolineedle_amd as ja
    from oracle.gpt_ref import build_gpt_ref
    from jolineedle_amd.config import model_config
    kw = dict(model_type=model, block_size=bs, patch_size=16, use_pos_emb=pos, concat_emb=cat, no_patch_emb=True,
              with_detector=False, gpt_backbone=None, image_processor=None, nclasses=N_ACTIONS)
    oracle = build_gpt_ref(1234 + bs, **kw)
    oracle.eval()
    product = ja.GPT(model_config(**kw), max_batch=8)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product


def run_case(model, bs, pos, cat, nb=B, recurrent=True):
    """{name: array} of one case: the full-sequence call (cache lengths 0 .. T, class token first) and the recurrent
    calls t = 0 .. T - 1 (prev_embeddings; every new token at 1-D position 0, the two-token first call)."""
    product = build(model, bs, pos, cat)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library JNROLL_LIB points at")
    ap.add_argument("--which", choices=["short", "long"], default="short")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = os.environ.get("JNROLL_LIB")
    assert lib and Path(lib).is_file(), "JNROLL_LIB must point at the libjnroll.so built from the named commit"
    long_ = a.which == "long"
    a.out = a.out or str(OUT_LONG if long_ else OUT)
    kw = dict(nb=LONG_B, recurrent=False) if long_ else {}
    rec = {}
    for c in (LONG_CASES if long_ else CASES):
        one, two = run_case(*c, **kw), run_case(*c, **kw)
        for k in one:
            assert one[k].tobytes() == two[k].tobytes(), f"{k}: the recording library is not bit-reproducible"
            assert np.isfinite(one[k]).all(), k
        rec.update(one)
    rec["commit"] = np.array(a.commit)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, Path(a.out).stat().st_size, "bytes,", len(rec) - 1, "arrays, library of commit", a.commit)


if __name__ == "__main__":
    main()
