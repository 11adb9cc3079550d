"""Fixed-bar comparison of the yolox-nano patch encoder (448 px, train-mode BatchNorm) with an fp64 oracle.

Shared by the CPU test that shows the bars mean something on these inputs (tests/test_fp64_bars_cpu.py) and the GPU tests
that hold the engine to them at the launch shapes of the headline batch (tests/test_gpu_encoder_fp64.py).

The inputs are well conditioned on purpose: patches `torch.rand`, a dense `randn` upstream gradient on the FPN outputs.  The
encoder then has no near-tie (max-pool arg-max, ReLU) whose resolution moves whole gradient tensors, so the bars below are
fixed numbers: no noise factor, no conditioning draws, no family allowance.  Measured on the CPU for these inputs, distance
from fp64 (worst tensor; relative L2 / max-norm of max|ref|):
- fp32 oracle, 21 patches: maps 3.7e-5; gradients 2.3e-4 / 2.7e-4 (20 patches: 1.8e-4 / 3.2e-4; 8: 1.7e-4 / 2.6e-4);
- fp64 with one-ulp (1e-7) SiLU noise, 64 patches: maps 2.3e-5; gradients 2.5e-4 / 3.4e-4.  This is the conditioning an
  fp32 forward meets.  torch's fp32 CPU BatchNorm backward (fp32 sums over 200 000 - 800 000 pixels per channel) puts the
  fp32 oracle itself at up to 2e-3 on BN weight / bias gradients at 64 patches; the engine accumulates those sums in fp64.
The gradient bars are about 4x / 10x the noisy distances."""
import copy
import functools
import os

import torch

from oracle.gpt_ref import build_gpt_ref
from tests.helpers import randomize_bn

P = 448
SEED_MODEL, SEED_BN = 3, 5              # make_pair(3, ...) of the parity tests
MODEL_KW = dict(patch_size=P, block_size=2, with_detector=False, image_processor=None)
UPSTREAMS = ("all", "fpn2")             # dense gradient on all three FPN outputs / on fpn[2] only (the training backward)
PREFIX = "gpt_backbone."

# ---- the fixed bars (decided here, not derived from any engine output) -------------------------------------------------
MAP_L2 = 1e-4           # relative L2 per FPN level
MAP_MAX = 1e-3          # max-norm, relative to max|ref| of the level
STAT_ATOL = 1e-5        # running mean / var of every BN layer: |got - ref| <= STAT_ATOL + STAT_RTOL |ref|
STAT_RTOL = 1e-4
GRAD_L2 = 1e-3          # every encoder gradient: relative L2
GRAD_MAX = 3e-3         # ... and max-norm relative to max|ref|


def make_oracle():
    """The CPU oracle of make_pair(SEED_MODEL, bn_seed=SEED_BN, **MODEL_KW) (eval mode, fp32)."""
    oracle = build_gpt_ref(SEED_MODEL, **MODEL_KW)
    randomize_bn(oracle, SEED_BN)
    return oracle.eval()


def inputs(N):
    """Patches [N, 3, P, P] in [0, 1) and the upstream gradients R[i] (shapes of the three FPN outputs), fixed seeds."""
    g = torch.Generator().manual_seed(7000 + N)
    x = torch.rand((N, 3, P, P), generator=g)
    chans = (64, 128, 256)              # yolox-nano widths (0.25): 256, 512, 1024 x 0.25
    R = [torch.randn((N, c, P // s, P // s), generator=g) for c, s in zip(chans, (8, 16, 32))]
    return x, R


def upstream(R, which):
    assert which in UPSTREAMS, which
    return list(R) if which == "all" else [None, None, R[2]]


def encoder_pass(oracle, x, R, dtype=torch.float64, upstreams=UPSTREAMS):
    """One train-mode forward of oracle.gpt_backbone (a copy in `dtype`) and one backward per upstream variant.
    Returns {"maps": [3 levels], "stats": {running mean / var}, "grads": {variant: {parameter: gradient}}}, fp64 tensors,
    names as in the product's state_dict."""
    enc = copy.deepcopy(oracle.gpt_backbone).to(dtype).train()
    maps = enc(x.to(dtype))
    out = {"maps": [m.detach().double() for m in maps],
           "stats": {PREFIX + n: b.detach().double().clone() for n, b in enc.named_buffers()
                     if n.endswith(("running_mean", "running_var"))},
           "grads": {}}
    for k, which in enumerate(upstreams):
        enc.zero_grad(set_to_none=True)
        loss = sum((m * r.to(dtype)).sum() for m, r in zip(maps, upstream(R, which)) if r is not None)
        loss.backward(retain_graph=k + 1 < len(upstreams))
        out["grads"][which] = {PREFIX + n: p.grad.detach().double().clone() for n, p in enc.named_parameters()}
    return out


@functools.lru_cache(maxsize=1)
def reference(N):
    """The fp64 oracle on inputs(N): computed once per N (about 20 s and 16 GB of host memory at N = 64)."""
    return encoder_pass(make_oracle(), *inputs(N), dtype=torch.float64)


@functools.lru_cache(maxsize=1)
def eval_reference(N):
    """Eval-mode (running-statistics BN) FPN maps of inputs(N), fp64."""
    enc = copy.deepcopy(make_oracle().gpt_backbone).double().eval()
    with torch.no_grad():
        return [m.double() for m in enc(inputs(N)[0].double())]


def flat(result, which):
    """One upstream variant of an encoder_pass / reference result, as check() takes it."""
    return {"maps": result["maps"], "stats": result["stats"], "grads": result["grads"][which]}


def distances(got, ref):
    """[(kind, name, relative L2, max-norm / max|ref|, max|ref|)] for every tensor `got` holds; stats rows carry the
    worst |d| / (STAT_ATOL + STAT_RTOL |ref|) instead of the max-norm."""
    rows = []
    for i, g in enumerate(got.get("maps", ())):
        r, g = ref["maps"][i], g.detach().cpu().double()
        assert g.shape == r.shape, (i, g.shape, r.shape)
        scale = r.abs().max().item()
        rows.append(("map", f"fpn{i}", ((g - r).norm() / r.norm()).item(), (g - r).abs().max().item() / scale, scale))
    for name, g in got.get("stats", {}).items():
        r, g = ref["stats"][name], g.detach().cpu().double()
        d = (g - r).abs()
        rows.append(("stat", name, (d.norm() / max(r.norm().item(), 1e-30)).item(),
                     (d / (STAT_ATOL + STAT_RTOL * r.abs())).max().item(), r.abs().max().item()))
    for name, g in got.get("grads", {}).items():
        r, g = ref["grads"][name], g.detach().cpu().double().reshape(ref["grads"][name].shape)
        scale = r.abs().max().item()
        assert scale > 1e-12, ("a gradient that is zero in fp64", name)
        rows.append(("grad", name, ((g - r).norm() / r.norm()).item(), (g - r).abs().max().item() / scale, scale))
    return rows


def check(got, ref, tag="", map_l2=MAP_L2, map_max=MAP_MAX, map_abs=0.0, grad_l2=GRAD_L2, grad_max=GRAD_MAX,
          noise=None):
    """Holds `got` = {"maps": [...], "stats": {...}, "grads": {...}} (any subset; names as in the product's state_dict)
    to the fixed bars against the fp64 result `ref` (flat()).  Every tensor of `ref` of a kind that `got` holds must be
    there.  The map max-norm bar is map_max * max|ref| + map_abs.  `noise`: optional {name: relative L2 of the fp32 oracle},
    for the report only.  Returns the rows of distances(), worst first (by distance / bar); raises AssertionError naming
    every tensor over its bar."""
    for kind in ("stats", "grads"):
        if kind in got:
            missing = sorted(set(ref[kind]) - set(got[kind]))
            assert not missing, (tag, f"{kind} missing", missing[:5])
    if "maps" in got:
        assert len(got["maps"]) == len(ref["maps"]), tag
    rows = []
    for kind, name, l2, mx, scale in distances(got, ref):
        if kind == "map":
            bar2, barm = map_l2, map_max + map_abs / scale
        elif kind == "stat":
            bar2, barm = float("inf"), 1.0
        else:
            bar2, barm = grad_l2, grad_max
        rows.append((max(l2 / bar2, mx / barm), kind, name, l2, mx, scale, bar2, barm))
    rows.sort(key=lambda r: r[0], reverse=True)
    rep = os.environ.get("JN_TEST_GRAD_REPORT")
    if rep:
        with open(rep, "a") as f:
            f.write(f"# {tag}: worst max-norm tensors (tensor, max-norm distance, max|ref|, fp32-oracle noise, relative L2, "
                    f"fixed max-norm bar, L2 bar)\n")
            for ratio, kind, name, l2, mx, scale, bar2, barm in rows[:25]:
                f.write(f"{tag}\t{name}\t{mx:.3e}\t{scale:.3e}\t{(noise or {}).get(name, float('nan')):.3e}\tL2 {l2:.3e}\t"
                        f"bar {barm:.1e}\tL2bar {bar2:.1e}{'  OVER-BAR' if ratio >= 1.0 else ''}\n")
            g = [r for r in rows if r[1] == "grad"]
            if g:
                w = max(g, key=lambda r: r[3])
                f.write(f"# {tag}: worst relative L2 / bar: {w[2]} {w[3]:.3e} (bar {w[6]:.1e})\n")
    over = [(name, f"L2 {l2:.3e} (bar {bar2:.1e})", f"max {mx:.3e} (bar {barm:.1e})")
            for ratio, kind, name, l2, mx, scale, bar2, barm in rows if not ratio < 1.0]
    assert not over, (tag, f"{len(over)} tensor(s) over the fixed fp64 bars", over[:8])
    return rows


def summary(rows):
    """(worst map relative L2, worst gradient relative L2, worst gradient max-norm) of check()'s rows."""
    pick = lambda kind, i: max((r[i] for r in rows if r[1] == kind), default=0.0)
    return pick("map", 3), pick("grad", 3), pick("grad", 4)


# ---- the one-ulp SiLU noise of the conditioning probe (used by tests/test_gpu_parity.py and the CPU test) ---------------
class _UlpSiLU(torch.nn.Module):
    def __init__(self, gen, eps=1e-7):
        super().__init__()
        self.gen, self.eps = gen, eps

    def forward(self, x):
        y = torch.nn.functional.silu(x)
        return y * (1.0 + self.eps * torch.randn(y.shape, generator=self.gen, dtype=y.dtype))


def _with_noisy_silu(oracle, seed, eps):
    """A copy of the oracle whose every SiLU output carries relative Gaussian noise `eps`."""
    o = copy.deepcopy(oracle)
    gen = torch.Generator().manual_seed(seed)

    def swap(mod):
        for n, c in list(mod.named_children()):
            if isinstance(c, torch.nn.SiLU):
                setattr(mod, n, _UlpSiLU(gen, eps))
            else:
                swap(c)
    swap(o)
    return o
