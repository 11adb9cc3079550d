"""Cases, inputs, fp64 references and bars for the decision-side training kernels (csrc/kernels_train.hip: reinforce_loss_kernel,
logits_grad_kernel, ce_loss_kernel, adamw_kernel), one kernel at a time through the context-free entries jn_reinforce_loss,
jn_logits_grad, jn_ce_loss and jn_adamw.

Shared by tests/test_train_cases_cpu.py (the bars mean something on these inputs and bite on the mistakes such kernels make) and
tests/test_gpu_train_kernels.py (every kernel against the reference).  Fixed seeds, no committed tensors.

The references are statements of the formulas, not of the kernels.  The losses are written in torch fp64 on the fp32 inputs and
differentiated by autograd:
 - REINFORCE: masked mean of -logp[action] adv + w x masked mean of -H over the tokens with t < S and mask != 0,
   adv = (returns - mean) / (std + 1e-8) with reward_norm, else the returns;
 - logits_grad: sum(dlogprobs logp[action] + dentropies H) over the rows t < S;
 - cross-entropy: torch's weighted cross_entropy (weight[8] = stop_weight), meaned over the masks == 1 tokens.
AdamW's reference is torch.optim.AdamW itself on CPU fp64 tensors, after the trainers' scale-then-clip_grad_value_.

A loss case is a Case tuple (kind "rf" / "lg" / "ce"); the fields a kind does not use stay at their defaults:
 - mask: "full", "holes" (about a third of the tokens off), "agent" (holes, and one agent entirely off), "none" (everything off);
 - stop: 0 = no n_done array, 1 = S = 1, 2 = S = T - 1, 3 = an array that never reaches B (no stop);
 - norm, ew, scale: reward_norm, entropy_weight, loss_scale;  big: logits x 30 (the max subtraction);
 - tiny: returns of size 1e-7, so that the 1e-8 beside the standard deviation is a tenth of the advantage;
 - up: "both" / "nolp" (dlogprobs null) / "noent" (dentropies null);  sw: stop_weight.
Shapes: B T in {1, 255, 256, 257, 1300} with T in {1, 5, 20}: the 256-thread stride loop of the two one-workgroup kernels runs zero,
one and several times and a tail is cut; logits_grad_kernel's grid has one, one full, two and six workgroups.

An AdamW case is an Adam tuple: n elements, p "zero" (with wd 0 the parameter after the step is the update itself) or "normal"
(N(0, 1), with a few of size 2e-3: a decay applied after the update moves a parameter by lr wd |update| = 1e-8, which only a small
parameter shows), wd, clip (0 = off), gs = grad_scale, and either steps = 5 consecutive steps from zero moments or step = one step
numbered `step` from moments pre-loaded from the fp64 reference's state after seven steps, rounded to fp32."""
import collections
import functools
import math
import zlib

import numpy as np
import torch

CANARY = 77777.0
F = np.float32

Case = collections.namedtuple("Case", "kind B T nA mask stop norm ew scale big tiny up sw")
_DEFAULTS = dict(nA=9, mask="full", stop=0, norm=1, ew=0.01, scale=1.0, big=0, tiny=0, up="both", sw=2.5)
Adam = collections.namedtuple("Adam", "n p wd clip gs steps step")

SHAPES = ((1, 1), (51, 5), (256, 1), (257, 1), (65, 20))
LR = 1e-3
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
WARM_STEPS = 7                  # the reference steps behind the pre-loaded moments

# ---- the bars -------------------------------------------------------------------------------------------------------------------
# Measured as RED_BAR (dw_cases.py) was: the plain fp32 restatement of each kernel below, in natural order (one token after the
# other, one class after the other), against the fp64 reference on the cases of this file (test_train_cases_cpu.py prints the
# figures); the bar 4 x that, rounded up to one digit.  dlogits: relative L2 (l2) and max |delta| / max |ref| (mx); metrics:
# absolute (met).  The logits x 30 cases have bars of their own: logits - logsumexp is rounded at the size of the logits, so every
# figure is several times that of the other cases, which would otherwise be held to the large logits' bar.
RF_FP32_MEASURED = dict(l2=1.7e-7, mx=4.2e-7, met=6.8e-7)      # (65 x 20 with holes: S = 1; no stop; reward_norm off)
RF_BAR = dict(l2=7e-7, mx=2e-6, met=3e-6)
LG_FP32_MEASURED = dict(l2=3.7e-7, mx=7.4e-7)                  # (dlogprobs null, 65 x 20 and 51 x 5)
LG_BAR = dict(l2=2e-6, mx=3e-6)
CE_FP32_MEASURED = dict(l2=2.8e-7, mx=6.2e-7, met=5.2e-6)      # (1 x 1; 65 x 20; the loss of 65 x 20 x 5: 1300 terms one after the other)
CE_BAR = dict(l2=2e-6, mx=3e-6, met=3e-5)
BIG_FP32_MEASURED = dict(rf=dict(l2=5.0e-7, mx=1.5e-6, met=9.2e-7), lg=dict(l2=6.3e-7, mx=1.9e-6), ce=dict(l2=5.5e-7, mx=3.6e-6, met=2.6e-5))
BIG_BAR = dict(rf=dict(l2=2e-6, mx=6e-6, met=4e-6), lg=dict(l2=3e-6, mx=8e-6), ce=dict(l2=3e-6, mx=2e-5, met=2e-4))
# AdamW, per element, the worst of a case's steps: p |delta| / max(|ref|, lr) (an update is of the size of lr); m |delta| over the
# sum of the |terms| of m so far (adam_reference); v |delta| / |ref|
AD_FP32_MEASURED = dict(p=7.1e-7, m=3.7e-7, v=4.1e-7)          # (all three: five steps over 65537 elements)
AD_BAR = dict(p=3e-6, m=2e-6, v=2e-6)


def bar_of(measured):
    """4 x the measured figure, rounded up to one digit."""
    x = 4.0 * measured
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def _case(kind, B, T, **kw):
    return Case(kind, B, T, **dict(_DEFAULTS, **kw))


def _loss_cases():
    rf = [_case("rf", B, T) for B, T in SHAPES]
    rf += [_case("rf", B, T, nA=5, mask="holes") for B, T in ((51, 5), (65, 20))]
    rf += [_case("rf", B, T, mask="holes") for B, T in ((51, 5), (257, 1), (65, 20))]
    rf += [_case("rf", 51, 5, mask="agent"), _case("rf", 51, 5, mask="none"), _case("rf", 1, 1, mask="none")]
    rf += [_case("rf", B, T, mask="holes", stop=s) for B, T in ((51, 5), (65, 20)) for s in (1, 2, 3)]
    rf += [_case("rf", 65, 20, mask="holes", norm=0), _case("rf", 65, 20, mask="holes", ew=0.0, scale=0.25),
           _case("rf", 65, 20, mask="holes", norm=0, ew=0.0, scale=0.25), _case("rf", 51, 5, scale=0.25, stop=2)]
    rf += [_case("rf", 65, 20, big=1), _case("rf", 51, 5, mask="holes", tiny=1)]
    lg = [_case("lg", B, T) for B, T in SHAPES]
    lg += [_case("lg", 51, 5, nA=5), _case("lg", 65, 20, nA=5, stop=2)]
    lg += [_case("lg", B, T, up=u) for B, T in ((51, 5), (65, 20)) for u in ("nolp", "noent")]
    lg += [_case("lg", B, T, stop=s) for B, T in ((51, 5), (65, 20)) for s in (1, 2, 3)]
    lg += [_case("lg", 65, 20, big=1)]
    ce = [_case("ce", B, T, mask="holes" if B * T > 1 else "full") for B, T in SHAPES]
    ce += [_case("ce", B, T, sw=1.0, mask="holes") for B, T in ((51, 5), (65, 20))]
    ce += [_case("ce", 51, 5, nA=5, mask="holes"), _case("ce", 65, 20, nA=5)]
    ce += [_case("ce", 65, 20), _case("ce", 51, 5, mask="agent"), _case("ce", 51, 5, mask="none"), _case("ce", 1, 1, mask="none")]
    ce += [_case("ce", 65, 20, big=1)]
    return rf + lg + ce


def _adam_cases():
    seq = lambda n, **kw: Adam(**dict(dict(n=n, p="zero", wd=0.0, clip=1.0, gs=1.0, steps=5, step=0), **kw))
    one = lambda step, **kw: Adam(**dict(dict(n=257, p="zero", wd=0.0, clip=1.0, gs=1.0, steps=0, step=step), **kw))
    cases = [seq(n) for n in (1, 255, 256, 257, 65537)]
    cases += [seq(257, clip=0.0), seq(257, gs=0.25), seq(257, gs=0.25, clip=0.0), seq(257, p="normal", wd=0.01), seq(257, p="normal"),
              seq(1, p="normal", wd=0.01), seq(65537, p="normal", wd=0.01, gs=0.25)]
    cases += [one(s) for s in (1, 2, 10, 1000)] + [one(s, p="normal", wd=0.01) for s in (1, 2, 10, 1000)]
    cases += [one(1, gs=0.25), one(10, clip=0.0, gs=0.25), one(1000, clip=0.0)]
    return cases


LOSS_CASES = _loss_cases()
ADAM_CASES = _adam_cases()


def case_id(c):
    if isinstance(c, Adam):
        return f"adam-n{c.n}-{c.p}-wd{c.wd:g}-clip{c.clip:g}-gs{c.gs:g}-" + (f"steps{c.steps}" if c.steps else f"step{c.step}")
    return (f"{c.kind}-{c.B}x{c.T}x{c.nA}-{c.mask}-stop{c.stop}-norm{c.norm}-ew{c.ew:g}-scale{c.scale:g}-sw{c.sw:g}-{c.up}" +
            ("-big" if c.big else "") + ("-tiny" if c.tiny else ""))


def _seed(c):
    return zlib.crc32(repr(tuple(c)).encode())


def steps_of(c, n_done):
    """S: the first t in 1..T at which every agent is done, T without one."""
    if n_done is not None:
        for t in range(1, c.T + 1):
            if int(n_done[t]) >= c.B:
                return t
    return c.T


# ==== inputs =======================================================================================================================
@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's tensors on the CPU (fp32, int64, uint8, int32), never modified.  Scalars that reach the kernel as fp32 are fp32
    values here (ret_mean, ret_std, ew)."""
    g = torch.Generator().manual_seed(_seed(c))
    B, T, nA = c.B, c.T, c.nA
    logits = torch.randn((B, T, nA), generator=g) * (30.0 if c.big else 3.0)
    actions = torch.randint(0, nA, (B, T), generator=g)
    if c.mask == "full":
        masks = torch.ones((B, T), dtype=torch.uint8)
    elif c.mask == "none":
        masks = torch.zeros((B, T), dtype=torch.uint8)
    else:
        masks = (torch.rand((B, T), generator=g) > 0.3).to(torch.uint8)
        masks.view(-1)[0], masks.view(-1)[-1] = 1, 0
        if c.mask == "agent":
            masks[B // 2] = 0
    if c.stop == 0:
        n_done = None
    else:
        S = {1: 1, 2: T - 1, 3: T + 1}[c.stop]
        assert S >= 1
        n_done = torch.tensor([B if t >= S else min(t, B - 1) for t in range(T + 1)], dtype=torch.int32)
    d = dict(logits=logits, actions=actions, masks=masks, n_done=n_done)
    if c.kind == "rf":
        d["returns"] = torch.randn((B, T), generator=g) * (1e-7 if c.tiny else 1.0)
        d["rewards"] = torch.randn((B, T), generator=g)
        r = d["returns"].double()
        d["ret_mean"] = float(F(r.mean().item()))
        d["ret_std"] = float(F(r.std().item())) if B * T > 1 else 1.0
        d["ew"] = float(F(c.ew))
    elif c.kind == "lg":
        glp, gh = torch.randn((B, T), generator=g), torch.randn((B, T), generator=g)
        for i in {0, (B * T) // 2}:                        # tokens with both upstream values 0: exactly zero rows
            glp.view(-1)[i] = gh.view(-1)[i] = 0.0
        d["dlogprobs"] = None if c.up == "nolp" else glp
        d["dentropies"] = None if c.up == "noent" else gh
        d["zero_rows"] = sorted({0, (B * T) // 2})
    else:
        # a constructed tie on a counted token: classes 1 and 3 share the maximum, the target is the first
        top = logits[0, 0].abs().max() + 1.0
        logits[0, 0, 1] = logits[0, 0, 3] = top
        d["target"] = actions
        d["target"][0, 0] = 1
    return d


# ==== fp64 references ==============================================================================================================
def _parts64(logits):
    lg = logits.double().clone().requires_grad_(True)
    logp = torch.log_softmax(lg, dim=-1)
    H = -(logp.exp() * logp).sum(dim=-1)
    return lg, logp, H


@functools.lru_cache(maxsize=None)
def reference(c):
    """{"dlogits": fp64 [B, T, nA], "metrics": fp64 list, "S", "sel": the counted tokens}, never modified."""
    d = inputs(c)
    B, T, nA = c.B, c.T, c.nA
    S = steps_of(c, d["n_done"])
    executed = (torch.arange(T) < S)[None, :].expand(B, T)
    lg, logp, H = _parts64(d["logits"])
    zero = torch.zeros((B, T, nA), dtype=torch.float64)
    if c.kind == "rf":
        sel = (d["masks"] != 0) & executed
        lp = logp.gather(-1, d["actions"][..., None]).squeeze(-1)
        ret = d["returns"].double()
        adv = (ret - d["ret_mean"]) / (d["ret_std"] + 1e-8) if c.norm else ret
        n = sel.sum().double()
        action_loss = (-(lp * adv))[sel].sum() / n
        entropy_loss = (-H)[sel].sum() / n
        loss = action_loss + d["ew"] * entropy_loss
        if int(n) > 0:
            (c.scale * loss).backward()
        metrics = [action_loss.item(), entropy_loss.item(), loss.item(), (d["rewards"].double()[sel].sum() / B).item(), (n / B).item(), float(S)]
        return dict(dlogits=lg.grad if int(n) > 0 else zero, metrics=metrics, S=S, sel=sel)
    if c.kind == "lg":
        lp = logp.gather(-1, d["actions"][..., None]).squeeze(-1)
        glp = torch.zeros((B, T), dtype=torch.float64) if d["dlogprobs"] is None else d["dlogprobs"].double()
        gh = torch.zeros((B, T), dtype=torch.float64) if d["dentropies"] is None else d["dentropies"].double()
        (glp * lp + gh * H)[executed].sum().backward()
        return dict(dlogits=lg.grad, S=S, sel=executed)
    sel = d["masks"] == 1
    w = torch.ones(nA, dtype=torch.float64)
    if nA > 8:
        w[8] = c.sw
    y = d["target"]
    ce = torch.nn.functional.cross_entropy(lg.reshape(B * T, nA), y.flatten(), weight=w, reduction="none").view(B, T)
    loss = ce[sel].mean()
    n = int(sel.sum())
    if n > 0:
        loss.backward()
    pred = torch.from_numpy(np.argmax(d["logits"].numpy(), axis=-1))          # numpy: the first occurrence of the maximum
    hits = int((pred[sel] == y[sel]).sum())
    metrics = [loss.item(), hits / n if n else float("nan"), n / B]
    return dict(dlogits=lg.grad if n > 0 else zero, metrics=metrics, S=T, sel=sel, hits=hits, n=n, pred=pred)


# ==== the kernels restated in plain fp32, in natural order ==========================================================================
def _seqsum(x):
    """fp32 sum, one element after the other."""
    x = np.asarray(x, dtype=F)
    return F(np.cumsum(x, dtype=F)[-1]) if x.size else F(0.0)


def _parts32(lg):
    """lg fp32 [n, nA] -> (lse, logp, p, H): maximum, then the exponentials and the entropy one class after the other."""
    n, nA = lg.shape
    mx = lg.max(axis=1)
    se = np.zeros(n, dtype=F)
    for j in range(nA):
        se = se + np.exp(lg[:, j] - mx)
    lse = mx + np.log(se)
    lp = lg - lse[:, None]
    p = np.exp(lp)
    H = np.zeros(n, dtype=F)
    for j in range(nA):
        H = H - lp[:, j] * p[:, j]
    return lse, lp, p, H


def compute(c, mutant=None):
    """The case's kernel in fp32 numpy.  mutant: None, or one of the planted faults "mean_bt" (the mean over B T instead of the
    counted tokens), "no_H" (H dropped from the entropy gradient), "adv_no_eps" (the advantage without the 1e-8), "wrong_class" (the
    stop weight on class 7), "unzeroed" (rows that are not counted keep what a counted row would get), "ignore_S" (S = T)."""
    d = inputs(c)
    B, T, nA = c.B, c.T, c.nA
    n = B * T
    S = T if mutant == "ignore_S" else steps_of(c, d["n_done"])
    t = np.arange(n) % T
    lg = d["logits"].numpy().reshape(n, nA)
    lse, lp, p, H = _parts32(lg)
    Hg = np.zeros_like(H) if mutant == "no_H" else H
    with np.errstate(divide="ignore", invalid="ignore"):
        if c.kind == "rf":
            act = d["actions"].numpy().reshape(n)
            onehot = (np.arange(nA)[None, :] == act[:, None]).astype(F)
            sel = (d["masks"].numpy().reshape(n) != 0) & (t < S)
            msum = F(n) if mutant == "mean_bt" else F(sel.sum())
            ret = d["returns"].numpy().reshape(n)
            if c.norm:
                adv = (ret - F(d["ret_mean"])) / (F(d["ret_std"]) + (F(0.0) if mutant == "adv_no_eps" else F(1e-8)))
            else:
                adv = ret
            k = F(c.scale) / msum
            dl = k * (-adv[:, None] * (onehot - p) + F(d["ew"]) * p * (lp + Hg[:, None]))
            if mutant != "unzeroed":
                dl[~sel] = 0.0
            la = _seqsum((-(lp[np.arange(n), act]) * adv)[sel])
            le = _seqsum((-H)[sel])
            lr = _seqsum(d["rewards"].numpy().reshape(n)[sel])
            m0, m1 = la / msum, le / msum
            metrics = [m0, m1, m0 + F(d["ew"]) * m1, lr / F(B), msum / F(B), F(S)]
            return dict(dlogits=dl.reshape(B, T, nA), metrics=[float(x) for x in metrics])
        if c.kind == "lg":
            act = d["actions"].numpy().reshape(n)
            onehot = (np.arange(nA)[None, :] == act[:, None]).astype(F)
            glp = np.zeros(n, dtype=F) if d["dlogprobs"] is None else d["dlogprobs"].numpy().reshape(n)
            gh = np.zeros(n, dtype=F) if d["dentropies"] is None else d["dentropies"].numpy().reshape(n)
            dl = glp[:, None] * (onehot - p) - gh[:, None] * p * (lp + Hg[:, None])
            dl[t >= S] = 0.0
            return dict(dlogits=dl.reshape(B, T, nA))
        y = d["target"].numpy().reshape(n)
        onehot = (np.arange(nA)[None, :] == y[:, None]).astype(F)
        sel = d["masks"].numpy().reshape(n) != 0
        nvalid = F(n) if mutant == "mean_bt" else F(sel.sum())
        wy = np.where(y == (7 if mutant == "wrong_class" else 8), F(c.sw), F(1.0)).astype(F)
        dl = wy[:, None] * (np.exp(lg - lse[:, None]) - onehot) / nvalid
        if mutant != "unzeroed":
            dl[~sel] = 0.0
        ls = _seqsum((-wy * (lg[np.arange(n), y] - lse))[sel])
        acc = F((np.argmax(lg, axis=1) == y)[sel].sum())
        metrics = [ls / nvalid, acc / nvalid, nvalid / F(B)]
        return dict(dlogits=dl.reshape(B, T, nA), metrics=[float(x) for x in metrics])


LOSS_MUTANTS = {
    "mean_bt": lambda c: c.kind in ("rf", "ce") and c.mask in ("holes", "agent"),
    "no_H": lambda c: (c.kind == "rf" and c.ew != 0.0) or (c.kind == "lg" and c.up != "noent"),
    "adv_no_eps": lambda c: c.kind == "rf" and c.norm and c.tiny,
    "wrong_class": lambda c: c.kind == "ce" and c.nA > 8 and c.sw != 1.0 and c.mask != "none",
    "unzeroed": lambda c: c.kind in ("rf", "ce") and c.mask in ("holes", "agent"),
    "ignore_S": lambda c: c.kind in ("rf", "lg") and c.stop in (1, 2),
}


# ==== distances and bars ===========================================================================================================
def bars(c):
    return BIG_BAR[c.kind] if c.big else {"rf": RF_BAR, "lg": LG_BAR, "ce": CE_BAR}[c.kind]


def distances(c, got, ref):
    """{"l2", "mx": dlogits relative L2 and max |delta| / max |ref| (0 where the reference is all zero and so is `got`, inf where only
    the reference is), "met": the worst absolute distance of a metric (NaN counts as equal to NaN, and as inf against a number)}."""
    g, r = torch.as_tensor(got["dlogits"]).double(), ref["dlogits"]
    assert g.shape == r.shape
    if float(r.abs().max()) == 0.0:
        l2 = mx = 0.0 if float(g.abs().max()) == 0.0 else float("inf")
    else:
        l2, mx = float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max())
    out = dict(l2=l2, mx=mx)
    if "metrics" in ref:
        worst = 0.0
        for a, b in zip(got["metrics"], ref["metrics"]):
            a, b = float(a), float(b)
            if math.isnan(a) or math.isnan(b):
                worst = worst if (math.isnan(a) and math.isnan(b)) else float("inf")
            else:
                worst = max(worst, abs(a - b))
        out["met"] = worst
    return out


def over_bars(c, got, ref):
    """The bars `got` misses: [(name, distance, bar)].  A NaN distance misses."""
    bar = bars(c)
    return [(k, v, bar[k]) for k, v in distances(c, got, ref).items() if not v <= bar[k]]


# ==== AdamW ========================================================================================================================
_SPECIAL = (3.0, -3.0, 0.0, 1e-12, -1e-12, 1e-3, -1e-3, 0.999, -0.999, 1.0, -1.0, 1.001, -1.001, 50.0, -50.0)


@functools.lru_cache(maxsize=None)
def adam_inputs(c):
    """{"p", "m", "v": fp32 [n] start state, "g": [fp32 [n]] one gradient per step, "first": the number of the first step}.  The
    gradients hold 0, +-1e-12 (eps dominates), +-1e-3, +-0.999, +-1, +-1.001 and +-50 (the clip at 1) and +-3 (scale 0.25, then
    clip, gives 0.75; clip, then scale, 0.25) four times over, then N(0, 1) x 10^U(-4, 1); each step rolls them by one element."""
    g = torch.Generator().manual_seed(_seed(c))
    n = c.n
    base = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 5.0 - 4.0)
    k = min(n, 4 * len(_SPECIAL))
    base[:k] = torch.tensor((_SPECIAL * 4)[:k])
    if c.p == "zero":
        p = torch.zeros(n)
    else:
        p = torch.randn(n, generator=g)
        small = torch.arange(0, min(n, 64), 8)
        p[small] = 2e-3 * (1.0 + small / 64.0) * (1.0 - 2.0 * ((small // 8) % 2))
    n_steps = c.steps or 1
    grads = [torch.roll(base, s) for s in range(n_steps)]
    if c.steps:
        return dict(p=p, m=torch.zeros(n), v=torch.zeros(n), g=grads, first=1)
    # moments of a run of WARM_STEPS reference steps on other gradients of the same kind, rounded to fp32
    warm = [torch.roll(base, -s - 1) * (1.0 + 0.25 * s) for s in range(WARM_STEPS)]
    st = _torch_adamw(torch.zeros(n, dtype=torch.float64), None, None, 0, warm, c)[-1]
    return dict(p=p, m=st["m"].float(), v=st["v"].float(), g=grads, first=c.step)


def _torch_adamw(p0, m0, v0, steps_done, grads, c):
    """torch.optim.AdamW on fp64 CPU tensors from the given state (moments None: a fresh optimiser), the gradient of each step
    scaled, then clipped by clip_grad_value_, as the trainers do.  [{"p", "m", "v", "gp": the gradient the optimiser saw}] per step."""
    p = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.AdamW([p], lr=LR, betas=(BETA1, BETA2), eps=EPS, weight_decay=c.wd, foreach=False)
    if m0 is not None:
        opt.state[p] = dict(step=torch.tensor(float(steps_done)), exp_avg=m0.clone().double(), exp_avg_sq=v0.clone().double())
    out = []
    for gr in grads:
        p.grad = gr.double() * c.gs
        if c.clip > 0:
            torch.nn.utils.clip_grad_value_([p], c.clip)
        opt.step()
        st = opt.state[p]
        out.append(dict(p=p.detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(), gp=p.grad.clone()))
    return out


@functools.lru_cache(maxsize=None)
def adam_reference(c):
    """The fp64 trajectory: per step {"p", "m", "v", "m_terms"}, never modified.  m_terms is the first moment of |g'| from |m| of the
    start state: the sum of the |terms| of m over all the steps so far, which is what a rounding error of an earlier step is
    carried against (m itself may cancel to nothing)."""
    d = adam_inputs(c)
    traj = _torch_adamw(d["p"], d["m"], d["v"], d["first"] - 1, d["g"], c)
    scale = d["m"].double().abs()
    for st in traj:
        scale = BETA1 * scale + (1.0 - BETA1) * st["gp"].abs()
        st["m_terms"] = scale
    return traj


def adam_compute(c, mutant=None):
    """adamw_kernel in fp32 numpy over the case's steps, the state carried in fp32; like torch, the bias corrections, lr / bc1 and
    sqrt(bc2) in double, and so 1 - beta1 and 1 - beta2.  mutant: None, "clip_first" (clip before scale), "decay_last" (the decay
    after the update), "no_bc2" (sqrt(bc2) dropped), "eps_inside" (eps under the square root), "fp32_betas" (1 - beta and the bias
    corrections formed in fp32 from 0.9f and 0.999f)."""
    d = adam_inputs(c)
    p, m, v = (d[k].numpy().astype(F).copy() for k in ("p", "m", "v"))
    lr, wd, clip, gs, b1, b2, eps = F(LR), F(c.wd), F(c.clip), F(c.gs), F(BETA1), F(BETA2), F(EPS)
    out = []
    for i, g in enumerate(d["g"]):
        step = d["first"] + i
        g = g.numpy().astype(F)
        if mutant == "clip_first":
            gr = (np.clip(g, -clip, clip) if c.clip > 0 else g) * gs
        else:
            gr = g * gs
            if c.clip > 0:
                gr = np.clip(gr, -clip, clip)
        decay = F(1.0) - lr * wd
        if mutant != "decay_last":
            p = p * decay
        if mutant == "fp32_betas":      # everything from 0.9f and 0.999f in fp32, as the kernel's launcher once did
            omb1, omb2 = F(1.0) - b1, F(1.0) - b2
            bc1, bc2 = F(1.0) - np.power(b1, F(step)), F(1.0) - np.power(b2, F(step))
            step_size, bc2_sqrt = lr / bc1, np.sqrt(bc2)
        else:
            omb1, omb2 = F(1.0 - BETA1), F(1.0 - BETA2)
            bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
            step_size, bc2_sqrt = F(float(lr) / bc1), F(1.0 if mutant == "no_bc2" else math.sqrt(bc2))
        m = b1 * m + omb1 * gr
        v = b2 * v + omb2 * gr * gr
        if mutant == "eps_inside":
            denom = np.sqrt(v / (bc2_sqrt * bc2_sqrt) + eps)
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps
        p = p - step_size * (m / denom)
        if mutant == "decay_last":
            p = p * decay
        out.append(dict(p=p.copy(), m=m.copy(), v=v.copy()))
    return out


ADAM_MUTANTS = {
    "clip_first": lambda c: c.gs != 1.0 and c.clip > 0,
    "decay_last": lambda c: c.wd > 0,
    "no_bc2": lambda c: True,
    "eps_inside": lambda c: True,
    "fp32_betas": lambda c: True,
}


def _rel(g, r, scale):
    """max |g - r| / scale over the elements with scale > 0; where scale is 0 the two must be equal (else inf)."""
    g, r = torch.as_tensor(g).double(), r.double()
    pos = scale > 0
    if not torch.equal(g[~pos], r[~pos]):
        return float("inf")
    return float(((g - r).abs()[pos] / scale[pos]).max()) if bool(pos.any()) else 0.0


def adam_distances(got, ref):
    """The worst of the steps: {"p": |delta| / max(|ref|, lr), "m": |delta| / m_terms, "v": |delta| / |ref|}."""
    out = dict(p=0.0, m=0.0, v=0.0)
    for g, r in zip(got, ref):
        out["p"] = max(out["p"], _rel(g["p"], r["p"], r["p"].abs().clamp(min=LR)))
        out["m"] = max(out["m"], _rel(g["m"], r["m"], r["m_terms"]))
        out["v"] = max(out["v"], _rel(g["v"], r["v"], r["v"].abs()))
    return out


def adam_over_bars(got, ref):
    return [(k, v, AD_BAR[k]) for k, v in adam_distances(got, ref).items() if not v <= AD_BAR[k]]
