"""Action masks (``jn_set_rollout_action_mask``, ``jn_action_sets``, ``jn_reinforce_loss_masked``, ``jn_logits_grad_masked``): the rule
of the sets restated in numpy, the masked log-softmax, entropy, REINFORCE loss and gradients in fp64, the case lists and the bars.

Shared by tests/test_action_mask_cases_cpu.py (the restatement has the properties the contract states, the bars mean something on
these inputs, every planted mistake is caught) and tests/test_gpu_action_mask.py.  Fixed seeds, no committed tensors.

The contract.  A set is a uint16, bit a = action a allowed.  For a < 8 with target (y + dy[a], x + dx[a]): inside(a) = the target lies
on the agent's gh x gw grid, fresh(a) = inside(a) and the target is not visited (`visited` before the step's update: the current cell
is marked).  "grid": M = {inside}; "unvisited": M = {fresh}, or {inside} when that is empty.  M still empty (1 x 1): all of 0..7.
nA == 9: STOP (8) is added.  A forced action is added.  Under M, logp = log_softmax over the members' logits, H over the members,
the greedy choice is the first maximum among the members, a sample the inverse CDF over the members in index order (the last member
when none passes).  d logp[a] / d logits_j = [j == a] - p_j and d H / d logits_j = -p_j (logp_j + H) for j in M, exactly 0 outside."""
import collections
import functools
import zlib

import numpy as np
import torch

from jolineedle_amd import ragged
from jolineedle_amd.common import ACTION_DELTAS, Action
from tests import train_cases as tc

F = np.float32
CANARY = tc.CANARY
POLICIES = {"grid": 1, "unvisited": 2}
DY = [ACTION_DELTAS[Action(a)][0] for a in range(9)]
DX = [ACTION_DELTAS[Action(a)][1] for a in range(9)]
TAG_SAMPLE = 0x53414D50
OUTSIDE = 1e30                    # what the loss cases put at every logit outside the set: read once, it spoils every figure


# ==== the rule of the sets ==========================================================================================================
def action_set(policy, y, x, gh, gw, visited, nA, forced=None, mutant=None):
    """The set of one state.  visited: [>= gh, >= gw] array, non-zero = visited.  mutant: None, "no_stop" (STOP bit dropped),
    "no_fallback" (an empty fresh set is not replaced by the inside moves)."""
    assert policy in POLICIES
    inside = fresh = 0
    for a in range(min(nA, 8)):
        ty, tx = y + DY[a], x + DX[a]
        if 0 <= ty < gh and 0 <= tx < gw:
            inside |= 1 << a
            if not visited[ty][tx]:
                fresh |= 1 << a
    if policy == "grid":
        m = inside
    else:
        m = fresh if (fresh or mutant == "no_fallback") else inside
    if not m:
        m = (1 << min(nA, 8)) - 1
    if nA > 8 and mutant != "no_stop":
        m |= 1 << 8
    if forced is not None:
        m |= 1 << int(forced)
    return m


def members(m, nA):
    return [a for a in range(nA) if m >> a & 1]


GRIDS = ((1, 1), (1, 3), (3, 1), (2, 2), (3, 4))
CANVAS = (3, 4)
PATTERNS = ("empty", "full", "ring")      # only the current cell; every cell; the current cell and all its neighbours


def _visited(pattern, y, x, gh, gw, Gh, Gw):
    v = np.zeros((Gh, Gw), dtype=np.uint8)
    if pattern == "full":
        v[:gh, :gw] = 1
    elif pattern == "ring":
        v[max(y - 1, 0):min(y + 2, gh), max(x - 1, 0):min(x + 2, gw)] = 1
    v[y, x] = 1
    return v


@functools.lru_cache(maxsize=None)
def states(canvas=None):
    """Every grid of GRIDS x every position x every pattern.  canvas None: each grid on a canvas of its own size, returned as
    {grid: (positions [n, 2], visited [n, gh, gw])}; a canvas: all of them on that canvas with extents, (positions [69, 2], visited
    [69, Gh, Gw], extents [69, 2]) — the extents are smaller than the canvas for four of the five grids."""
    per, pos_all, vis_all, ext_all = {}, [], [], []
    for gh, gw in GRIDS:
        Gh, Gw = canvas or (gh, gw)
        pos, vis = [], []
        for y in range(gh):
            for x in range(gw):
                for p in PATTERNS:
                    pos.append((y, x)); vis.append(_visited(p, y, x, gh, gw, Gh, Gw))
        per[gh, gw] = (np.array(pos, dtype=np.int64), np.stack(vis))
        pos_all += pos; vis_all += vis; ext_all += [(gh, gw)] * len(pos)
    if canvas is None:
        return per
    return np.array(pos_all, dtype=np.int64), np.stack(vis_all), np.array(ext_all, dtype=np.int32)


def forced_for(n, nA, seed=5):
    return np.random.default_rng(seed + nA).integers(0, nA, size=n).astype(np.int64)


def sets_of(policy, pos, vis, ext, nA, forced=None, mutant=None):
    """uint16 [n]: action_set over arrays (ext None: the whole of vis's grid)."""
    out = np.zeros(len(pos), dtype=np.uint16)
    for i, (y, x) in enumerate(pos.tolist()):
        gh, gw = (vis.shape[1], vis.shape[2]) if ext is None else ext[i].tolist()
        out[i] = action_set(policy, y, x, gh, gw, vis[i], nA, None if forced is None else forced[i], mutant)
    return out


def replay_sets(policy, positions, extents, Gh, Gw, nA, forced=None):
    """The sets of a walk from its own outputs: positions int [B, S + 1, 2]; visited starts with the start cell and gains the cell
    reached by every step.  -> (sets uint16 [B, S], visited-before-step [B, S, Gh, Gw])."""
    positions = np.asarray(positions)
    B, S = positions.shape[0], positions.shape[1] - 1
    sets, seen = np.zeros((B, S), dtype=np.uint16), np.zeros((B, S, Gh, Gw), dtype=np.uint8)
    for b in range(B):
        gh, gw = (Gh, Gw) if extents is None else (int(extents[b][0]), int(extents[b][1]))
        v = np.zeros((Gh, Gw), dtype=np.uint8)
        for t in range(S):
            y, x = int(positions[b, t, 0]), int(positions[b, t, 1])
            v[y, x] = 1
            seen[b, t] = v
            sets[b, t] = action_set(policy, y, x, gh, gw, v, nA, None if forced is None else forced[b][t])
    return sets, seen


# ==== the masked Categorical in fp64 ================================================================================================
def in_set(sets, nA):
    """bool [..., nA] from uint16 [...]."""
    return (np.asarray(sets).astype(np.int64)[..., None] >> np.arange(nA)) & 1 == 1


def parts64(logits, sets):
    """fp64 (logp [..., nA], p, H [...]) of the softmax over the members; logp is -inf and p is 0 outside the set."""
    lg = np.asarray(logits, dtype=np.float64)
    m = in_set(sets, lg.shape[-1])
    z = np.where(m, lg, -np.inf)
    mx = z.max(axis=-1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True))
    logp = z - lse
    p = np.exp(logp)
    H = -np.where(m, p * np.where(m, logp, 0.0), 0.0).sum(axis=-1)
    return logp, p, H


def greedy64(logits, sets):
    """The first maximum among the members."""
    lg = np.asarray(logits, dtype=np.float64)
    return np.argmax(np.where(in_set(sets, lg.shape[-1]), lg, -np.inf), axis=-1)


def sample_uniform(seed, index, t):
    """The uniform of the engine's sampled decision for stream (seed, index) at step t, as fp32."""
    return float(F((ragged._philox4x32(int(seed), int(index), int(t), TAG_SAMPLE, 0)[0] >> 8) * (1.0 / 16777216.0)))


def inverse_cdf64(logits, m, u, nA):
    """(action, distance of u from the nearest CDF boundary) over the members of m in index order; the last member when none passes."""
    _, p, _ = parts64(np.asarray(logits)[None], np.array([m]))
    cdf, act, gap = 0.0, None, float("inf")
    mem = members(int(m), nA)
    for a in mem:
        cdf += float(p[0, a])
        gap = min(gap, abs(u - cdf))
        if act is None and u < cdf:
            act = a
    return (mem[-1] if act is None else act), gap


# ==== loss and gradient cases =======================================================================================================
MCase = collections.namedtuple("MCase", "kind B T nA stop big")
LOSS_CASES = [MCase(k, B, T, nA, stop, big) for k in ("rf", "lg") for (B, T) in ((3, 5), (65, 7)) for nA in (8, 9)
              for stop, big in ((0, 0), (1, 0), (0, 1))]
EW, SCALE = 0.01, 0.5

# The bars, set as tests/train_cases.py sets its own: the plain fp32 restatement below (`compute`), in natural order, against the
# fp64 reference on the cases of this file (test_action_mask_cases_cpu.py prints the figures and holds these to them); the bar is
# 4 x the figure, rounded up to one digit (train_cases.bar_of).  dlogits: relative L2 (l2) and max |delta| / max |ref| (mx);
# metrics: absolute (met).  The logits x 30 cases have bars of their own, as there.
FP32_MEASURED = dict(rf=dict(l2=1.7e-7, mx=2.8e-7, met=1.9e-7), lg=dict(l2=1.4e-7, mx=2.5e-7))
BAR = dict(rf=dict(l2=7e-7, mx=2e-6, met=8e-7), lg=dict(l2=6e-7, mx=1e-6))
BIG_FP32_MEASURED = dict(rf=dict(l2=5.5e-7, mx=1.2e-6, met=3.0e-6), lg=dict(l2=4.4e-7, mx=1.7e-6))
BIG_BAR = dict(rf=dict(l2=3e-6, mx=5e-6, met=2e-5), lg=dict(l2=2e-6, mx=7e-6))


def case_id(c):
    return f"{c.kind}-{c.B}x{c.T}x{c.nA}-stop{c.stop}" + ("-big" if c.big else "")


def bars(c):
    return (BIG_BAR if c.big else BAR)[c.kind]


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's CPU tensors, never modified.  sets: random non-empty subsets, a fifth of them one-element sets, the first token's
    set full; the action of every token is a member; every logit outside the set is OUTSIDE."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(c)).encode()))
    B, T, nA = c.B, c.T, c.nA
    n = B * T
    logits = torch.randn((B, T, nA), generator=g) * (30.0 if c.big else 3.0)
    bits = (torch.rand((n, nA), generator=g) < 0.5)
    one = torch.rand(n, generator=g) < 0.2
    keep = torch.randint(0, nA, (n,), generator=g)
    bits[one] = False
    bits[torch.arange(n), keep] = True                       # never empty; the one-element sets hold `keep` alone
    bits[0] = True
    pick = torch.rand((n, nA), generator=g).masked_fill(~bits, -1.0)
    actions = pick.argmax(dim=1).view(B, T)
    sets = (bits.long() << torch.arange(nA)).sum(dim=1).view(B, T)
    logits = torch.where(bits.view(B, T, nA), logits, torch.full_like(logits, OUTSIDE))
    masks = (torch.rand((B, T), generator=g) > 0.3).to(torch.uint8)
    masks.view(-1)[0], masks.view(-1)[-1] = 1, 0
    S = T - 2 if c.stop else T
    n_done = torch.tensor([B if t >= S else min(t, B - 1) for t in range(T + 1)], dtype=torch.int32) if c.stop else None
    d = dict(logits=logits, actions=actions, sets=sets.numpy().astype(np.uint16), bits=bits.view(B, T, nA).numpy(), masks=masks,
             n_done=n_done, S=S)
    d["returns"], d["rewards"] = torch.randn((B, T), generator=g), torch.randn((B, T), generator=g)
    r = d["returns"].double()
    d["ret_mean"], d["ret_std"], d["ew"] = float(F(r.mean().item())), float(F(r.std().item())), float(F(EW))
    d["dlogprobs"], d["dentropies"] = torch.randn((B, T), generator=g), torch.randn((B, T), generator=g)
    return d


@functools.lru_cache(maxsize=None)
def reference(c):
    """fp64, from the contract's formulas: {"dlogits" [B, T, nA], "metrics" (rf), "sel": the counted tokens}."""
    d = inputs(c)
    B, T, nA = c.B, c.T, c.nA
    executed = np.broadcast_to(np.arange(T)[None, :] < d["S"], (B, T))
    logp, p, H = parts64(d["logits"].numpy(), d["sets"])
    m = d["bits"]
    act = d["actions"].numpy()
    onehot = np.arange(nA)[None, None, :] == act[..., None]
    lpa = np.take_along_axis(logp, act[..., None], axis=-1)[..., 0]
    safe_logp = np.where(m, logp, 0.0)
    d_lp = np.where(m, onehot - p, 0.0)
    d_H = np.where(m, -p * (safe_logp + H[..., None]), 0.0)
    if c.kind == "lg":
        dl = d["dlogprobs"].double().numpy()[..., None] * d_lp + d["dentropies"].double().numpy()[..., None] * d_H
        dl[~executed] = 0.0
        return dict(dlogits=torch.from_numpy(dl), sel=executed)
    sel = (d["masks"].numpy() != 0) & executed
    n = float(sel.sum())
    adv = (d["returns"].double().numpy() - d["ret_mean"]) / (d["ret_std"] + 1e-8)
    action_loss, entropy_loss = (-(lpa * adv))[sel].sum() / n, (-H)[sel].sum() / n
    dl = SCALE / n * (-adv[..., None] * d_lp - d["ew"] * d_H)
    dl[~sel] = 0.0
    metrics = [action_loss, entropy_loss, action_loss + d["ew"] * entropy_loss, d["rewards"].double().numpy()[sel].sum() / B, n / B, float(d["S"])]
    return dict(dlogits=torch.from_numpy(dl), metrics=[float(v) for v in metrics], sel=sel)


MUTANTS = ("set_ignored", "masked_in_max", "entropy_over_all")


def compute(c, mutant=None):
    """The masked kernels restated in plain fp32 numpy, one class after the other.  mutant: None or one of MUTANTS — the set
    ignored altogether, a logit outside the set read into the maximum, the entropy summed over all actions."""
    d = inputs(c)
    B, T, nA = c.B, c.T, c.nA
    n = B * T
    lg = d["logits"].numpy().reshape(n, nA)
    m = np.ones((n, nA), dtype=bool) if mutant == "set_ignored" else d["bits"].reshape(n, nA)
    t = np.arange(n) % T
    with np.errstate(all="ignore"):
        mx = np.full(n, -np.inf, dtype=F)
        for j in range(nA):
            mx = np.where(m[:, j] | (mutant == "masked_in_max"), np.maximum(mx, lg[:, j]), mx)
        se = np.zeros(n, dtype=F)
        for j in range(nA):
            se = np.where(m[:, j], se + np.exp(lg[:, j] - mx), se)
        lse = mx + np.log(se)
        lp = (lg - lse[:, None]).astype(F)
        p = np.exp(lp)
        H = np.zeros(n, dtype=F)
        for j in range(nA):
            H = np.where(m[:, j] | (mutant == "entropy_over_all"), H - lp[:, j] * p[:, j], H)
        act = d["actions"].numpy().reshape(n)
        onehot = (np.arange(nA)[None, :] == act[:, None]).astype(F)
        if c.kind == "lg":
            glp, gh = d["dlogprobs"].numpy().reshape(n), d["dentropies"].numpy().reshape(n)
            dl = glp[:, None] * (onehot - p) - gh[:, None] * p * (lp + H[:, None])
            dl = np.where(m, dl, F(0.0))
            dl[t >= d["S"]] = 0.0
            return dict(dlogits=dl.reshape(B, T, nA))
        sel = (d["masks"].numpy().reshape(n) != 0) & (t < d["S"])
        msum = F(sel.sum())
        adv = (d["returns"].numpy().reshape(n) - F(d["ret_mean"])) / (F(d["ret_std"]) + F(1e-8))
        k = F(SCALE) / msum
        dl = k * (-adv[:, None] * (onehot - p) + F(d["ew"]) * p * (lp + H[:, None]))
        dl = np.where(m, dl, F(0.0))
        dl[~sel] = 0.0
        la = tc._seqsum((-(lp[np.arange(n), act]) * adv)[sel])
        le = tc._seqsum((-H)[sel])
        lr = tc._seqsum(d["rewards"].numpy().reshape(n)[sel])
        m0, m1 = la / msum, le / msum
        metrics = [m0, m1, m0 + F(d["ew"]) * m1, lr / F(B), msum / F(B), F(d["S"])]
        return dict(dlogits=dl.reshape(B, T, nA), metrics=[float(v) for v in metrics])


def distances(c, got, ref):
    return tc.distances(c, got, ref)


def over_bars(c, got, ref):
    """The bars `got` misses: [(name, distance, bar)].  A NaN distance misses."""
    bar = bars(c)
    return [(k, v, bar[k]) for k, v in distances(c, got, ref).items() if not v <= bar[k]]
