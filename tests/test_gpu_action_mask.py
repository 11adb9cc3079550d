"""Action masks on the GPU (``jn_set_rollout_action_mask``): the set kernel against the numpy restatement bit for bit, masked rollouts
on both decision routes checked from their own outputs (sets, membership, moves, log-probs, entropies, greedy and sampled choices),
the default path's bits after arming and disarming, the masked loss and gradient kernels against fp64 with the bars of
tests/action_mask_cases.py, and a masked training iteration against a torch-CPU graph of the oracle.  64-px patches, tiny models."""
import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, ragged
from jolineedle_amd._lib import check, ptr
from oracle import env_ref, gpt_ref, rollout_ref
from tests import action_mask_cases as am
from tests.helpers import make_pair, model_config, randomize_bn, synth_batch
from tests.test_action_mask_cases_cpu import CDF_MARGIN, SAMPLE_SEEDS
from tests.test_gpu_parity import _check_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, T = 64, 6
GRID = (3, 4)
LOGP_BAR = 1e-5                      # tests/test_gpu_parity.py holds the unmasked log-probs and entropies to the same
gpt_ref.GPT_ZOO.setdefault("narrow-128", (2, 4, 128))
DIMS = {"per-agent": ("gpt-nano", (3, 3, 48), 0), "wide": ("narrow-128", (2, 4, 128), 1)}      # name, (layers, heads, n_embd), route
BASE = dict(patch_size=P, block_size=T, gpt_backbone="yolox-nano", image_processor=None, with_detector=False)
SIZES = [(100, 150), (150, 120), (130, 190), (120, 100), (64, 64), (60, 200), (190, 50)]         # ragged images: grids 1 x 1 .. 3 x 3


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _u16(t):
    """uint16 values of a device tensor that holds them as int16 bit patterns."""
    return (t.cpu().to(torch.int64) & 0xFFFF).numpy().astype(np.uint16)


# ---- 1. the set kernel ----------------------------------------------------------------------------------------------------------
def _sets_on_device(policy, pos, vis, ext, nA, forced):
    n, (Gh, Gw) = len(pos), vis.shape[1:]
    out = torch.full((n + 1,), -1, device=DEV, dtype=torch.int16)                    # one canary element behind the sets
    pos_d, vis_d = _dev(pos), _dev(vis)                                              # (named: alive until the launch has run)
    ext_d, forced_d = None if ext is None else _dev(ext), None if forced is None else _dev(forced)
    assert pos_d.dtype == torch.int64 and vis_d.dtype == torch.uint8 and (ext_d is None or ext_d.dtype == torch.int32)
    check(_lib.load_library().jn_action_sets(ptr(pos_d), ptr(vis_d), ptr(ext_d), ptr(forced_d), n, Gh, Gw, am.POLICIES[policy], nA,
                                             ptr(out), _stream()), "jn_action_sets")
    torch.cuda.synchronize()
    assert int(out[n]) == -1
    return _u16(out[:n])


@pytest.mark.parametrize("use_forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("nA", [8, 9])
@pytest.mark.parametrize("policy", list(am.POLICIES))
def test_action_sets_kernel_equals_the_restatement_bit_for_bit(policy, nA, use_forced):
    pos, vis, ext = am.states(am.CANVAS)                                              # every grid on the 3 x 4 canvas, with extents
    forced = am.forced_for(len(pos), nA) if use_forced else None
    for n in (65, len(pos)):
        f = None if forced is None else forced[:n]
        got = _sets_on_device(policy, pos[:n], vis[:n], ext[:n], nA, f)
        assert np.array_equal(got, am.sets_of(policy, pos[:n], vis[:n], ext[:n], nA, f)), n
    for grid, (gpos, gvis) in am.states().items():                                   # each grid as its own canvas, no extents
        f = None if forced is None else forced[:len(gpos)]
        assert np.array_equal(_sets_on_device(policy, gpos, gvis, None, nA, f), am.sets_of(policy, gpos, gvis, None, nA, f)), grid


# ---- 2. rollouts ------------------------------------------------------------------------------------------------------------------
def _new_product(route):
    """An eval-mode decision model on `route` in a context of its own, room for 65 agents."""
    name, (n_layer, n_head, n_embd), want = DIMS[route]
    oracle = gpt_ref.build_gpt_ref(5, model_type=name, **BASE)
    randomize_bn(oracle, 5)
    with torch.no_grad():                           # logits about a unit apart, so that the decisions differ from agent to agent
        oracle.action_head.lm_heads[0].weight.mul_(10.0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("JN_GPT_WIDE", "1") if want else mp.delenv("JN_GPT_WIDE", raising=False)
        product = ja.GPT(model_config(**dict(BASE, model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd)), max_batch=65)
    eng = product.engine()
    assert eng.lib.jn_debug_decision_route(eng.handle) == want
    product.load_state_dict(oracle.state_dict())
    return product.eval()


@pytest.fixture(scope="module")
def products():
    return {route: _new_product(route) for route in DIMS}


def _cfg(seed=1, stop=True, **kw):
    return ja.CfgNode(max_seq_len=T, entropy_weight=0.01, stop_enabled=stop, reward_norm=True, seed=seed, patch_size=P, **kw)


def _batch(B, ragged_batch, tr):
    """(env, extents [B, 2] or None, canvas grid, start positions) of B agents: a 3 x 4 grid, or images of SIZES on their canvas."""
    g = torch.Generator().manual_seed(100 + B)
    if not ragged_batch:
        images, bboxes, _ = synth_batch(B, *GRID, P, seed=31)
        start = torch.stack((torch.randint(0, GRID[0], (B,), generator=g), torch.randint(0, GRID[1], (B,), generator=g)), 1)
        return ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, True), None, GRID, start
    imgs = [torch.rand((3, *SIZES[i % len(SIZES)]), generator=g) for i in range(B)]
    rows = [torch.tensor([[5, 5, 40, 40]]) for _ in range(B)]
    env = ragged.image_env(tr, imgs, rows)
    ext = np.asarray(env.grid_extents.tolist() if torch.is_tensor(env.grid_extents) else env.grid_extents, dtype=np.int64)
    start = torch.stack([torch.tensor([int(torch.randint(0, int(e[0]), (1,), generator=g)), int(torch.randint(0, int(e[1]), (1,), generator=g))])
                         for e in ext])
    return env, ext, (env.n_vertical_patches, env.n_horizontal_patches), start


def _check_rollout(ro, policy, mode, ext, canvas, nA, forced, seed):
    """Every check of a masked rollout, from its own outputs.  Returns (pairs left out of the sampled check, pairs)."""
    sets = ro["action_sets"].cpu().numpy().astype(np.uint16)
    pos, act = ro["positions"].cpu().numpy(), ro["actions"].cpu().numpy()
    logits = ro["logits"].cpu().numpy()
    B, S = act.shape
    assert sets.shape == (B, S) and S == T
    want, seen = am.replay_sets(policy, pos, ext, *canvas, nA, None if forced is None else forced.numpy())
    assert np.array_equal(sets, want)                                                 # the sets are those of the states the walk saw
    member = am.in_set(sets, nA)
    assert np.take_along_axis(member, act[..., None], axis=-1).all()                  # every chosen action is in its set
    logp, p, H = am.parts64(logits, sets)
    lpa = np.take_along_axis(logp, act[..., None], axis=-1)[..., 0]
    d_lp = np.abs(ro["logprobs"].cpu().numpy().astype(np.float64) - lpa).max()
    d_H = np.abs(ro["entropies"].cpu().numpy().astype(np.float64) - H).max()
    print(f"{policy} {mode} B={B}: log-probs {d_lp:.2e}, entropies {d_H:.2e} from the fp64 masked log-softmax")
    assert d_lp < LOGP_BAR and d_H < LOGP_BAR
    out = 0
    for b in range(B):
        gh, gw = canvas if ext is None else (int(ext[b][0]), int(ext[b][1]))
        for t in range(S):
            a, (y, x), (ny, nx) = int(act[b, t]), pos[b, t], pos[b, t + 1]
            if mode != "forced" and a != 8 and (gh, gw) != (1, 1):                   # (a 1 x 1 grid has nowhere to go: every move is allowed)
                assert (int(ny - y), int(nx - x)) == (am.DY[a], am.DX[a]), (b, t, a)  # no move is clamped
                if policy == "unvisited":
                    fresh = [m for m in range(8) if 0 <= y + am.DY[m] < gh and 0 <= x + am.DX[m] < gw and not seen[b, t][y + am.DY[m], x + am.DX[m]]]
                    assert not fresh or not seen[b, t][ny, nx], (b, t, a)            # no cell twice while a fresh neighbour existed
            if mode == "greedy":
                assert a == int(am.greedy64(logits[b, t].astype(np.float32), sets[b, t])), (b, t)
            elif mode == "forced":
                assert a == int(forced[b, t])
            else:
                want_a, gap = am.inverse_cdf64(logits[b, t], int(sets[b, t]), am.sample_uniform(seed, b, t), nA)
                if gap < CDF_MARGIN:
                    out += 1
                else:
                    assert a == want_a, (b, t, a, want_a, gap)
    return out, B * S


@pytest.mark.parametrize("ragged_batch", [False, True], ids=["grid3x4", "ragged"])
@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("route", list(DIMS))
def test_masked_rollouts_decide_inside_their_sets(products, route, B, ragged_batch):
    product, nA = products[route], 9
    left_out = pairs = 0
    with torch.no_grad():
        for policy in am.POLICIES:
            for k, mode in enumerate(("greedy", "sample", "forced")):
                tr = ja.ReinforceTrainer(_cfg(seed=k + 1), product)
                env, ext, canvas, start = _batch(B, ragged_batch, tr)
                forced = torch.randint(0, nA, (B, T), generator=torch.Generator().manual_seed(7)) if mode == "forced" else None
                ro = tr.rollout(env, sample_actions=mode == "sample", forced_actions=forced, start_positions=start, stop_early=False,
                                keep_patches=False, action_mask=policy)
                seed = ragged.rollout_seed(tr, tr._rollouts)
                assert mode != "sample" or seed in SAMPLE_SEEDS
                o, n = _check_rollout(ro, policy, mode, ext, canvas, nA, forced, seed)
                left_out, pairs = left_out + o, pairs + (n if mode == "sample" else 0)
    print(f"{route} B={B}: {left_out} of {pairs} sampled pairs within {CDF_MARGIN:g} of a CDF boundary")
    assert left_out * 100 <= pairs


def test_a_one_element_set_has_log_prob_zero_and_entropy_zero():
    """A 1 x 2 grid without STOP under "grid": one move stays inside."""
    product, _ = make_pair(5, patch_size=P, block_size=T, nclasses=8, with_detector=False, image_processor=None)
    images, bboxes, _ = synth_batch(2, 1, 2, P, seed=31)
    tr = ja.ReinforceTrainer(_cfg(stop=False), product.eval())
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T, 1, False)
    with torch.no_grad():
        ro = tr.rollout(env, sample_actions=True, start_positions=torch.tensor([[0, 0], [0, 1]]), stop_early=False, keep_patches=False,
                        action_mask="grid")
    sets, act = ro["action_sets"].cpu(), ro["actions"].cpu()
    assert set(sets.flatten().tolist()) == {1 << 0, 1 << 1}                           # LEFT or RIGHT alone
    assert torch.equal(act, torch.where(sets == 2, 1, 0))
    assert float(ro["logprobs"].abs().max()) == 0.0 and float(ro["entropies"].abs().max()) == 0.0


def test_keyword_reaches_the_chunked_rollouts_and_inference(products):
    product = products["per-agent"]
    g = torch.Generator().manual_seed(3)
    imgs = [torch.rand((3, *SIZES[i]), generator=g) for i in range(4)]
    rows = [torch.tensor([[5, 5, 40, 40]]) for _ in imgs]
    with torch.no_grad():
        tr = ja.ReinforceTrainer(_cfg(), product)
        for ch in ragged.rollout_chunks(tr, imgs, rows, 3, sample_actions=True, action_mask="grid"):
            ro, ext = ch["rollout"], np.asarray(ch["extents"])
            canvas = (ch["env"].n_vertical_patches, ch["env"].n_horizontal_patches)
            want, _ = am.replay_sets("grid", ro["positions"].cpu().numpy(), ext, *canvas, 9)
            assert np.array_equal(ro["action_sets"].cpu().numpy(), want)
        assert "action_sets" not in next(iter(ragged.rollout_chunks(tr, imgs, rows, 3)))["rollout"]
        cfg = _cfg(action_mask="unvisited")                                           # None reads config.action_mask
        ro = ja.ReinforceTrainer(cfg, product).rollout(_batch(3, False, None)[0], keep_patches=False)
        assert "action_sets" in ro
        res = ja.infer_images(ja.ReinforceTrainer(_cfg(), product), imgs, sample_actions=True, do_detection=False, batch_size=2,
                              action_mask="grid")
        assert len(res["positions"]) == 4
        with pytest.raises(ValueError, match="action_mask"):
            tr.rollout(_batch(3, False, None)[0], action_mask="border")


# ---- 3. the default keeps its bits ------------------------------------------------------------------------------------------------
KEYS = ("rewards", "returns", "logprobs", "entropies", "masks", "logit_masks", "positions", "actions", "logits", "final_emb")


@pytest.mark.parametrize("route", list(DIMS))
def test_a_context_that_armed_and_disarmed_gives_the_bits_of_one_that_never_armed(route):
    def run(model, mask=None):
        tr = ja.ReinforceTrainer(_cfg(seed=4), model)
        env, _, _, start = _batch(3, False, tr)
        with torch.no_grad():
            return tr.rollout(env, sample_actions=True, start_positions=start, stop_early=False, keep_patches=False, action_mask=mask)
    never = run(_new_product(route))                                                  # a context that never armed
    other = _new_product(route)
    for mask in am.POLICIES:
        armed = run(other, mask)
        assert "action_sets" in armed and not torch.equal(armed["logprobs"], never["logprobs"])
        after = run(other)
        assert "action_sets" not in after
        for k in KEYS:
            assert torch.equal(never[k], after[k]), (mask, k)
    eng = other.engine()                                                              # armed and disarmed at the library, no rollout between
    assert eng.lib.jn_set_rollout_action_mask(eng.handle, 2, None) == 0 and eng.lib.jn_set_rollout_action_mask(eng.handle, 0, None) == 0
    again = run(other)
    for k in KEYS:
        assert torch.equal(never[k], again[k]), k


# ---- 4. the masked loss and gradient kernels ----------------------------------------------------------------------------------------
def _run_loss_case(c, sets, masked=True, logits=None):
    d = am.inputs(c)
    lib = _lib.load_library()
    B, T_, nA = c.B, c.T, c.nA
    lg, act = _dev(d["logits"] if logits is None else logits), _dev(d["actions"])
    nd = None if d["n_done"] is None else _dev(d["n_done"])
    dl = torch.full((B * T_ + 1, nA), am.CANARY, device=DEV)                         # one canary row behind the gradient
    st = None if sets is None else _dev(sets.astype(np.int16))
    if c.kind == "rf":
        met = torch.full((8,), am.CANARY, device=DEV)
        ret, rew, mk = _dev(d["returns"]), _dev(d["rewards"]), _dev(d["masks"])      # (named: alive until the launch has run)
        args = (ptr(lg), ptr(act), ptr(ret), ptr(rew), ptr(mk), ptr(nd), B, T_, nA, 1, d["ret_mean"], d["ret_std"], d["ew"], am.SCALE,
                ptr(dl), ptr(met))
        if masked:
            check(lib.jn_reinforce_loss_masked(*args, ptr(st), _stream()), "jn_reinforce_loss_masked")
        else:
            check(lib.jn_reinforce_loss(*args, _stream()), "jn_reinforce_loss")
    else:
        met = None
        glp, gh = _dev(d["dlogprobs"]), _dev(d["dentropies"])
        args = (ptr(lg), ptr(act), ptr(glp), ptr(gh), ptr(nd), B, T_, nA, ptr(dl))
        if masked:
            check(lib.jn_logits_grad_masked(*args, ptr(st), _stream()), "jn_logits_grad_masked")
        else:
            check(lib.jn_logits_grad(*args, _stream()), "jn_logits_grad")
    torch.cuda.synchronize()
    assert bool((dl[B * T_] == am.CANARY).all()) and (met is None or bool((met[6:] == am.CANARY).all()))
    out = dict(dlogits=dl[:B * T_].view(B, T_, nA).cpu())
    if met is not None:
        out["metrics"] = met[:6].cpu().tolist()
    return out


@pytest.mark.parametrize("c", am.LOSS_CASES, ids=[am.case_id(c) for c in am.LOSS_CASES])
def test_masked_loss_and_gradient_kernels_meet_their_bars(c):
    d, ref = am.inputs(c), am.reference(c)
    got = _run_loss_case(c, d["sets"])
    dist = am.distances(c, got, ref)
    print(am.case_id(c), {k: f"{v:.2e}" for k, v in dist.items()}, "bars", am.bars(c))
    assert not am.over_bars(c, got, ref), am.over_bars(c, got, ref)
    dl = got["dlogits"].numpy()
    assert (dl[~d["bits"]] == 0).all()                                                # exactly zero outside the set (the logit there is 1e30)
    assert (dl[~ref["sel"]] == 0).all()                                               # uncounted rows
    assert np.isfinite(dl).all()


@pytest.mark.parametrize("c", [c for c in am.LOSS_CASES if not c.big], ids=[am.case_id(c) for c in am.LOSS_CASES if not c.big])
def test_all_ones_sets_give_the_bits_of_the_unmasked_entries(c):
    """(on the case's logits with the 1e30 entries replaced: a full set reads them all)"""
    d = am.inputs(c)
    lg = torch.where(torch.from_numpy(d["bits"]), d["logits"], torch.full_like(d["logits"], -1.5))
    full = np.full((c.B, c.T), (1 << c.nA) - 1, dtype=np.uint16)
    a, b = _run_loss_case(c, full, logits=lg), _run_loss_case(c, None, masked=False, logits=lg)
    assert torch.equal(a["dlogits"], b["dlogits"])
    assert a.get("metrics") == b.get("metrics")


# ---- 5. training under "grid" -------------------------------------------------------------------------------------------------------
def _masked_oracle_grads(oracle, images, bboxes, start, forced, sets, Tn, mean, std, ew):
    """A train-mode REINFORCE iteration on the CPU oracle, GPT.forward step by step as oracle/rollout_ref.py walks it, with the
    log-softmax and the entropy over the members of the engine's sets [B, Tn]."""
    oracle.train()
    oracle.zero_grad()
    env = env_ref.EnvRef(images, bboxes, P, Tn, 1, True)
    B = env.batch_size
    member = torch.from_numpy(am.in_set(sets, 9))
    actions, classes = torch.zeros((B, 1), dtype=torch.long), torch.zeros((B,), dtype=torch.long)
    patches, infos = env.reset(start)
    positions = infos["positions"].unsqueeze(1)
    masks, rewards, logprobs, entropies, emb = [torch.ones(B, dtype=torch.bool)], [], [], [], None
    for t in range(Tn):
        logits, emb = oracle(patches, actions, classes, positions, emb)
        m = member[:, t]
        logp = torch.log_softmax(logits[:, -1].masked_fill(~m, float("-inf")), dim=-1)
        safe = torch.where(m, logp, torch.zeros_like(logp))
        logprobs.append(safe.gather(1, forced[:, t:t + 1]).squeeze(1))
        entropies.append(-(safe.exp() * safe * m).sum(-1))
        new_patches, r, terminated, truncated, infos = env.step(forced[:, t])
        rewards.append(r); masks.append(~terminated)
        actions = torch.cat((actions, forced[:, t:t + 1]), dim=1)
        patches = torch.cat((patches, new_patches), dim=1)
        positions = torch.cat((positions, infos["positions"][:, None]), dim=1)
        if bool(torch.all(terminated | truncated)):
            break
    rewards, masks = torch.stack(rewards, 1), torch.stack(masks, 1)
    logit_masks, returns = rollout_ref.discounted_returns(rewards, masks)
    ro = {"rewards": rewards, "returns": returns, "logprobs": torch.stack(logprobs, 1), "entropies": torch.stack(entropies, 1),
          "logit_masks": logit_masks, "positions": positions}
    norm = rollout_ref.ReturnNormaliser()
    norm.mean, norm.std = mean, std
    metrics = rollout_ref.reinforce_metrics(ro, ew, norm)
    metrics["loss"].backward()
    return ro, metrics


def _forced_inside(start, B, Tn, seed=3):
    """Forced moves that stay on the 3 x 4 grid (each inside its own "grid" set), never STOP."""
    rng = np.random.default_rng(seed)
    pos, out = start.numpy().copy(), np.zeros((B, Tn), dtype=np.int64)
    for t in range(Tn):
        for b in range(B):
            inside = [a for a in range(8) if 0 <= pos[b, 0] + am.DY[a] < GRID[0] and 0 <= pos[b, 1] + am.DX[a] < GRID[1]]
            a = int(rng.choice(inside))
            out[b, t] = a
            pos[b] += (am.DY[a], am.DX[a])
    return torch.from_numpy(out)


def test_masked_training_iteration_and_bridge_gradients_vs_oracle():
    B, Tn, mean, std, ew = 4, 3, 0.25, 1.5, 0.01
    product, oracle = make_pair(5, patch_size=P, block_size=Tn, nclasses=9, with_detector=False, image_processor=None)
    images, bboxes, start = synth_batch(B, *GRID, P, seed=41)
    start[0] = torch.tensor([0, 0])                                                   # a corner: three of the eight moves stay inside
    forced = _forced_inside(start, B, Tn)
    cfg = ja.CfgNode(max_seq_len=Tn, entropy_weight=ew, stop_enabled=True, reward_norm=True, seed=1, learning_rate=1e-3,
                     gradient_accumulation=1, patch_size=P, detection_enabled=False)
    tr = ja.ReinforceTrainer(cfg, product)
    tr.last_return_mean, tr.last_return_std = mean, std
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    got_m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False, action_mask="grid")
    S = int(got_m["steps"])
    sets = _u16(tr._last_action_sets)[:, :S]
    want_sets, _ = am.replay_sets("grid", tr._last_train_buffers["positions"][:, :S + 1].cpu().numpy(), None, *GRID, 9, forced.numpy())
    assert np.array_equal(sets, want_sets) and (sets != 0x1FF).any() and bin(int(sets[0, 0])).count("1") == 4
    ro, m = _masked_oracle_grads(oracle, images, bboxes, start, forced, sets, Tn, mean, std, ew)
    assert ro["logprobs"].shape[1] == S
    for k in ("action_loss", "entropy_loss", "loss", "returns", "episode_length"):
        assert abs(float(got_m[k]) - float(m[k].detach())) < 2e-4, (k, float(got_m[k]), float(m[k].detach()))
    # the unmasked loss is another number: the mask is not a no-op on this batch
    plain = rollout_ref.rollout(oracle, env_ref.EnvRef(images, bboxes, P, Tn, 1, True), forced_actions=forced, start_positions=start)
    assert float((plain["logprobs"].detach() - ro["logprobs"].detach()).abs().max()) > 0.1
    assert _check_grads(product.engine_grads(), oracle, tag="masked reinforce, train_iteration") > 150

    # the same gradients through the autograd bridge: training_step's backward goes through the masked logits_grad
    product2, _ = make_pair(5, patch_size=P, block_size=Tn, nclasses=9, with_detector=False, image_processor=None)
    tr2 = ja.ReinforceTrainer(cfg, product2)
    tr2.last_return_mean, tr2.last_return_std = mean, std
    seen = {}

    class Recorder:                                                                   # stands in for the optimiser: keeps param.grad
        def step(self):
            seen.update({n: p.grad.detach().clone().cpu() for n, p in product2.named_parameters() if p.grad is not None})

        def zero_grad(self):
            pass
    tr2.training_step({"image": images.to(DEV), "bboxes": bboxes}, Recorder(), None, sync_gradients=False, forced_actions=forced,
                      start_positions=start, action_mask="grid")
    assert float(max(g.abs().max() for g in seen.values())) < 1.0                    # (clip_grad_value_(1) left them as they were)
    assert _check_grads(seen, oracle, tag="masked reinforce, training_step") > 150


def test_arming_between_a_forward_and_its_backward_makes_the_forward_stale():
    B, Tn = 2, 3
    product, _ = make_pair(5, patch_size=P, block_size=Tn, nclasses=9, with_detector=False, image_processor=None)
    images, bboxes, start = synth_batch(B, *GRID, P, seed=41)
    tr = ja.ReinforceTrainer(ja.CfgNode(max_seq_len=Tn, entropy_weight=0.01, stop_enabled=True, reward_norm=False, seed=1), product)
    product.train()
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    ro = tr.rollout(env, start_positions=start, keep_patches=False, action_mask="grid")     # disarmed on the way out: still fresh
    eng = product.engine()
    assert eng.lib.jn_set_rollout_action_mask(eng.handle, 1, None) == 0
    assert eng.lib.jn_set_rollout_action_mask(eng.handle, 0, None) == 0
    with pytest.raises(_lib.JnError, match="jn_reinforce_backward needs a preceding"):
        ro["logprobs"].sum().backward()
