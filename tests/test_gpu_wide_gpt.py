"""The wide decision route (kernels_gptwide.hip: every Linear one skinny GEMM over all agents) on the GPU:
  (a) route against route — the same weights of an admitted narrow model in two contexts, one created under
      JN_GPT_WIDE=1: integers identical, floats within the project's 1e-4 bar of each other and of the oracle;
  (b) wide models (n_embd 320 and the zoo's gopher-44m, gpt2) against the CPU oracle, and run-to-run determinism;
  (c) training of a wide model: REINFORCE, supervised, dropout with injected masks, one AdamW step, the refusal of a
      sequence length the batched backward does not take.
64-px patches, yolox-nano patch encoder, no detector, T <= 4 throughout."""
import functools

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd._lib import JnError
from oracle import env_ref, gpt_ref, rollout_ref
from tests.helpers import model_config, randomize_bn, synth_batch, synth_tokens
from tests.test_gpu_parity import TOL_LOGIT, _check_grads, _oracle_reinforce_grads, build_like

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 64
BASE = dict(patch_size=P, gpt_backbone="yolox-nano", image_processor=None, with_detector=False)
PER_AGENT, WIDE = 0, 1
# an odd-sized wide model: K = 320 is no power of two, five column tiles of 64, N = 960 / 1280
gpt_ref.GPT_ZOO["wide-320"] = (2, 5, 320)
gpt_ref.GPT_ZOO["narrow-128"] = (2, 4, 128)
DIMS = {"wide-320": (2, 5, 320), "narrow-128": (2, 4, 128), "gpt-mini": (6, 6, 192), "gopher-44m": (8, 16, 512),
        "gpt2": (12, 12, 768)}
SAMPLE_SEED = 1          # the trainer seed of the sampled route-to-route rollout (checked: both routes draw the same walks)
# image seeds whose oracle greedy top-2 logit margin exceeds 1e-3 at every step (CPU: 8.8e-2 and 1.7e-2; the test asserts it)
GREEDY_BATCH_SEED = {"wide-320": 31, "gopher-44m": 34}


def _cfg(**kw):
    return ja.CfgNode(max_seq_len=kw.pop("T"), entropy_weight=0.01, stop_enabled=True, reward_norm=True, seed=kw.pop("seed", 1), **kw)


@functools.lru_cache(maxsize=None)
def _oracle(name, seed, kw_items):
    o = gpt_ref.build_gpt_ref(seed, model_type=name, **dict(BASE, **dict(kw_items)))
    randomize_bn(o, 5)
    return o.eval()


def _product(name, oracle, monkeypatch, wide, max_batch, **kw):
    """The engine side of `oracle`: by its dimensions (model_type=None), on the route asked for."""
    n_layer, n_head, n_embd = DIMS[name]
    if wide:
        monkeypatch.setenv("JN_GPT_WIDE", "1")
    else:
        monkeypatch.delenv("JN_GPT_WIDE", raising=False)
    cfg = model_config(**dict(BASE, model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd, **kw))
    product = ja.GPT(cfg, max_batch=max_batch)
    monkeypatch.delenv("JN_GPT_WIDE", raising=False)
    eng = product.engine()
    assert eng.lib.jn_debug_decision_route(eng.handle) == (WIDE if wide or n_embd > 256 else PER_AGENT)
    product.load_state_dict(oracle.state_dict())
    return product


def _kw(**kw):
    return tuple(sorted(kw.items()))


def _compare_rollouts(a, b, bar, tag):
    """Integers exact, floats within `bar`; returns the largest float distance."""
    worst = 0.0
    assert a["rewards"].shape == b["rewards"].shape, (tag, a["rewards"].shape, b["rewards"].shape)      # the same n_done
    for k in ("masks", "logit_masks", "positions", "actions", "rewards"):
        assert torch.equal(a[k].cpu(), b[k].cpu() if torch.is_tensor(b[k]) else b[k]), (tag, k)
    for k in ("returns", "logprobs", "entropies", "logits"):
        d = float((a[k].cpu() - b[k].cpu()).abs().max())
        print(f"{tag}: {k}: max distance {d:.3e}")
        worst = max(worst, d)
        assert d < bar, (tag, k, d)
    return worst


# ---- (a) route against route ------------------------------------------------------------------------------------------
def _env_state(env):
    """What a rollout leaves in its env: (visited grid, last positions), copied to the host at once — the state lives in
    the model's context, and the next env bound to that model takes its place."""
    torch.cuda.synchronize()
    return env.visited_patches.cpu().bool().clone(), env.positions.cpu().long().clone()


def _same_env_state(a, b, tag):
    assert torch.equal(a[0], b[0]), (tag, "visited")
    assert torch.equal(a[1], b[1]), (tag, "env positions")


def _n_done(ro):
    """Finished agents after every executed step (what the skip path reads): from the masks; the step count is the shape."""
    return (~ro["masks"].cpu().bool()).sum(0)


def _route_vs_route_rollouts(name, B, monkeypatch, **arch):
    Tn = 4
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(9))
    forced[:, 2] = 8                             # every agent stops at step 2: step 3 takes the skip path of every launch
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    for tp in ("recurrent", "sequence"):
        kw = dict(block_size=Tn, no_recurrent_embedding=tp == "sequence", **arch)
        oracle = _oracle(name, 5, _kw(**kw))
        envo = env_ref.EnvRef(images, bboxes, P, Tn, 1, True)
        with torch.no_grad():
            ref = rollout_ref.rollout(oracle, envo, forced_actions=forced, start_positions=start, stop_early=True)
        assert ref["rewards"].shape[1] == 3
        ros, envs = {}, {}
        for wide in (False, True):
            product = _product(name, oracle, monkeypatch, wide, B, **kw)
            envs[wide] = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
            tr = ja.ReinforceTrainer(_cfg(T=Tn), product)
            ros[wide] = tr.rollout(envs[wide], forced_actions=forced, start_positions=start, token_positions=tp)
            tag = f"{name} B={B} {tp} {'wide' if wide else 'per-agent'} vs oracle"
            _compare_rollouts(ros[wide], ref, TOL_LOGIT, tag)
            envs[wide] = _env_state(envs[wide])
            assert torch.equal(envs[wide][0], envo.visited_patches.bool()), (tag, "visited")
            assert torch.equal(envs[wide][1], envo.positions.long()), (tag, "env positions")
            assert torch.equal(_n_done(ros[wide]), _n_done(ref)), (tag, "n_done")
            if tp == "recurrent":                # a sampled rollout: the same draws on the same probabilities
                tr_s = ja.ReinforceTrainer(_cfg(T=Tn, seed=SAMPLE_SEED), product)
                env_s = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
                ros[("sample", wide)] = tr_s.rollout(env_s, sample_actions=True, start_positions=start)
                envs[("sample", wide)] = _env_state(env_s)
        d = _compare_rollouts(ros[True], ros[False], TOL_LOGIT, f"{name} B={B} {tp} route to route")
        _same_env_state(envs[True], envs[False], f"{name} B={B} {tp} route to route")
        assert torch.equal(_n_done(ros[True]), _n_done(ros[False]))
        print(f"{name} B={B} {tp}: measured route-to-route distance {d:.3e}")
        if tp == "recurrent":
            sa, sb = ros[("sample", True)], ros[("sample", False)]
            assert sa["rewards"].shape == sb["rewards"].shape
            for k in ("actions", "positions", "masks", "rewards"):
                assert torch.equal(sa[k].cpu(), sb[k].cpu()), ("sampled", k)
            assert torch.equal(_n_done(sa), _n_done(sb))
            _same_env_state(envs[("sample", True)], envs[("sample", False)], f"{name} B={B} sampled")
            assert len(set(sa["actions"].cpu().flatten().tolist())) > 2          # a walk, not a constant


@pytest.mark.parametrize("B", [3, 65])           # rows no multiple of 16; a second row block
@pytest.mark.parametrize("name", ["narrow-128", "gpt-mini"])
def test_rollouts_agree_between_the_routes_and_with_the_oracle(name, B, monkeypatch):
    _route_vs_route_rollouts(name, B, monkeypatch)


# the embedding's other branches: the mean merge with learned positions and no 2-D rows (two parts + the patch), concat
# over three parts (the layout of the GEMM's operand changes), and no patch embedding at all
@pytest.mark.parametrize("arch", [dict(concat_emb=False, decoder_pos_encoding=False, use_pos_emb=False),
                                  dict(concat_emb=True, use_pos_emb=False),
                                  dict(concat_emb=True, no_patch_emb=True),
                                  dict(concat_emb=False, no_patch_emb=True, decoder_pos_encoding=False)],
                         ids=["mean-wpe-nopos2d", "concat3", "concat-nopatch", "mean-nopatch-wpe"])
def test_rollouts_agree_between_the_routes_on_the_other_embedding_branches(arch, monkeypatch):
    _route_vs_route_rollouts("narrow-128", 3, monkeypatch, **arch)


@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("name", ["narrow-128", "gpt-mini"])
def test_gpt_forward_full_and_recurrent_agree_between_the_routes(name, B, monkeypatch):
    """GPT.forward on the full sequence (class and teacher tokens) and recurrent with prev_embeddings (given tokens)."""
    Tn = 3
    oracle = _oracle(name, 5, _kw(block_size=Tn))
    patches, actions, positions = synth_tokens(B, Tn, P, 9, 5, seed=11)
    classes = torch.arange(B) % 100
    with torch.no_grad():
        rl, re = oracle(patches, actions, classes, positions)
        e_o, rec = None, []
        for t in range(Tn):
            lo, e_o = oracle(patches[:, :t + 1], actions[:, :t + 1], classes, positions[:, :t + 1], e_o)
            rec.append(lo[:, -1])
    got = {}
    for wide in (False, True):
        product = _product(name, oracle, monkeypatch, wide, B * Tn, block_size=Tn)
        lg, emb = product(patches, actions, classes, positions)
        e_p, rp = None, []
        for t in range(Tn):
            lp, e_p = product(patches[:, :t + 1], actions[:, :t + 1], classes, positions[:, :t + 1], e_p)
            rp.append(lp[:, -1].cpu())
        got[wide] = (lg.cpu(), emb.cpu(), torch.stack(rp, 1), e_p.cpu())
        for tag, x, ref in (("logits", got[wide][0], rl), ("final_emb", got[wide][1], re),
                            ("recurrent logits", got[wide][2], torch.stack(rec, 1)), ("recurrent emb", got[wide][3], e_o)):
            d = float((x - ref).abs().max())
            print(f"{name} B={B} {'wide' if wide else 'per-agent'} vs oracle: {tag} {d:.3e}")
            assert d < TOL_LOGIT, (tag, wide, d)
    for i, tag in enumerate(("logits", "final_emb", "recurrent logits", "recurrent emb")):
        d = float((got[True][i] - got[False][i]).abs().max())
        print(f"{name} B={B}: measured route-to-route distance, {tag}: {d:.3e}")
        assert d < TOL_LOGIT, (tag, d)


# ---- (b) wide models against the oracle ----------------------------------------------------------------------------------
def _greedy_margin(ref):
    top2 = ref["logits"].topk(2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


@pytest.mark.parametrize("name", ["wide-320", "gopher-44m"])
def test_wide_eval_rollouts_vs_oracle(name, monkeypatch):
    B, Tn = 5, 4
    oracle = _oracle(name, 5, _kw(block_size=Tn))
    product = _product(name, oracle, monkeypatch, False, B, block_size=Tn)
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(9))
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=GREEDY_BATCH_SEED[name])
    tr = ja.ReinforceTrainer(_cfg(T=Tn), product)
    for tag, okw, pkw in (("forced", dict(forced_actions=forced), dict(forced_actions=forced)),
                          ("greedy", dict(sample_actions=False), dict(sample_actions=False))):
        with torch.no_grad():
            ref = rollout_ref.rollout(oracle, env_ref.EnvRef(images, bboxes, P, Tn, 1, True), start_positions=start,
                                      stop_early=True, **okw)
        if tag == "greedy":                      # checked on the CPU first: no near-tie the engine could resolve the other way
            assert _greedy_margin(ref) > 1e-3, _greedy_margin(ref)
        env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
        ro = tr.rollout(env, start_positions=start, **pkw)
        _compare_rollouts(ro, ref, TOL_LOGIT, f"{name} {tag} vs oracle")


def test_gpt2_eval_rollout_size_smoke(monkeypatch):
    B, Tn = 2, 2
    oracle = _oracle("gpt2", 5, _kw(block_size=Tn))
    product = _product("gpt2", oracle, monkeypatch, False, B, block_size=Tn)
    forced = torch.tensor([[1, 3], [2, 0]])
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    with torch.no_grad():
        ref = rollout_ref.rollout(oracle, env_ref.EnvRef(images, bboxes, P, Tn, 1, True), forced_actions=forced,
                                  start_positions=start, stop_early=True)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    ro = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, forced_actions=forced, start_positions=start)
    _compare_rollouts(ro, ref, TOL_LOGIT, "gpt2 forced vs oracle")


def test_wide_eval_rollout_is_bit_identical_from_run_to_run(monkeypatch):
    """No float atomics on the wide route: greedy and sampled trajectories depend on it."""
    B, Tn = 5, 4
    oracle = _oracle("wide-320", 5, _kw(block_size=Tn))
    product = _product("wide-320", oracle, monkeypatch, False, B, block_size=Tn)
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=31)
    runs = []
    for _ in range(2):
        env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
        ro = ja.ReinforceTrainer(_cfg(T=Tn), product).rollout(env, sample_actions=False, start_positions=start)
        runs.append({k: v.cpu() for k, v in ro.items() if torch.is_tensor(v)})
    assert set(runs[0]) == set(runs[1]) and "logits" in runs[0]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ---- (c) training ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdrop", [0.0, 0.1], ids=["nodrop", "dropout"])
def test_wide_reinforce_iteration_gradients_vs_oracle(pdrop, monkeypatch):
    """REINFORCE on wide-320 at B = 4, T = 3 against oracle autograd under the bars of tests/test_gpu_parity.py; with
    dropout 0.1 the oracle applies the engine's masks (oracle/dropout_ref.py), which the batched backward regenerates."""
    B, Tn, seed = 4, 3, 77
    oracle = build_like(_oracle("wide-320", 5, _kw(block_size=Tn, dropout=pdrop)))
    product = _product("wide-320", oracle, monkeypatch, False, B, block_size=Tn, dropout=pdrop)
    if pdrop:
        oracle.enable_dropout(pdrop, seed)
        product.set_dropout_seed(seed)
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(3))
    ro, m = _oracle_reinforce_grads(oracle, images, bboxes, start, forced, P, Tn, True, 0.25, 1.5, 0.01)
    tr = ja.ReinforceTrainer(_cfg(T=Tn, learning_rate=1e-3, gradient_accumulation=1), product)
    tr.last_return_mean, tr.last_return_std = 0.25, 1.5
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    got = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    d = float((tr._last_train_buffers["logits"].cpu() - ro["logits"].detach()).abs().max())
    print(f"wide-320 train-mode logits vs oracle (dropout {pdrop}): {d:.3e}")
    assert d < 1e-3
    for k in ("action_loss", "entropy_loss", "loss"):
        assert abs(float(got[k]) - float(m[k].detach())) < 2e-4, (k, float(got[k]), float(m[k].detach()))
    assert _check_grads(product.engine_grads(), oracle, tag=f"wide-320 reinforce dropout {pdrop}") > 150


def test_wide_supervised_step_vs_oracle(monkeypatch):
    B, Tn = 4, 3
    oracle = build_like(_oracle("wide-320", 13, _kw(block_size=Tn)))
    product = _product("wide-320", oracle, monkeypatch, False, B * Tn, block_size=Tn)
    patches, cur, positions = synth_tokens(B, Tn, P, 9, 5, seed=21)
    nxt = torch.randint(0, 9, (B, Tn), generator=torch.Generator().manual_seed(4))
    masks = torch.ones((B, Tn), dtype=torch.long)
    masks[1, Tn - 1:] = 0
    keep = masks.flatten() == 1
    classes = torch.tensor([3, 99, 3, 0])
    oracle.train()
    oracle.zero_grad()
    logits, _ = oracle(patches, cur, classes, positions)
    loss = torch.nn.functional.cross_entropy(logits.reshape(B * Tn, 9), nxt.flatten(), reduction="none")[keep].mean()
    loss.backward()
    cfg = ja.CfgNode(stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, gradient_accumulation=1)
    m = ja.SupervisedTrainer(cfg, product).train_step(patches, cur, nxt, positions, masks, optimizer_step=False, classes=classes)
    assert (m["logits"].cpu() - logits.detach()).abs().max() < 1e-3
    assert abs(float(m["loss"]) - float(loss)) < 2e-4
    assert _check_grads(product.engine_grads(), oracle, skip_prefix=(), tag="wide-320 supervised") > 150


def test_wide_optimizer_step_matches_adamw(monkeypatch):
    B, Tn = 4, 3
    oracle = build_like(_oracle("wide-320", 5, _kw(block_size=Tn)))
    product = _product("wide-320", oracle, monkeypatch, False, B, block_size=Tn)
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=43)
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(5))
    _oracle_reinforce_grads(oracle, images, bboxes, start, forced, P, Tn, True, 0.0, 1.0, 0.01)
    params = [p for n, p in oracle.named_parameters()]
    before = {n: p.detach().clone() for n, p in oracle.named_parameters()}
    ograds = {n: p.grad.detach().clone() for n, p in oracle.named_parameters() if p.grad is not None}
    opt = torch.optim.AdamW(params, lr=1e-3)
    torch.nn.utils.clip_grad_value_(params, 1)
    opt.step()
    tr = ja.ReinforceTrainer(_cfg(T=Tn, learning_rate=1e-3, gradient_accumulation=1), product)
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=True)
    product.pull_parameters()
    psd = dict(product.named_parameters())
    checked = 0
    for name, p in oracle.named_parameters():
        g = ograds.get(name)
        if g is None or not p.requires_grad:
            continue
        # AdamW's first step moves a weight by ~lr * sign(g): compare where the sign of g is well defined
        sig = g.abs() > 1e-2 * g.abs().max()
        got_upd = (psd[name].detach().cpu() - before[name])[sig]
        ref_upd = (p.detach() - before[name])[sig]
        assert torch.allclose(got_upd, ref_upd, atol=5e-5), (name, (got_upd - ref_upd).abs().max())
        checked += 1
    assert checked > 150


def test_wide_training_refuses_a_sequence_the_batched_backward_does_not_take(monkeypatch):
    """Head size 64: 4 (T + 1) 64 + 2 (T + 1)^2 <= 16384 floats of LDS holds up to T = 45.  A wide model has no other
    backward (gpt_backward_kernel ends at n_embd 256), so T = 46 is refused up front with JN_EINVAL."""
    Tn = 46
    oracle = _oracle("wide-320", 5, _kw(block_size=Tn))
    product = _product("wide-320", oracle, monkeypatch, False, Tn, block_size=Tn)
    patches, cur, positions = synth_tokens(1, Tn, P, 9, 5, seed=21)
    nxt = torch.zeros((1, Tn), dtype=torch.long)
    masks = torch.ones((1, Tn), dtype=torch.long)
    cfg = ja.CfgNode(stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, gradient_accumulation=1)
    with pytest.raises(JnError, match=r"failed with code -1: .*batched backward"):          # -1 = JN_EINVAL
        ja.SupervisedTrainer(cfg, product).train_step(patches, cur, nxt, positions, masks, optimizer_step=False)
