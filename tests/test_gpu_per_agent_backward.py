"""gpt_backward_kernel (csrc/kernels_train.hip), the one-workgroup-per-agent backward of the decision transformer, on shapes
that gpt_backward_route sends to it: the LDS form of the batched backward does not fit and T <= 62.  No zoo model has such a shape
below T = 63, so two are registered here and handed to the product by their dimensions:

  heads-64   (n_layer 2, n_head 2, n_embd 128): head size 64, per-agent from T = 46; two heads, so the h * hs indexing matters;
  head-256   (1, 1, 256): one head of 256 channels, per-agent from T = 15.

  1. the route: 2 at every shape below, 1 at the length one under it;
  2. the supervised step against oracle autograd (the machinery of test_gpu_long_walks.py section 2, for B sequences with a
     padded tail);
  3. one REINFORCE iteration with every agent forced to STOP at step 40 of 46;
  4. the same supervised step with and without JN_GPT_BWD_TILED=1: per-agent kernel against the tiled batched form, with dropout
     at its four sites and under every embedding variant the kernel branches on.
64-px patches, yolox-nano patch encoder, no detector throughout.

No defect of gpt_backward_kernel was found: every case below passes on the kernel as it was."""
import copy

import pytest
import torch

import jolineedle_amd as ja
from oracle import gpt_ref
from tests.helpers import model_config, randomize_bn, synth_batch, synth_tokens
from tests.test_gpu_long_walks import oracle_noise
from tests.test_gpu_parity import (L2_DECISION, _cfg, _check_grads, _check_grads_probed, _grads64, _oracle_reinforce_grads, grad_bar,
                                   l2_bar)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 64
BASE = dict(patch_size=P, gpt_backbone="yolox-nano", image_processor=None, with_detector=False)
DIMS = {"heads-64": (2, 2, 128), "head-256": (1, 1, 256)}
for _name, _dims in DIMS.items():
    gpt_ref.GPT_ZOO[_name] = _dims
LDS, PER_AGENT, TILED = 1, 2, 3


def build_oracle(name, seed, **kw):
    o = gpt_ref.build_gpt_ref(seed, model_type=name, **dict(BASE, **kw))
    randomize_bn(o, 5)
    return o.eval()


def build_product(name, oracle, max_batch, **kw):
    """The engine side of `oracle`, by its dimensions (model_type=None)."""
    n_layer, n_head, n_embd = DIMS[name]
    product = ja.GPT(model_config(**dict(BASE, model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd, **kw)), max_batch=max_batch)
    product.load_state_dict(oracle.state_dict())
    return product


def route_of(product, T):
    eng = product.engine()
    return eng.lib.jn_gpt_backward_route(eng.cfg.n_embd, eng.cfg.n_head, T, eng.lib.jn_debug_decision_route(eng.handle))


# ======================================================================================
# 1. the route
# ======================================================================================
def test_the_shapes_of_this_file_take_the_per_agent_route():
    from jolineedle_amd import _lib
    r = _lib.load_library().jn_gpt_backward_route
    for C, nh, T in ((128, 2, 46), (128, 2, 62), (256, 1, 15)):
        assert r(C, nh, T, 0) == PER_AGENT, (C, nh, T)
    for C, nh, T in ((128, 2, 45), (256, 1, 14)):
        assert r(C, nh, T, 0) == LDS, (C, nh, T)


# ======================================================================================
# 2. the supervised step against oracle autograd
# ======================================================================================
# (model, T, B) -> seed of the weights and of the tokens, chosen on the CPU (see the docstring of the test)
SUPERVISED_CASES = {("heads-64", 46, 2): 14, ("heads-64", 62, 1): 14, ("head-256", 15, 2): 14}
PAD = 7                     # B > 1: the last PAD tokens of sequence 1 are padding


def supervised_inputs(B, T, seed):
    """test_gpu_long_walks.supervised_inputs for B sequences, and the masks: sequence 1 has a padded tail."""
    patches, cur, positions = synth_tokens(B, T, P, 9, 5, seed=seed + 8)
    nxt = torch.randint(0, 9, (B, T), generator=torch.Generator().manual_seed(seed + 9))
    nxt[0, 1] = 8
    masks = torch.ones((B, T), dtype=torch.long)
    if B > 1:
        masks[1, T - PAD:] = 0
    return patches, cur, positions, nxt, masks


def run_supervised_oracle(o, inputs, dt=torch.float32, classes=None):
    """test_gpu_long_walks.run_supervised_oracle for B sequences: cross-entropy meaned over the tokens that are not padding."""
    patches, cur, positions, nxt, masks = inputs
    B, T = cur.shape
    o.train()
    o.zero_grad()
    lg, _ = o(patches.to(dt), cur, torch.zeros(B, dtype=torch.long) if classes is None else classes, positions)
    ce = torch.nn.functional.cross_entropy(lg.reshape(B * T, 9), nxt.flatten(), reduction="none")
    loss = ce[masks.flatten() == 1].mean()
    loss.backward()
    return lg, loss


def supervised_noise(name, T, B, seed):
    """The CPU pre-check: {tensor: fractions of its bars} of the fp32 oracle against its own fp64 evaluation at the case's inputs."""
    o32 = build_oracle(name, seed, block_size=T)
    o64 = copy.deepcopy(o32).double()
    inputs = supervised_inputs(B, T, seed)
    run_supervised_oracle(o32, inputs)
    run_supervised_oracle(o64, inputs, torch.float64)
    return oracle_noise(o32, o64)


SUP_CFG = dict(stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, gradient_accumulation=1)


@pytest.mark.parametrize("model,T,B", list(SUPERVISED_CASES))
def test_supervised_step_on_the_per_agent_route_vs_oracle(model, T, B):
    """B sequences of T tokens (max_batch = B T: the encoder sees every patch in one pass): train-mode logits within 1e-3 of the
    oracle, the loss within 2e-4, every gradient under grad_bar and the relative-L2 bars, none skipped.  heads-64 at T = 46 is the
    first per-agent length at head size 64 and B = 2 makes every per-agent stride count (final_emb, scratch, positions, the
    patch-embedding gradient); T = 62 fills 63 of the kernel's 64 LayerNorm statistic slots; head-256 at T = 15 is the first
    per-agent length of a 256-channel head.
    CPU pre-check of seed 14 (weights; tokens 22, targets 23): the fp32 oracle against its own fp64 evaluation at these inputs,
    worst tensor as a fraction of its bar (max-norm / relative L2): heads-64 T = 46 B = 2 0.079 / 0.069, heads-64 T = 62 B = 1
    0.221 / 0.108, head-256 T = 15 B = 2 0.065 / 0.054 — all under a quarter, encoder included, so no tensor needs the probed check.
    Measured on one MI355X: logits 1.5e-5 / 1.3e-5 / 1.1e-5 from the oracle's, losses equal to six decimals, worst gradient as a
    fraction of its bar (max-norm / relative L2) 0.104 / 0.098, 0.278 / 0.155, 0.084 / 0.070."""
    seed = SUPERVISED_CASES[(model, T, B)]
    oracle = build_oracle(model, seed, block_size=T)
    product = build_product(model, oracle, B * T, block_size=T)
    assert route_of(product, T) == PER_AGENT
    inputs = supervised_inputs(B, T, seed)
    logits, loss = run_supervised_oracle(oracle, inputs)
    patches, cur, positions, nxt, masks = inputs
    m = ja.SupervisedTrainer(ja.CfgNode(**SUP_CFG), product).train_step(patches, cur, nxt, positions, masks, optimizer_step=False)
    d = float((m["logits"].cpu() - logits.detach()).abs().max())
    grads = product.engine_grads()
    worst = (0.0, 0.0)
    for n, p in oracle.named_parameters():
        if p.grad is not None and float(p.grad.abs().max()) > 1e-12:
            ref = p.grad.double()
            worst = (max(worst[0], float((grads[n].double() - ref).abs().max() / ref.abs().max()) / grad_bar(n)),
                     max(worst[1], float((grads[n].double() - ref).norm() / ref.norm()) / l2_bar(n)))
    print(f"per-agent supervised {model} T={T} B={B}: train-mode logits max distance {d:.3e}, loss {float(m['loss']):.6f} vs "
          f"{float(loss.detach()):.6f}, worst gradient at {worst[0]:.3f} of its max-norm bar, {worst[1]:.3f} of its L2 bar")
    assert d < 1e-3
    assert abs(float(m["loss"]) - float(loss.detach())) < 2e-4
    assert _check_grads(grads, oracle, skip_prefix=(), tag=f"per-agent supervised {model} T={T} B={B}") > 150


# ======================================================================================
# 3. one REINFORCE iteration with a forced STOP
# ======================================================================================
REINFORCE_SEED = 5
T_WALK, STOP_STEP = 46, 40


def reinforce_inputs():
    B = 2
    images, bboxes, start = synth_batch(B, 4, 5, P, seed=41)
    forced = torch.randint(0, 8, (B, T_WALK), generator=torch.Generator().manual_seed(3))
    forced[:, STOP_STEP - 1] = 8
    return images, bboxes, start, forced


def run_reinforce_oracle(o, dt=torch.float32):
    images, bboxes, start, forced = reinforce_inputs()
    return _oracle_reinforce_grads(o, images.to(dt), bboxes, start, forced, P, T_WALK, True, 0.25, 1.5, 0.01)


def test_reinforce_iteration_on_the_per_agent_route_vs_oracle():
    """heads-64, B = 2, a 4 x 5 grid, T = 46, every agent forced to STOP at step 40: 41 of the 47 tokens are live.  Losses within
    2e-4 of the oracle loop; the decision side at L2_DECISION and grad_bar with no allowance; the steps that never ran get a zero
    patch-embedding gradient, seen through the encoder gradients, which equal the oracle's (it never ran those steps).
    CPU pre-check (weights seed 5, images 41, actions 3; fp32 oracle against its fp64 evaluation, worst decision-side tensor as a
    fraction of its bar): 0.131 max-norm, 0.165 relative L2 — under a quarter.  The encoder is not, under any seed: every step's
    BatchNorms see two patches (as in test_reinforce_iteration_on_a_long_walk_vs_oracle) and all 232 encoder tensors are over a
    quarter in the fp32 oracle itself (worst 81 x the max-norm bar, 12 x the L2 bar), so embed_fpn.0 and the gpt_backbone tensors are held with
    _check_grads_probed, centred on the fp32 oracle, at most 8 draws on demand.
    Measured on one MI355X: losses within 1e-6, worst decision-side relative L2 2.1e-4 (bar 1e-3); 265 tensors, 1 probe draw."""
    images, bboxes, start, forced = reinforce_inputs()
    oracle = build_oracle("heads-64", REINFORCE_SEED, block_size=T_WALK, nclasses=9)
    product = build_product("heads-64", oracle, 8, block_size=T_WALK, nclasses=9)
    assert route_of(product, T_WALK) == PER_AGENT
    ro, m = run_reinforce_oracle(oracle)
    assert ro["logits"].shape[1] == STOP_STEP
    tr = ja.ReinforceTrainer(_cfg(T=T_WALK, stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    tr.last_return_mean, tr.last_return_std = 0.25, 1.5
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, T_WALK, 1, True)
    got = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    for k in ("action_loss", "entropy_loss", "loss", "returns", "episode_length"):
        print(f"per-agent reinforce: {k} {float(got[k]):.6f} vs {float(m[k].detach()):.6f}")
        assert abs(float(got[k]) - float(m[k].detach())) < 2e-4, (k, float(got[k]), float(m[k].detach()))
    grads = product.engine_grads()
    worst = 0.0
    for name, p in oracle.named_parameters():                            # the decision side gets no allowance
        if p.grad is not None and l2_bar(name) == L2_DECISION and float(p.grad.norm()) > 1e-12:
            ref = p.grad.double()
            l2 = float((grads[name].double() - ref).norm() / ref.norm())
            mx = float((grads[name].double() - ref).abs().max() / ref.abs().max())
            worst = max(worst, l2)
            assert l2 < L2_DECISION and mx < grad_bar(name), (name, l2, mx)
    print(f"per-agent reinforce: worst decision-side relative L2 {worst:.3e}")
    n, draws = _check_grads_probed(grads, oracle, run_reinforce_oracle, _grads64(oracle), 1e-7, f"per-agent reinforce T={T_WALK} stop at {STOP_STEP}",
                                   max_draws=8, full_size=False)
    print(f"per-agent reinforce: {n} tensors, {draws} probe draws")
    assert n > 150


# ======================================================================================
# 4. the per-agent kernel against the tiled form
# ======================================================================================
FORM_CASES = {
    "heads-64": ("heads-64", 46, 0.0, {}, False),
    "heads-64-dropout": ("heads-64", 46, 0.1, {}, False),
    "head-256": ("head-256", 15, 0.0, {}, False),
    "no-concat": ("heads-64", 46, 0.0, dict(concat_emb=False), False),
    "no-pos-emb": ("heads-64", 46, 0.0, dict(use_pos_emb=False), False),
    "learned-wpe": ("heads-64", 46, 0.0, dict(decoder_pos_encoding=False, pos_emb_size=64), False),      # (a wpe row per token: 46 <= 64)
    "classes": ("heads-64", 46, 0.0, {}, True),
}


@pytest.mark.parametrize("case", list(FORM_CASES))
def test_per_agent_kernel_against_the_tiled_form(case, monkeypatch):
    """B = 3: the supervised step with and without JN_GPT_BWD_TILED=1 (read per launch), so the same shape goes through
    gpt_backward_kernel (route 2) and through the batched backward with tiled attention (route 3): the forward logits are
    bit-equal and every gradient is within 1e-4 relative L2 of the other run's.  With dropout 0.1 and set_dropout_seed(77) the keys,
    so the masks, are equal at all four sites (embedding, attention, the two residual branches).  The embedding variants are the
    branches of the kernel's token-embedding section: the mean instead of the projection (concat_emb off), no 2-D position part,
    the learned wpe table and its gradient (decoder_pos_encoding off), a class row other than 0.  The batched form takes all of
    them; none is dropped.
    Measured on one MI355X, worst relative L2 between the forms: heads-64 3.2e-6, with dropout 3.5e-6, head-256 3.9e-6, no-concat
    3.1e-6, no-pos-emb 3.5e-6, learned-wpe 3.3e-6, classes 3.4e-6 (253 to 266 tensors each)."""
    model, T, pdrop, arch, with_classes = FORM_CASES[case]
    B = 3
    patches, cur, positions = synth_tokens(B, T, P, 9, 5, seed=21)
    nxt = torch.randint(0, 9, (B, T), generator=torch.Generator().manual_seed(4))
    masks = torch.ones((B, T), dtype=torch.long)
    classes = torch.tensor([3, 99, 0]) if with_classes else None
    oracle = build_oracle(model, 13, block_size=T, dropout=pdrop, **arch)
    runs = []
    for hook in (None, "1"):
        if hook:
            monkeypatch.setenv("JN_GPT_BWD_TILED", hook)
        else:
            monkeypatch.delenv("JN_GPT_BWD_TILED", raising=False)
        product = build_product(model, oracle, B * T, block_size=T, dropout=pdrop, **arch)
        assert route_of(product, T) == (TILED if hook else PER_AGENT)
        if pdrop:
            product.set_dropout_seed(77)
        m = ja.SupervisedTrainer(ja.CfgNode(**SUP_CFG), product).train_step(patches, cur, nxt, positions, masks, optimizer_step=False,
                                                                            classes=classes)
        runs.append((m["logits"].cpu(), product.engine_grads()))
    monkeypatch.delenv("JN_GPT_BWD_TILED", raising=False)
    assert torch.equal(runs[0][0], runs[1][0])                          # the forward does not know the hook
    worst, compared = 0.0, 0
    for name, g0 in runs[1][1].items():                                 # (the tiled form, held by test_gpu_long_walks.py, is the yardstick)
        g1 = runs[0][1][name]
        if float(g0.norm()) < 1e-12:
            assert float(g1.norm()) < 1e-9, name
            continue
        d = float((g1.double() - g0.double()).norm() / g0.double().norm())
        worst, compared = max(worst, d), compared + 1
        assert d < 1e-4, (name, d)
    print(f"per-agent against tiled, {case}: worst relative L2 between the forms {worst:.3e} over {compared} tensors")
    assert compared > 150
    if case == "learned-wpe":
        assert float(runs[0][1]["transformer.wpe.weight"].norm()) > 0
    if with_classes:
        rows = runs[0][1]["embed_class.weight"].abs().sum(dim=1).nonzero().flatten().tolist()
        assert rows == [0, 3, 99]
