"""The GEMMs of the batched GPT backward (gptb_tok_gemm_kernel: forward recompute and data gradients; gptb_wgrad_kernel:
weight gradients with the bias gradient's column sums folded in; kernels_gptbwd.hip) through the training entry points,
against torch autograd on the CPU oracle with the bars of the existing gradient tests (imported, not restated).

The training entry points refuse a model without a patch encoder, so the models carry the smallest one (yolox-nano at
64 px); what is looked at is the decision side, whose every Linear is three launches of these kernels.  Token rows M = B * (T + 1): 18 (less than one 32-row tile), 105 (no multiple of a tile; the tile edge cuts
a sequence), 1344 (the headline's; 42 row tiles).  N = K = n_actions = 9 at the head takes the guarded 4-byte loads.  In
the supervised cases every token row is live (a row r is dead iff r % (T + 1) >= L, L = executed steps + 1; the padding
masks only zero d logits of the padded tokens, rows of zeros in the operands).  Dead rows — the kernels must write zeros
there and add nothing from them — come from the forced STOP of the REINFORCE cases: 12 rows in one tile, and 144 rows over
five row tiles and three weight-gradient slices, with dead rows at every tile edge (rows 3 .. 5 of each six)."""
import pytest
import torch

import jolineedle_amd as ja
from tests.helpers import make_pair, synth_batch, synth_tokens
from tests.test_gpu_parity import DEV, _cfg, _check_grads, _oracle_reinforce_grads

pytestmark = pytest.mark.gpu

ENCODER = ("gpt_backbone.", "embed_fpn.0")       # pinned at these sizes by the existing tests; not this kernel's output


@pytest.mark.parametrize("B,T", [(3, 5), (5, 20), (64, 20)])
def test_supervised_decision_gradients_vs_oracle(B, T):
    P = 64
    product, oracle = make_pair(13, patch_size=P, block_size=T, with_detector=False, image_processor=None, max_batch=B * T)
    patches, cur, positions = synth_tokens(B, T, P, 9, 5, seed=21 + B)
    g = torch.Generator().manual_seed(4)
    nxt = torch.randint(0, 9, (B, T), generator=g)
    nxt[0, 1] = 8
    masks = torch.ones((B, T), dtype=torch.long)
    masks[1, T - 2:] = 0                                       # padded tails: rows of zeros in d logits (the rows stay live)
    masks[B - 1, 1:] = 0
    keep = masks.flatten() == 1
    classes = torch.arange(B) % 100
    oracle.train()
    oracle.zero_grad()
    lg, _ = oracle(patches, cur, classes, positions)
    ce = torch.nn.functional.cross_entropy(lg.reshape(B * T, 9), nxt.flatten(), reduction="none")
    loss = ce[keep].mean()
    loss.backward()
    tr = ja.SupervisedTrainer(ja.CfgNode(stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, gradient_accumulation=1), product)
    m = tr.train_step(patches, cur, nxt, positions, masks, optimizer_step=False, classes=classes)
    assert (m["logits"].cpu() - lg.detach()).abs().max() < 1e-3
    assert abs(float(m["loss"]) - float(loss)) < 2e-4
    n = _check_grads(product.engine_grads(), oracle, skip_prefix=ENCODER, tag=f"gptb gemm supervised B={B} T={T}")
    assert n >= 40                                             # every decision-side tensor of gpt-nano


@pytest.mark.parametrize("P,B", [(128, 2), (64, 24)])
def test_reinforce_gradients_with_a_forced_stop(P, B):
    """Executed steps S = 2 < T = 5: token rows 3 .. 5 of every agent are dead through *L.  B = 2 on the 128 px encoder;
    B = 24 (M = 144) puts dead rows at the edges of the 32-row tiles and of the 64-row weight-gradient slices."""
    Tn = 5
    product, oracle = make_pair(5, patch_size=P, block_size=Tn, with_detector=False, image_processor=None, max_batch=max(B, 8))
    images, bboxes, start = synth_batch(B, 3, 4, P, seed=41)
    forced = torch.randint(0, 8, (B, Tn), generator=torch.Generator().manual_seed(3))
    forced[:, 1] = 8                                           # STOP at step 2 for every agent
    ro, m = _oracle_reinforce_grads(oracle, images, bboxes, start, forced, P, Tn, True, 0.25, 1.5, 0.01)
    tr = ja.ReinforceTrainer(_cfg(T=Tn, stop=True, learning_rate=1e-3, gradient_accumulation=1), product)
    tr.last_return_mean, tr.last_return_std = 0.25, 1.5
    env = ja.NeedleGeneralEnv(images.to(DEV), bboxes, P, Tn, 1, True)
    got = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
    assert float(m["episode_length"].detach()) < Tn           # the oracle's walk stopped early as well
    for k in ("action_loss", "entropy_loss", "loss", "returns", "episode_length"):
        assert abs(float(got[k]) - float(m[k].detach())) < 2e-4, (k, float(got[k]), float(m[k].detach()))
    assert _check_grads(product.engine_grads(), oracle, tag=f"gptb gemm reinforce forced STOP B={B}") > 150
