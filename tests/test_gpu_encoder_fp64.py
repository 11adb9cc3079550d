"""The patch encoder at the launch shapes of the headline batch (64 patches of 448 px) and around the 56 x 56 deferral
boundary, against the fp64 oracle with the fixed bars of tests/fp64_bars.py (no noise factor, no conditioning draws).

Which kernels run depends on the pixels per launch M = N * H * W: BatchNorm tables are deferred to the consumer for
M <= JN_DEFER_MAX_M (jn_kernels.h), the forward 1x1 layers run pixel-stationary (pw_xs / pw_x3) for M <= JN_XS_MAX_M
(kernels_conv.hip), 14 x 14 maps take the tiny-map tiles for M <= 16384 and the narrow persistent 1x1 kernel / the
small-map data-gradient tiles switch at 65536.  The parity tests of tests/test_gpu_parity.py run 2 - 6 patches; these
run the batch bench.py times."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib
from jolineedle_amd._lib import check, ptr
from oracle.gpt_ref import build_gpt_ref
from tests import fp64_bars as fb
from tests.helpers import make_pair, randomize_bn

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

JN_DEFER_MAX_M = 65536          # jn_kernels.h
JN_XS_MAX_M = 262144            # jn_kernels.h
TINY_M = 16384                  # kernels_conv.hip: tiny_m
SMALL_M = 65536                 # kernels_conv.hip: pw_narrow minimum / JN_PW_WT_SMALL_M default


def _product(N, **kw):
    product, _ = make_pair(fb.SEED_MODEL, bn_seed=fb.SEED_BN, max_batch=N, **fb.MODEL_KW, **kw)
    return product


def _routes(N):
    """The route facts each N of the train-pass test stands for (pixels per launch of the 56, 28 and 14 px maps)."""
    m112, m56, m28, m14 = N * 112 * 112, N * 56 * 56, N * 28 * 28, N * 14 * 14
    assert m56 <= JN_XS_MAX_M                                 # 56 x 56 and below pixel-stationary
    assert m28 <= JN_DEFER_MAX_M and m14 <= TINY_M            # 28 x 28 tables deferred, 14 x 14 on the tiny-map tiles
    if N == 64:
        assert m112 > JN_XS_MAX_M and m56 > JN_DEFER_MAX_M and m28 < SMALL_M   # the headline mix: 50 176 / 12 544 pixels
    elif N == 21:
        assert m112 > JN_XS_MAX_M and m56 > JN_DEFER_MAX_M    # just above both boundaries (263 424, 65 856 pixels)
        assert m14 % 128 and m28 % 128                        # partial pixel tiles (4 116, 16 464)
    else:
        assert N == 20 and m56 <= JN_DEFER_MAX_M and m112 <= JN_XS_MAX_M   # just below: 56 x 56 tables deferred (62 720),
        #                                                       112 x 112 layers pixel-stationary too (250 880)


def _running_stats(product):
    product.pull_bn_statistics()
    return {k: v.cpu() for k, v in product.state_dict().items()
            if k.startswith(fb.PREFIX) and k.endswith(("running_mean", "running_var"))}


def _report_line(text):
    rep = os.environ.get("JN_TEST_GRAD_REPORT")
    if rep:
        with open(rep, "a") as f:
            f.write(text + "\n")


@pytest.mark.parametrize("N,which", [(64, "all"), (64, "fpn2"), (21, "all"), (21, "fpn2"), (20, "all"), (20, "fpn2")])
def test_encoder_train_pass_and_backward_vs_fp64(N, which):
    """One train-mode pass (batch statistics over the N patches) and its backward for a dense random upstream gradient on
    all three FPN outputs ("all") or on fpn[2] only ("fpn2": the other two None, the routes of the training backward):
    the maps, the running statistics of every BN layer and every encoder gradient within the fixed fp64 bars."""
    _routes(N)
    ref = fb.reference(N)
    x, R = fb.inputs(N)
    product = _product(N)
    product.engine_zero_grad()
    maps = product.backbone_features(x, train=True)
    product.backbone_backward(x, fb.upstream(R, which))
    got = {"maps": maps, "stats": _running_stats(product), "grads": product.engine_grads(fb.PREFIX)}
    torch.cuda.synchronize()
    rows = fb.check(got, fb.flat(ref, which), tag=f"encoder fp64 N={N} {which}")
    m2, g2, gm = fb.summary(rows)
    _report_line(f"# encoder fp64 N={N} {which}: worst map rel-L2 {m2:.3e}, worst grad rel-L2 {g2:.3e}, "
                 f"worst grad max-norm {gm:.3e}")
    assert sum(r[1] == "grad" for r in rows) > 200 and sum(r[1] == "stat" for r in rows) > 150


@pytest.mark.parametrize("mode", ["eval-f32", "eval-bf16"])
def test_encoder_forward_at_the_headline_batch_vs_fp64(mode):
    """The eval-mode passes of bench.py --mode rollout [--dtype bf16] at 64 patches of 448 px against fp64.  bf16 storage
    rounds every activation to 8 bits of mantissa (~0.4 % per rounding): relative L2 1e-2 and the max-norm form of
    test_bf16_mode_backbone_maps."""
    N = 64
    ref = fb.eval_reference(N)
    x, _ = fb.inputs(N)
    if mode == "eval-f32":
        product = _product(N)
        bars = {}
    else:
        product = _product(N, act_dtype="bf16")
        bars = dict(map_l2=1e-2, map_max=5e-3, map_abs=1e-4)
    got = product.backbone_features(x)
    rows = fb.check({"maps": got}, {"maps": ref}, tag=f"encoder fp64 {mode} N={N}", **bars)
    _report_line(f"# encoder fp64 {mode} N={N}: worst map rel-L2 {fb.summary(rows)[0]:.3e}")


_PLAN_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from tests.helpers import make_pair
N, P = 4, 64
product, _ = make_pair(3, patch_size=P, block_size=2, with_detector=False, image_processor=None, max_batch=N)
g = torch.Generator().manual_seed(9)
x = torch.rand((N, 3, P, P), generator=g)
R = [torch.randn((N, c, P // s, P // s), generator=g) for c, s in zip((64, 128, 256), (8, 16, 32))]
for tag, gs in (("none", [None, None, R[2]]), ("zero", [torch.zeros_like(R[0]), torch.zeros_like(R[1]), R[2]])):
    product.engine_zero_grad()
    product.backbone_features(x, train=True)
    torch.cuda.synchronize()
    print("=== " + tag, file=sys.stderr, flush=True)
    product.backbone_backward(x, gs)
    torch.cuda.synchronize()
    print("=== end", file=sys.stderr, flush=True)
"""


def test_null_fpn_gradient_takes_the_training_backward_routes():
    """jn_backbone_backward with fpn[0] / fpn[1] = NULL runs the routes of the training backward (fpn_zero): the stride-2
    depthwise backward of bu_conv2 / bu_conv1 writes its input gradient and forms the producer's BatchNorm sums, so the
    plan (JN_DBG_BWD_PLAN, read once per process: a fresh child) has strictly fewer separate-reduce elements than with
    explicit zero gradients, whose gradient must be accumulated."""
    env = dict(os.environ, JN_DBG_BWD_PLAN="1")
    res = subprocess.run([sys.executable, "-c", _PLAN_CHILD, str(ROOT)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    sep, cur = {}, None
    for line in res.stderr.splitlines():
        if line.startswith("=== "):
            cur = line[4:].strip()
            sep.setdefault(cur, 0)
        elif line.startswith("[bwd-plan]") and cur in ("none", "zero"):
            sep[cur] += int(line.split("separate-reduce elements/patch")[1].split()[0])
    assert set(sep) >= {"none", "zero"}, res.stderr[-4000:]
    assert 0 < sep["none"] < sep["zero"], sep


def _maps_pair(product, x):
    """Train-mode maps with the split weight planes (pw_x3) and on the fp32 matrix pipe (JN_NO_PW_X3=1, read per pass)."""
    on = [t.cpu().double() for t in product.backbone_features(x, train=True)]
    os.environ["JN_NO_PW_X3"] = "1"
    try:
        off = [t.cpu().double() for t in product.backbone_features(x, train=True)]
    finally:
        del os.environ["JN_NO_PW_X3"]
    return on, off


def test_split_weight_planes_follow_every_parameter_writer(tmp_path):
    """The pw_x3 forward reads params_x3, re-split from the fp32 weights only when x3_dirty is set.  At 64 patches of
    448 px, train mode, a forward after each parameter writer — jn_load_weights (load_state_dict), jn_optimizer_step,
    jn_optimizer_step_group (EngineAdamW.step), jn_import_arena and a checkpoint resume — equals the same pass on the fp32
    matrix pipe to <= 1e-4 relative L2 per level (the map bar both routes meet against fp64; measured on the MI355X with
    freshly split planes: 2.1e-5 — train-mode batch statistics amplify the rounding of two correct routes).  A stale plane
    is off by the size of the writer's change, and each writer must move the maps by more than 1e-3, ten times the bar."""
    from jolineedle_amd import checkpoint
    N = 64
    x, R = fb.inputs(N)
    product = _product(N)
    eng = product.engine()
    stream = _lib.current_stream(product.device)
    rel = lambda a, b: max(float((u - v).norm() / v.norm()) for u, v in zip(a, b))
    prev = None

    def check_pair(writer):
        nonlocal prev
        on, off = _maps_pair(product, x)
        assert rel(on, off) <= 1e-4, (writer, rel(on, off))
        if prev is not None:
            assert rel(on, prev) > 1e-3, (writer, "the writer did not move the weights", rel(on, prev))
        prev = on

    def backward():
        product.engine_zero_grad()
        product.backbone_features(x, train=True)
        product.backbone_backward(x, fb.upstream(R, "fpn2"))

    check_pair("initial upload")
    other = build_gpt_ref(fb.SEED_MODEL + 1, **fb.MODEL_KW)
    randomize_bn(other, fb.SEED_BN + 1)
    product.load_state_dict(other.state_dict())
    check_pair("load_state_dict")
    backward()
    check(eng.lib.jn_optimizer_step(eng.handle, 1e-3, 0.01, 0.0, 1.0, stream), "jn_optimizer_step")
    check_pair("jn_optimizer_step")
    checkpoint.save_checkpoint(product, tmp_path)                      # this state, AdamW moments included
    optim_gpt, _ = product.configure_optimizers(ja.CfgNode(learning_rate=1e-3))
    product.bind_flat()
    product._flat_grads.normal_(generator=torch.Generator(device=product.device).manual_seed(2))
    optim_gpt.step()
    check_pair("EngineAdamW.step")
    buf = product._flat_params.clone()
    buf.mul_(1.0 + 2e-2 * torch.randn(buf.shape, device=buf.device, generator=torch.Generator(device=buf.device).manual_seed(3)))
    check(eng.lib.jn_import_arena(eng.handle, 0, ptr(buf), buf.numel(), stream), "jn_import_arena")
    check_pair("jn_import_arena")
    checkpoint.load_checkpoint(ja.CfgNode(resume_training=str(tmp_path), learning_rate=1e-3), product)
    check_pair("checkpoint resume")
