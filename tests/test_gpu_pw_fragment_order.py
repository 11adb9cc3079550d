"""The wide forward 1x1 layers (K >= 128) at three patches of 448 px: the smallest launches with both a full and a partial
pixel tile on every wide shape (14 x 14 maps: 588 pixels = nine 64-pixel tiles and one of 12; 28 x 28 maps: 2 352 pixels =
73 32-pixel tiles and a half one).  The tests pin what the layers compute (fp64 oracle, the fp32-pipe route, the bf16
inference mode), not the order in which pw_x3_kernel's split weight planes are stored."""
import os

import pytest
import torch

from tests import fp64_bars as fb
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu
N = 3


def _product(**kw):
    product, _ = make_pair(fb.SEED_MODEL, bn_seed=fb.SEED_BN, max_batch=N, **fb.MODEL_KW, **kw)
    return product


def _running_stats(product):
    product.pull_bn_statistics()
    return {k: v.cpu() for k, v in product.state_dict().items()
            if k.startswith(fb.PREFIX) and k.endswith(("running_mean", "running_var"))}


def test_train_pass_at_three_patches_vs_fp64():
    """Train-mode FPN maps and the running statistics of every BatchNorm layer within the fixed fp64 bars (maps 1e-4 / 1e-3,
    statistics 1e-5 + 1e-4 |ref|).  The fp32 CPU oracle sits at 1.1e-5 / 1.9e-5 / 3.0e-5 on the maps and 0.004 of the
    statistics bar on these inputs."""
    assert (N * 14 * 14) % 64 and (N * 14 * 14) > 64 and (N * 28 * 28) % 32 and (N * 28 * 28) > 32
    ref = fb.reference(N)
    x, _ = fb.inputs(N)
    product = _product()
    maps = product.backbone_features(x, train=True)
    got = {"maps": maps, "stats": _running_stats(product)}
    torch.cuda.synchronize()
    rows = fb.check(got, {"maps": ref["maps"], "stats": ref["stats"]}, tag=f"pw fragment order train N={N}")
    for r in rows[:6]:
        print(r[1], r[2], f"L2 {r[3]:.3e} max {r[4]:.3e}")
    assert sum(r[1] == "stat" for r in rows) > 150 and sum(r[1] == "map" for r in rows) == 3


def test_split_plane_route_equals_fp32_pipe_route_at_three_patches():
    """Eval mode (fixed statistics: nothing amplifies the rounding): the default route against JN_NO_PW_X3=1 (read per
    pass), <= 1e-4 relative L2 per level."""
    x, _ = fb.inputs(N)
    product = _product()
    on = [t.cpu().double() for t in product.backbone_features(x)]
    os.environ["JN_NO_PW_X3"] = "1"
    try:
        off = [t.cpu().double() for t in product.backbone_features(x)]
    finally:
        del os.environ["JN_NO_PW_X3"]
    assert len(on) == len(off) == 3
    for i, (u, v) in enumerate(zip(on, off)):
        d = float((u - v).norm() / v.norm())
        print(f"fpn{i} default vs fp32 pipe: rel L2 {d:.3e}")
        assert d <= 1e-4, (i, d)


def test_bf16_inference_at_three_patches_vs_fp64():
    """The bf16 inference mode (one plane: the h plane of the split weights) against the eval-mode fp64 maps, with the bars
    of the headline-batch test."""
    ref = fb.eval_reference(N)
    x, _ = fb.inputs(N)
    product = _product(act_dtype="bf16")
    got = product.backbone_features(x)
    rows = fb.check({"maps": got}, {"maps": ref}, tag=f"pw fragment order eval-bf16 N={N}", map_l2=1e-2, map_max=5e-3,
                    map_abs=1e-4)
    for r in rows:
        print(r[1], r[2], f"L2 {r[3]:.3e} max {r[4]:.3e}")
