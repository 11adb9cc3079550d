"""The fixed fp64 bars of tests/fp64_bars.py mean something on their inputs (CPU only).  21 patches of 448 px (the batch
just above the 56 x 56 deferral boundary that tests/test_gpu_encoder_fp64.py also runs), both upstream variants:

- the fp32 oracle (torch's own rounding) meets every gradient bar at HALF its value and the map / statistics bars;
- two fixed one-ulp SiLU-noise evaluations do the same: the input has no near-tie that the GPU side would need a
  conditioning probe for;
- the comparator rejects small deliberate errors (negative controls), each by the relative-L2 bar alone, and the
  gradient ones also by the max-norm bar alone."""
import math
import re

import pytest
import torch

from tests import fp64_bars as fb

N = 21
INF = math.inf


@pytest.fixture(scope="module")
def ref():
    return fb.reference(N)


@pytest.fixture(scope="module")
def fp32(ref):
    return fb.encoder_pass(fb.make_oracle(), *fb.inputs(N), dtype=torch.float32)


@pytest.mark.parametrize("which", fb.UPSTREAMS)
def test_fp32_oracle_meets_half_the_gradient_bars(ref, fp32, which):
    rows = fb.check(fb.flat(fp32, which), fb.flat(ref, which), tag=f"fp32 oracle N={N} {which}",
                    grad_l2=fb.GRAD_L2 / 2, grad_max=fb.GRAD_MAX / 2)
    kinds = [r[1] for r in rows]
    assert kinds.count("map") == 3 and kinds.count("grad") > 200 and kinds.count("stat") > 150


@pytest.mark.parametrize("seed", [1234, 1235])
def test_one_ulp_silu_noise_meets_half_the_gradient_bars(ref, seed):
    noisy = fb._with_noisy_silu(fb.make_oracle(), seed, 1e-7)
    got = fb.encoder_pass(noisy, *fb.inputs(N), dtype=torch.float32)
    for which in fb.UPSTREAMS:
        fb.check(fb.flat(got, which), fb.flat(ref, which), tag=f"fp32 oracle + SiLU noise 1e-7 (seed {seed}) {which}",
                 grad_l2=fb.GRAD_L2 / 2, grad_max=fb.GRAD_MAX / 2)


def _rejects(got, ref, name, **bars):
    with pytest.raises(AssertionError, match=re.escape(name)):
        fb.check(got, ref, tag="negative control", **bars)


GRAD_CONTROLS = {
    "stem": "gpt_backbone.backbone.stem.conv.conv.weight",
    "depthwise": "gpt_backbone.bu_conv2.dconv.conv.weight",
    "pointwise": "gpt_backbone.C3_n4.conv3.conv.weight",
    "bn weight": "gpt_backbone.backbone.dark3.1.m.1.conv2.pconv.bn.weight",
    "bn bias": "gpt_backbone.backbone.dark2.1.conv1.bn.bias",
}


@pytest.mark.parametrize("which", fb.UPSTREAMS)
def test_negative_controls_are_rejected(ref, fp32, which):
    r, base = fb.flat(ref, which), fb.flat(fp32, which)
    fb.check(base, r)                                           # the unperturbed fp32 oracle passes

    def with_grad(name, t):
        return dict(base, grads=dict(base["grads"], **{name: t}))

    # one gradient tensor scaled by 1.01 (a 1 %-sized bug in one route), once per layer kind
    for kind, name in GRAD_CONTROLS.items():
        got = with_grad(name, base["grads"][name] * 1.01)
        _rejects(got, r, name)
        _rejects(got, r, name, grad_max=INF)
        _rejects(got, r, name, grad_l2=INF)
    # one tensor with 1e-2 relative-L2 noise
    name = "gpt_backbone.backbone.dark4.1.conv2.conv.weight"
    g = base["grads"][name]
    noise = torch.randn(g.shape, generator=torch.Generator().manual_seed(3), dtype=g.dtype)
    got = with_grad(name, g + noise * (1e-2 * g.norm() / noise.norm()))
    _rejects(got, r, name)
    _rejects(got, r, name, grad_max=INF)
    _rejects(got, r, name, grad_l2=INF)
    # one FPN level off by 1e-3 relative
    for i in range(3):
        maps = list(base["maps"])
        maps[i] = maps[i] * (1 + 1e-3)
        _rejects(dict(base, maps=maps), r, f"fpn{i}")
        _rejects(dict(base, maps=maps), r, f"fpn{i}", map_max=INF)
    # the running variance of one BN layer off by 1e-3 relative
    name = "gpt_backbone.C3_p3.conv2.bn.running_var"
    _rejects(dict(base, stats=dict(base["stats"], **{name: base["stats"][name] * (1 + 1e-3)})), r, name)
