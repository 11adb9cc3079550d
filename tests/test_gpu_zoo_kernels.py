"""The kernels of a dense pass at channel counts that are no powers of two (yolox-m, yolox-x; tests/zoo_cases.py), one launch at a time through the
context-free entries, against the fp64 restatements and the bars of tests/glue_cases.py, tests/pw_cases.py and tests/conv3_cases.py.
Launch helpers and the checks around a launch (canaries, untouched inputs, skipped launches, two runs of one launch) are those of
tests/test_gpu_glue_kernels.py, tests/test_gpu_pw_kernels.py and tests/test_gpu_conv3_kernels.py.

These are the first launches of each kernel at such a count; the network tests of tests/test_gpu_zoo_networks.py come after them."""
import collections

import pytest
import torch

from jolineedle_amd import _lib
from tests import conv3_cases as cc
from tests import glue_cases as gc
from tests import pw_cases as pc
from tests import test_gpu_conv3_kernels as ck
from tests import test_gpu_glue_kernels as gk
from tests import test_gpu_pw_kernels as pk
from tests import zoo_cases as zc

pytestmark = pytest.mark.gpu


# ---- the glue kernels: the body of test_gpu_glue_kernels.test_kernel_against_fp64_at_its_edges over a list of cases ----------
def _glue(cases, name):
    worst = collections.defaultdict(float)
    for c in cases:
        r = gk._run(c)
        gk._check_untouched(c, r)
        if c.skip == 2:
            continue
        ref = gc.reference(c)
        gk._check_exact(c, r, ref)
        got, want = gk._comparable(c, r.res, ref)
        print(f"  {c}: " + gk._distances_line(c, got, want, worst))
        assert not gc.over_bars(c, got, want), (c, gc.over_bars(c, got, want))
        gk._same_launch_twice(c, r, gk._run(c), ref)
    print(f"{name}: {len(cases)} cases, " + ("worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) if worst else "the reference's bits"))


def test_batchnorm_backward_sums_at_the_zoo_channel_counts():
    cases = zc.bnb_cases()
    assert {c.C for c in cases} == set(zc.BNB_CHANNELS)
    _glue(cases, "bn_bwd_reduce_kernel, bn_bwd_consts_kernel")


def test_shortcut_sum_upsample_and_spp_at_24_96_and_192_channels():
    lib = _lib.load_library()
    cases = zc.glue_cases()
    for c in cases:
        if c.kind in ("spp", "sppb"):
            assert lib.jn_spp_route(c.dtype, 4 * c.C + gc.IN_PAD, c.C, c.H, c.W, gc.N, int(c.kind == "sppb")) >= 1, c
    _glue(cases, "addact, upsample, upsample_bwd, spp, spp_bwd")


# ---- 1x1 convs ---------------------------------------------------------------------------------------------------------------------------
def _pw_routes(c):
    """Route 0 first, then every route the entry admits for the launch."""
    lib = _lib.load_library()
    routes = [0]
    if c.kind == "pw":
        for r in range(1, 7):
            if lib.jn_pw_route(*pc.route_args(c, r), None) >= 1:
                routes.append(r)
    return routes


def _pw(cases, name):
    worst = collections.defaultdict(float)
    taken = collections.Counter()
    for c in cases:
        ref = pc.reference(c)
        for route in _pw_routes(c):
            r = pk._run(c, route)
            pk._check_untouched(c, r)
            if c.stats:
                assert torch.equal(r.f64[c.nrep:], r.f64_0[c.nrep:]), (c, route)
            if c.use_wpart:
                assert bool((r.wpart == 0).all()), ("the weight-gradient scratch was not left zero", c)
            l2, mx = pc.distances(r.res["out"], ref[0])
            worst["l2"], worst["max"] = max(worst["l2"], l2), max(worst["max"], mx)
            line = f"  {c} route {route}: rel L2 {l2:.2e} max {mx:.2e}"
            if ref[1] is not None:
                st = pc.stats_over_bar(r.res["stats"], ref[1], pc.pixels(c))
                worst["stats"] = max(worst["stats"], st)
                line += f" stats {st:.2e} of their bar"
            print(line)
            assert not pc.over_bars(c, pk._got(r), ref), (c, route, pc.over_bars(c, pk._got(r), ref))
            pk._same_launch_twice(c, r, pk._run(c, route), ref)
            taken[route] += 1
    print(f"{name}: {len(cases)} cases, launches per route {dict(taken)}, worst relative L2 {worst['l2']:.2e}, max-norm {worst['max']:.2e}")


def test_pointwise_forward_at_the_zoo_channel_counts_on_every_admitted_route():
    _pw(zc.pw_forward_cases(), "1x1 forward")


def test_pointwise_data_gradient_at_the_zoo_channel_counts_on_every_admitted_route():
    _pw(zc.pw_data_gradient_cases(), "1x1 data gradient")


def test_pointwise_weight_gradient_at_the_zoo_channel_counts():
    _pw(zc.pw_weight_gradient_cases(), "1x1 weight gradient")


# ---- dense 3x3 convs -------------------------------------------------------------------------------------------------------------------------
def test_dense_3x3_kernels_at_the_zoo_channel_counts(monkeypatch):
    monkeypatch.delenv("JN_NO_CONV3_X3", raising=False)
    lib = _lib.load_library()
    taken = collections.Counter()
    worst_l2 = worst_max = 0.0
    for c in zc.conv3_cases():
        (ld_a, _), (ld_b, c_b) = cc.lds(c)
        named = lib.jn_conv3_route(cc.entry_kind(c), cc.N, c.H, c.W, c.cin, c.cout, c.stride, c.slots, ld_a, ld_b)
        assert named >= 1, c
        if c.kind == "dw":
            assert named == zc.conv3_weight_route(c), (c, named)
        routes = [0] + ([1] if named != 1 and c.kind != "dw" else []) + ([3] if c.kind == "dw" else [])      # the rule's, fp32; dW: EXACT
        ref, ref_stats = cc.reference(c)
        for route in routes:
            cr = c._replace(route=route)
            r = ck._run(cr, route)
            assert r.inputs_intact, cr
            if c.kind != "dw":
                assert ck._bits(r.raw[..., c_b:], r.raw0[..., c_b:]), ("canary", cr)
            l2, mx = cc.distances(r.out, ref)
            worst_l2, worst_max = max(worst_l2, l2), max(worst_max, mx)
            line = f"  {cr} (rule: {named}): rel L2 {l2:.2e} max {mx:.2e}"
            if c.stats:
                OH, OW = cc.out_hw(c)
                st = cc.stats_over_bar(r.stats, ref_stats, cc.N * OH * OW * c.slots)
                line += f" stats {st:.2e} of their bar"
                assert st <= 1.0, ("stats", cr, st)
            print(line)
            assert not cc.over_bars(cr, r.out, ref), (cr, cc.over_bars(cr, r.out, ref))
            again = ck._run(cr, route)
            if c.kind != "dw":
                assert ck._bits(again.raw, r.raw), ("two runs differ", cr)
            else:
                d = (again.out - r.out).abs().max().item() / ref.abs().max().item()
                assert d <= cc.DW_ORDER, ("two runs differ by more than the order of their atomics", cr, d)
            taken[(c.kind, c.stride, route if route else named)] += 1
    print(f"dense 3x3: launches per (kind, stride, route) {dict(taken)}, worst relative L2 {worst_l2:.2e}, max-norm {worst_max:.2e}")
