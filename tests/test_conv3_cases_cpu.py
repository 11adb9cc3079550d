"""CPU side of the dense 3x3 kernel pins (tests/conv3_cases.py, tests/test_gpu_conv3_kernels.py):
 - the bars mean something on the cases' inputs: plain fp32 arithmetic meets the fp32-route bars with 4x to spare, emulations
   of the split and of the bf16 number formats meet theirs with 2x;
 - the bars bite: every mistake a kernel of this unit can plausibly make (transformed padding, unmirrored taps, a dropped
   halo row / column / input row, a dropped partial product, an ignored accumulate, a wrong slot table) puts the reference
   over a bar on every case it applies to;
 - jn_conv3_route (host code, no device call) agrees with the launch rule restated here from the comments of
   kernels_conv3.hip, and with the launches those comments and the suite name;
 - the entries refuse bad arguments and unmet route preconditions before any device call."""
import itertools
import math

import pytest
import torch

from jolineedle_amd import _lib
from tests import conv3_cases as cc

FP32_ROUTE = lambda c: (c.kind in ("fwd", "wt", "ds2") and c.route == 1) or (c.kind == "dw" and c.route == 3)
SPLIT_ROUTE = lambda c: (c.kind in ("fwd", "wt", "ds2") and c.route == 2) or (c.kind == "dw" and c.route in (1, 2))


def _unique(cases):
    """One case per distinct computation (routes of one arithmetic share inputs and reference)."""
    seen, out = set(), []
    for c in cases:
        k = c._replace(route=0, skip=0, max_wg=0)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


# ---- the case list itself ---------------------------------------------------------------------------------------------------
def test_every_kernel_meets_every_edge_and_option():
    assert len(cc.KERNELS) == 16      # the ten kernel templates of the unit in every instantiation the entries reach
    for name, cases in cc.KERNELS.items():
        c0 = cases[0]
        shapes = {(c.H, c.W) for c in cases}
        want = set(cc.SPATIAL_S2 if c0.stride == 2 else cc.SPATIAL_S1)
        if c0.kind == "bf16":
            want = {(5 * c0.stride, 5 * c0.stride), cc.TWO_TILES[c0.stride]}
        elif c0.stride == 1 and FP32_ROUTE(c0):
            want |= set(cc.SPATIAL_S1_F32)
        assert shapes == want, (name, shapes)
        pairs = {((c.cout, c.cin) if c.kind == "ds2" else (c.cin, c.cout)) for c in cases}
        want_pairs = {(32, 32), (64, 96)} if c0.kind == "bf16" else {(32, 32), (64, 96), (128, 64)}
        if c0.kind != "bf16" and (FP32_ROUTE(c0) or (c0.kind == "dw" and c0.route == 2)):
            want_pairs.add(cc.PAIR_F32)
        assert pairs == want_pairs, (name, pairs)
        two = cc.TWO_TILES[c0.stride]
        opt = lambda **kw: any((c.H, c.W) == two and all(getattr(c, k) == v for k, v in kw.items()) for c in cases)
        if c0.kind == "dw":
            assert all(opt(slots=s, max_wg=m) for s in (1, 3) for m in (0, 1, 2)), name
        elif c0.kind == "bf16":
            assert opt(skip=1) and opt(skip=2), name
        else:
            if c0.kind != "ds2":      # (the stride-2 data gradients have neither statistics nor a skip flag)
                assert opt(skip=1, stats=1) and opt(skip=2, stats=1) and opt(stats=1, skip=0), name
            if name != "conv3_x3s2_kernel":
                assert opt(accumulate=1), name
            if c0.kind in ("wt", "ds2"):
                assert opt(slots=3, accumulate=0) and opt(slots=3, accumulate=1), name
        for c in cases:      # N = 2 and padded leading dimensions everywhere
            (ld_a, c_a), (ld_b, c_b) = cc.lds(c)
            assert ld_a > c_a and ld_b > c_b and ld_a % 4 == 0 and ld_b % 4 == 0


# ---- the bars mean something --------------------------------------------------------------------------------------------------
def test_fp32_arithmetic_meets_the_fp32_route_bars_with_4x_margin():
    worst = 0.0
    for c in _unique([c for c in cc.ALL_CASES if FP32_ROUTE(c)]):
        ref, ref_stats = cc.reference(c)
        got, stats = cc.compute(c, torch.float32)
        assert not cc.over_bars(c, got, ref, margin=4.0), (c, cc.over_bars(c, got, ref, margin=4.0))
        worst = max(worst, cc.distances(got, ref)[0])
        if c.stats:
            oh, ow = cc.out_hw(c)
            assert cc.stats_over_bar(stats, ref_stats, cc.N * oh * ow * c.slots) * 4.0 <= 1.0, c
    print(f"fp32 arithmetic: worst relative L2 {worst:.2e}")


def test_split_emulation_meets_the_bars_with_2x_margin():
    worst = 0.0
    for c in _unique([c for c in cc.ALL_CASES if SPLIT_ROUTE(c)]):
        ref, ref_stats = cc.reference(c)
        got, stats = cc.compute_split(c)
        assert not cc.over_bars(c, got, ref, margin=2.0), (c, cc.over_bars(c, got, ref, margin=2.0))
        worst = max(worst, cc.distances(got, ref)[1])
        if c.stats:
            oh, ow = cc.out_hw(c)
            assert cc.stats_over_bar(stats, ref_stats, cc.N * oh * ow * c.slots) * 2.0 <= 1.0, c
    print(f"split emulation: worst max-norm {worst:.2e}")


def test_bf16_emulation_meets_the_bf16_bars_with_2x_margin():
    for c in _unique([c for c in cc.ALL_CASES if c.kind == "bf16"]):
        ref, _ = cc.reference(c)
        got, _ = cc.compute_bf16(c)
        print(c, "bf16 emulation: relative L2 %.2e max-norm %.2e" % cc.distances(got, ref))
        assert not cc.over_bars(c, got, ref, margin=2.0), (c, cc.over_bars(c, got, ref, margin=2.0))


# ---- the bars bite ------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "pad_silu": lambda c: c.kind in ("fwd", "wt", "dw", "bf16"),
    "unmirrored": lambda c: c.kind == "wt",
    "drop_last_row": lambda c: c.kind == "ds2",
    "drop_last_col": lambda c: c.kind == "ds2",
    "missing_row": lambda c: c.kind == "dw",
    "no_accumulate": lambda c: c.kind == "dw" or c.accumulate,
    "slot_table": lambda c: c.kind == "dw" and c.slots == 3,
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_of_the_reference_exceeds_a_bar_on_every_case_it_applies_to(mutant):
    cases = [c for c in cc.ALL_CASES if MUTANTS[mutant](c)]
    assert cases
    seen = set()
    for c in cases:
        key = c._replace(skip=0, max_wg=0, stats=0)      # (the route stays: it decides the bars)
        if key in seen:
            continue
        seen.add(key)
        ref, _ = cc.reference(c)
        got, _ = cc.compute(c, torch.float64, mutant=mutant)
        assert cc.over_bars(c, got, ref), (mutant, c, cc.distances(got, ref))


def test_split_emulation_without_the_hi_lo_product_exceeds_a_bar_on_every_split_case():
    for c in _unique([c for c in cc.ALL_CASES if SPLIT_ROUTE(c)]):
        ref, _ = cc.reference(c)
        got, _ = cc.compute_split(c, drop_hi_lo=True)
        assert cc.over_bars(c, got, ref), (c, cc.distances(got, ref))


# ---- the launch rule ------------------------------------------------------------------------------------------------------------
def _x3_cheaper(wg_f32, f32_per_round, f32_round_cost, wg_x3):
    """Rounds of workgroups x time per round: an x3 round (256 workgroups of 16 x 16 pixels) takes 0.65 of an fp32 round of
    8-row tiles."""
    return 0.65 * math.ceil(wg_x3 / 256) < math.ceil(wg_f32 / f32_per_round) * f32_round_cost


def rule(kind, n, H, W, cin, cout, stride, slots, ld_a, ld_b):
    """The route each launcher's rule picks, restated from the comments above x3_cheaper, conv3_x3_ok, conv3_x3s2_ok,
    launch_conv3_bwd_data_s2 and launch_conv3_bwd_weight (JN_NO_CONV3_X3 and JN_WW_EXACT unset)."""
    OH, OW = H // stride, W // stride
    tx = math.ceil(OW / 16)
    aligned = ld_a % 4 == 0 and ld_b % 4 == 0
    if kind in (0, 1):
        nbo = math.ceil(cout / 64)
        if cin % 32 or cout % 4 or not aligned:
            return 1
        if stride == 1:
            return 2 if _x3_cheaper(tx * math.ceil(OH / 8) * n * nbo * slots, 512, 1.0, tx * math.ceil(OH / 16) * n * nbo * slots) else 1
        if slots > 1:
            return 1
        return 2 if _x3_cheaper(tx * math.ceil(OH / 4) * n * nbo, 512, 0.5, tx * math.ceil(OH / 16) * n * nbo) else 1
    if kind == 2:
        nbi = math.ceil(cin / 64)
        if cout % 32 or not aligned:
            return 1
        return 2 if _x3_cheaper(tx * math.ceil(OH / 8) * n * nbi * 4 * slots, 512, 1.0, tx * math.ceil(OH / 16) * n * nbi * 4 * slots) else 1
    return 1 if cout % 16 == 0 and cin % 4 == 0 and aligned else 2


@pytest.fixture()
def lib(monkeypatch):
    monkeypatch.delenv("JN_NO_CONV3_X3", raising=False)
    return _lib.load_library()


def _route(lib, c_or_kind, *shape):
    if isinstance(c_or_kind, cc.Case):
        c = c_or_kind
        (ld_a, _), (ld_b, _) = cc.lds(c)
        return lib.jn_conv3_route(cc.entry_kind(c), cc.N, c.H, c.W, c.cin, c.cout, c.stride, c.slots, ld_a, ld_b)
    return lib.jn_conv3_route(c_or_kind, *shape)


def test_route_entry_agrees_with_the_restated_rule(lib):
    n_x3 = n_f32 = 0
    for kind, n, hw, (cin, cout), slots, pad in itertools.product(
            (0, 1, 2, 3), (1, 2, 6, 16, 21, 32, 64), (4, 10, 20, 34, 40, 80, 160), ((32, 32), (32, 64), (64, 64), (64, 128), (128, 64),
                                                                                    (256, 256), (20, 36), (96, 64)), (1, 3), (0, 4)):
        for stride in ((1,) if kind == 1 else (2,) if kind == 2 else (1, 2)):
            args = (kind, n, hw, hw + 2 * (hw % 4 == 0), cin, cout, stride, slots, (cin if kind < 2 else cout) + pad, (cout if kind < 2 else cin) + pad)
            got = lib.jn_conv3_route(*args)
            assert got == rule(*args), (args, got)
            n_x3 += got == 2
            n_f32 += got == 1
    assert n_x3 > 500 and n_f32 > 500      # the grid crosses the rule's thresholds both ways


def test_route_entry_on_the_launches_the_comments_and_the_suite_name(lib):
    # kernels_conv3.hip, above x3_cheaper: "forward of 16 patches at 40 x 40: 480 fp32 workgroups = one round, 288 x3 workgroups =
    # two" — 3 x 5 tiles x 16 patches x 2 output blocks of 64, i.e. a layer with 128 output channels: fp32
    assert lib.jn_conv3_route(0, 16, 40, 40, 64, 128, 1, 1, 64, 128) == 1
    # the same counts with 64 -> 64 channels (one output block) need 32 patches; 16 patches are 240 fp32 / 144 x3 workgroups,
    # one round each, and the rule gives those the x3 kernel
    assert lib.jn_conv3_route(0, 32, 40, 40, 64, 64, 1, 1, 64, 64) == 1
    assert lib.jn_conv3_route(0, 16, 40, 40, 64, 64, 1, 1, 64, 64) == 2
    # dark2.0.conv of yolox-s, 32 -> 64 channels, 160 x 160 -> 80 x 80, at (320 px, 6 patches): the stride-2 x3 kernel
    # (the one shape through which the suite reaches conv3_x3s2_kernel)
    assert lib.jn_conv3_route(0, 6, 160, 160, 32, 64, 2, 1, 32, 64) == 2
    for c in cc.ALL_CASES:
        if c.kind == "bf16":
            continue
        want = {"fwd": (2 if c.stride == 1 and c.cin % 32 == 0 else 1), "wt": 2 if c.cin % 32 == 0 else 1,
                "ds2": 2 if c.cout % 32 == 0 else 1, "dw": 1 if c.cout % 16 == 0 else 2}[c.kind]
        assert _route(lib, c) == want == rule(cc.entry_kind(c), cc.N, c.H, c.W, c.cin, c.cout, c.stride, c.slots,
                                              cc.lds(c)[0][0], cc.lds(c)[1][0]), c


def test_route_entry_honours_the_fp32_switch(lib, monkeypatch):
    monkeypatch.setenv("JN_NO_CONV3_X3", "1")      # read per launch
    for c in cc.ALL_CASES:
        if c.kind in ("fwd", "wt", "ds2"):
            assert _route(lib, c) == 1, c


# ---- refusals: every check runs before the first device call, so a made-up address is never touched -----------------------------
P = 4096      # stands for a device pointer


def _conv3(lib, **o):
    g = lambda k, d: o.get(k, d)
    cin, cout = g("cin", 32), g("cout", 32)
    return lib.jn_conv3(g("inp", P), g("in_ld", cin + 8), g("tab", P), g("w", P), g("out", P), g("out_ld", cout + 4), g("N", 2), g("H", 6),
                        g("W", 6), cin, cout, g("stride", 1), g("transposed", 0), g("accumulate", 0), g("stats", None), None, 0,
                        g("slots", 1), g("in_slot", 0), g("out_slot", 0), g("route", 1), None)


def _ds2(lib, **o):
    g = lambda k, d: o.get(k, d)
    cin, cout = g("cin", 32), g("cout", 32)
    return lib.jn_conv3_bwd_data_s2(g("gz", P), g("g_ld", cout + 8), g("w", P), g("gin", P), g("gin_ld", cin + 4), g("N", 2), g("H", 6),
                                    g("W", 6), cout, cin, 0, g("slots", 1), g("route", 1), None)


def _dw(lib, **o):
    g = lambda k, d: o.get(k, d)
    cin, cout = g("cin", 32), g("cout", 32)
    return lib.jn_conv3_bwd_weight(g("gz", P), g("g_ld", cout + 8), g("x", P), g("x_ld", cin + 8), g("tab", P), g("gw", P), g("N", 2),
                                   g("H", 6), g("W", 6), cout, cin, g("stride", 1), g("slots", 1), g("route", 1), g("max_wg", 0), None)


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    common = (dict(N=0), dict(H=0), dict(W=-1), dict(cin=0), dict(cout=0), dict(cin=30), dict(cout=34), dict(slots=0), dict(route=-1),
              dict(route=4))
    for bad in common + (dict(inp=None), dict(tab=None), dict(w=None), dict(out=None), dict(stride=3), dict(stride=0),
                         dict(stride=2, H=5), dict(stride=2, W=7), dict(in_ld=28), dict(out_ld=28), dict(in_ld=34), dict(out_ld=38),
                         dict(transposed=1, stride=2), dict(slots=3, in_slot=8, out_slot=8), dict(in_slot=-4)):
        assert _conv3(lib, **bad) == -1, bad
    for bad in common + (dict(gz=None), dict(w=None), dict(gin=None), dict(H=5), dict(W=7), dict(g_ld=28), dict(gin_ld=34), dict(route=3)):
        assert _ds2(lib, **bad) == -1, bad
    for bad in common + (dict(gz=None), dict(x=None), dict(tab=None), dict(gw=None), dict(stride=3), dict(stride=2, H=5), dict(g_ld=38),
                         dict(x_ld=28), dict(max_wg=-1)):
        assert _dw(lib, **bad) == -1, bad
    for kind, bad in ((4, {}), (-1, {}), (0, dict(H=0)), (1, dict(stride=2)), (2, dict(stride=1)), (2, dict(stride=2, H=5)), (0, dict(cin=30)),
                      (3, dict(slots=0)), (0, dict(ld_a=28))):
        a = dict(N=2, H=6, W=6, cin=32, cout=32, stride=2 if kind == 2 else 1, slots=1, ld_a=40, ld_b=36)
        a.update(bad)
        assert lib.jn_conv3_route(kind, a["N"], a["H"], a["W"], a["cin"], a["cout"], a["stride"], a["slots"], a["ld_a"], a["ld_b"]) == -1, (kind, bad)


def test_a_forced_route_refuses_a_launch_that_misses_its_preconditions(lib):
    # the split kernels contract whole chunks of 32 channels
    assert _conv3(lib, route=2, cin=20, cout=36) == -1
    assert _conv3(lib, route=2, cin=48) == -1
    assert _conv3(lib, route=2, transposed=1, cin=20, cout=36) == -1
    assert _conv3(lib, route=2, stride=2, cin=20, cout=36) == -1
    assert _ds2(lib, route=2, cout=20, cin=36) == -1
    # the stride-2 split forward neither accumulates nor takes slots
    assert _conv3(lib, route=2, stride=2, accumulate=1) == -1
    assert _conv3(lib, route=2, stride=2, slots=3, in_slot=2 * 36 * 40, out_slot=2 * 9 * 36) == -1
    # the bf16 kernel: whole groups of 8 input channels, no statistics, accumulate, slots or transposed weight
    assert _conv3(lib, route=3, cin=20, cout=36) == -1
    assert _conv3(lib, route=3, stats=P) == -1
    assert _conv3(lib, route=3, accumulate=1) == -1
    assert _conv3(lib, route=3, transposed=1) == -1
    assert _conv3(lib, route=3, slots=3, in_slot=2 * 36 * 40, out_slot=2 * 36 * 36) == -1
    # the transposed-read weight gradient: whole groups of 16 output channels
    assert _dw(lib, route=1, cout=36, cin=20) == -1
    assert _dw(lib, route=1, cout=40) == -1
