"""tests/zoo_cases.py without a GPU, after tests/test_glue_cases_cpu.py: the list holds what it claims, every launch is admitted by the
route entries, and the bars hold for plain fp32 arithmetic on these cases."""
import torch

from jolineedle_amd import _lib
from tests import conv3_cases as cc
from tests import glue_cases as gc
from tests import pw_cases as pc
from tests import zoo_cases as zc


def _unique(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def test_every_conv_case_is_admitted_by_its_route_entry():
    lib = _lib.load_library()
    for c in zc.pw_forward_cases() + zc.pw_data_gradient_cases():
        assert lib.jn_pw_route(*pc.route_args(c, 0), None) >= 1, c
    assert {(c.cin, c.cout) for c in zc.pw_forward_cases()} == set(zc.PW_LAYERS)
    assert {(c.cout, c.cin) for c in zc.pw_data_gradient_cases()} == set(zc.PW_LAYERS)
    assert {(c.cin, c.cout) for c in zc.pw_weight_gradient_cases()} == set(zc.PW_LAYERS)
    named = {}
    for c in zc.conv3_cases():
        (ld_a, _), (ld_b, _) = cc.lds(c)
        r = lib.jn_conv3_route(cc.entry_kind(c), cc.N, c.H, c.W, c.cin, c.cout, c.stride, c.slots, ld_a, ld_b)
        assert r >= 1, c
        if c.kind == "dw":
            assert r == zc.conv3_weight_route(c), c
            named[c.cout] = r
    assert named == {24: 2, 40: 2, 48: 1}      # Co = 24 and 40: SPLIT; 48: TR
    assert {cc.out_hw(c) for c in zc.conv3_cases()} == set(zc.C3_MAPS)
    for c in zc.glue_cases():
        if c.kind in ("spp", "sppb"):
            assert lib.jn_spp_route(c.dtype, 4 * c.C + gc.IN_PAD, c.C, c.H, c.W, gc.N, int(c.kind == "sppb")) >= 1, c


def test_batchnorm_sum_cases_straddle_a_workgroup_and_the_replicas():
    assert zc.bnb_rows_per_block(24) == 42 * 32 and zc.bnb_rows_per_block(96) == 10 * 32 and zc.bnb_rows_per_block(1280) == 32 and zc.bnb_rows_per_block(1032) == 32
    assert all(zc.bnb_rows_per_block(C) == gc.bnb_rows_per_block(C) for C in zc.BNB_CHANNELS if C <= 1024)
    cases = zc.bnb_cases()
    for C in zc.BNB_CHANNELS:
        ms = {c.M for c in cases if c.C == C and c.slots == 1}
        rows = zc.bnb_rows_per_block(C)
        assert {rows - 1, rows + 1} <= ms and max(ms) > 32 * rows, (C, rows)


P = 4096      # stands for a device pointer: every check runs before the first device call


def test_batchnorm_sums_above_1024_channels_go_in_halves_of_whole_quads_or_are_refused():
    """1280 (yolox-x's widest BatchNorm layer) is the limit; a count that does not halve into quads is refused, as is everything the
    entry refused before (tests/test_glue_cases_cpu.py: 1028, 2048)."""
    lib = _lib.load_library()
    for C in (1028, 1036, 1284, 1288, 2048, 2560):
        assert lib.jn_bn_bwd_sums(P, C + 8, P, C + 8, P, P, C, 10, 1, P, P, P, P, P, P, 1, 0, None) == -1, C
    assert all(C <= 1024 or C % 8 == 0 for C in zc.BNB_CHANNELS) and max(zc.BNB_CHANNELS) == 1280      # what the GPU test launches


def test_the_pointwise_weight_gradient_route_entry_names_the_wide_kernel_from_128_by_128():
    lib = _lib.load_library()
    assert [lib.jn_pw_bwd_weight_route(co, ci) for co, ci in ((24, 24), (124, 512), (128, 124), (128, 128), (640, 1280))] == [1, 1, 1, 2, 2]
    assert lib.jn_pw_bwd_weight_route(30, 64) == -1 and lib.jn_pw_bwd_weight_route(64, 0) == -1
    for c in zc.pw_weight_gradient_cases():      # the cases take the replica scratch exactly where the narrow kernel has room for it
        assert c.use_wpart == int(lib.jn_pw_bwd_weight_route(c.cout, c.cin) == 1 and c.cin * c.cout <= pc.WPART_MAX), c


def test_fp32_arithmetic_stays_within_the_bars():
    for c in _unique(zc.bnb_cases() + [c for c in zc.glue_cases() if not c.dtype], gc._key):
        if c.kind == "bnb" and c.M * c.C > 2e6:
            continue      # (seconds each in fp64 on a CPU; the same arithmetic as the smaller M)
        k = gc._key(c)
        ref, got = gc.reference(c), gc.compute(k, torch.float32)
        assert not gc.over_bars(k, got, ref), (c, gc.over_bars(k, got, ref))
    for c in zc.pw_forward_cases() + zc.pw_data_gradient_cases() + zc.pw_weight_gradient_cases():
        if c.slots > 1:
            continue
        assert not pc.over_bars(c, pc.compute(c, torch.float32), pc.reference(c)), c
    for c in zc.conv3_cases():
        if c.slots > 1 or cc.out_hw(c) == (24, 24):
            continue
        assert not cc.over_bars(c, cc.compute(c, torch.float32)[0], cc.reference(c)[0]), c
