"""CPU side of the depthwise 3x3 kernel pins (tests/dw_cases.py, tests/test_gpu_dw_kernels.py):
 - the case list covers every instantiation the launchers reach, at every edge and with every option;
 - the bars mean something on the cases' inputs: plain fp32 arithmetic meets the fp32 bars with 4x to spare (the RED bar is 4x
   what it measures here), an emulation of bf16 storage meets the bf16 bars with 2x;
 - the bars bite: every mistake a kernel of this family can plausibly make (transformed padding, a dropped halo row or column, a
   dropped last odd row or column, swapped parity, unmirrored taps, a transformed raw channel, an ignored accumulate, a wrong
   slot table, a missing c2 term, a pixel missing from a RED sum) puts the reference over a bar on every case it applies to;
 - jn_dw3x3_route (host code, no device call) agrees with the launch rule restated here from the comments of launch_dw;
 - the entries refuse bad arguments and unmet route preconditions before any device call."""
import itertools

import pytest
import torch

from jolineedle_amd import _lib
from tests import dw_cases as dc


def _unique(cases):
    """One case per distinct computation (routes and launch options share inputs and reference)."""
    seen, out = set(), []
    for c in cases:
        if dc._key(c) not in seen:
            seen.add(dc._key(c))
            out.append(c)
    return out


# ---- the case list itself ---------------------------------------------------------------------------------------------------
def test_every_kernel_meets_every_edge_and_option():
    # dw3x3_lds_kernel 4 fp32 + 3 bf16, dw3x3_kernel 2 x 2, dwpw_eval_kernel 7 x 2, dw_bwd_fused_kernel 3 x 2, the unfused route 2
    assert len(dc.KERNELS) == 7 + 4 + 14 + 6 + 2
    for name, cases in dc.KERNELS.items():
        c0 = cases[0]
        two = dc.TWO_TILES[c0.stride]
        assert {(c.H, c.W) for c in cases} == set(dc.SPATIAL[c0.stride]), name
        assert all(c.C == c0.C for c in cases if (c.H, c.W) != two), name      # the spatial edges at one channel count: 32, else 16
        chans = {c.C for c in cases}
        if c0.kind == "dwpw":
            assert chans == {16, 32, 64} and c0.C == 32 and all(c.cout == c0.cout for c in cases), name
        elif "lds_kernel" in name or "fused_kernel" in name:
            cb = int(name.split("<")[1].split(",")[1])
            every16 = c0.stride == 2 and (c0.dtype or c0.kind == "bwd")       # blocks of 16 whatever the count
            assert chans == (set(dc.CHANNELS) if every16 else {32, 64} if cb == 32 else {16, 48}), (name, chans)
            assert c0.C == (32 if 32 in chans else 16), name
        else:
            assert chans == set(dc.CHANNELS) and c0.C == 32, name             # the strip kernels take any count: C = 48 included
        opt = lambda **kw: any((c.H, c.W) == two and all(getattr(c, k) == v for k, v in kw.items()) for c in cases)
        if c0.kind == "fwd":
            assert opt(stats=1, skip=0, nrep=32) and opt(stats=1, nrep=8) and opt(stats=1, skip=1) and opt(stats=1, skip=2), name
            assert all(opt(C=C, stats=1, nrep=8) for C in chans), name      # statistics at every channel count, C = 48 included
        elif c0.kind == "dwpw":
            assert opt(res=0, skip=0) and opt(res=1, skip=0) and opt(skip=1) and opt(skip=2), name
        else:
            assert all(opt(slots=s) for s in (1, 3)) and all(opt(use_wpart=u) for u in (0, 1)) and all(opt(max_wg=m) for m in (0, 1, 2)), name
            assert all(c.red == c0.red for c in cases) and c0.red == int(name.endswith("true>")), name
            assert c0.red or (opt(accumulate=1, slots=1) and opt(accumulate=1, slots=3)), name
            assert not any(c.red and c.accumulate for c in cases), name
        if c0.stride == 2:      # the odd inputs
            assert {(9, 11), (33, 35)} <= {(c.H, c.W) for c in cases}, name
    names = list(dc.KERNELS)
    for dt in ("float", "bf16_t"):
        assert sum(n.startswith("dwpw_eval_kernel") and n.endswith(dt + ">") for n in names) == 7


def test_the_persistent_loop_runs_several_tiles_per_workgroup():
    for name, cases in dc.KERNELS.items():
        if "fused_kernel" not in name:
            continue
        looping = [c for c in cases if c.max_wg == 2]
        assert looping and all(dc.n_tiles(c) >= 6 for c in looping), name      # at least three tiles per workgroup
        assert any(c.max_wg == 1 and dc.n_tiles(c) >= 6 for c in cases), name


# ---- the bars mean something --------------------------------------------------------------------------------------------------
def test_fp32_arithmetic_meets_the_fp32_bars_with_4x_margin():
    worst = worst_red = 0.0
    for c in _unique([c for c in dc.ALL_CASES if not c.dtype]):
        ref = dc.reference(c)
        got = dc.compute(c, torch.float32)
        assert not dc.over_bars(c, got, ref, margin=4.0), (c, dc.over_bars(c, got, ref, margin=4.0))
        worst = max(worst, dc.distances(got["out"], ref["out"])[0])
        if c.red:
            worst_red = max(worst_red, dc.red_distance(got["red"], ref))
    print(f"fp32 arithmetic: worst relative L2 {worst:.2e}; RED sums in pixel order: worst |delta| / sum |terms| {worst_red:.2e}")
    # the RED bar is this measurement x 4, rounded up to one digit
    assert worst_red <= dc.RED_FP32_MEASURED and 4 * dc.RED_FP32_MEASURED <= dc.RED_BAR <= 6 * dc.RED_FP32_MEASURED


def test_bf16_emulation_meets_the_bf16_bars_with_2x_margin():
    worst = 0.0
    for c in _unique([c for c in dc.ALL_CASES if c.dtype]):
        ref = dc.reference(c)
        got = dc.compute_bf16(c)
        assert not dc.over_bars(c, got, ref, margin=2.0), (c, dc.over_bars(c, got, ref, margin=2.0))
        worst = max(worst, dc.distances(got["out"], ref["out"])[1])
    print(f"bf16 emulation: worst max-norm {worst:.2e}")


# ---- the bars bite ------------------------------------------------------------------------------------------------------------
_second_row_tile = lambda c: dc.out_hw(c)[0] > dc.TH[c.stride]
_second_col_tile = lambda c: dc.out_hw(c)[1] > 16
MUTANTS = {
    "pad_silu": lambda c: True,
    "halo_row": lambda c: c.kind != "bwd" and _second_row_tile(c),
    "halo_col": lambda c: c.kind != "bwd" and _second_col_tile(c),
    "gz_halo_row": lambda c: c.kind == "bwd" and _second_row_tile(c),
    "gz_halo_col": lambda c: c.kind == "bwd" and _second_col_tile(c),
    "drop_last_row": lambda c: c.stride == 2 and c.H % 2 == 1,
    "drop_last_col": lambda c: c.stride == 2 and c.W % 2 == 1,
    "parity": lambda c: c.kind == "bwd" and c.stride == 2,
    "unmirrored": lambda c: c.kind == "bwd",
    "raw_transformed": lambda c: not c.red,
    "no_accumulate": lambda c: c.kind == "bwd",
    "slot_table": lambda c: c.kind == "bwd" and c.slots == 3,
    "no_c2": lambda c: c.kind == "bwd",
    "red_missing_pixel": lambda c: c.red == 1,
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_of_the_reference_exceeds_a_bar_on_every_case_it_applies_to(mutant):
    cases = [c for c in dc.ALL_CASES if MUTANTS[mutant](c)]
    assert cases
    seen = set()
    for c in cases:
        key = dc._key(c)._replace(stats=0)      # (the dtype stays: it decides the bars)
        if key in seen:
            continue
        seen.add(key)
        ref = dc.reference(key)
        got = dc.compute(key, torch.float64, mutant=mutant)
        assert dc.over_bars(key, got, ref), (mutant, c, dc.distances(got["out"], ref["out"]))


# ---- the launch rule ------------------------------------------------------------------------------------------------------------
def rule(N, C, stride, dtype):
    """launch_dw: the LDS-tiled kernel takes whole blocks of 16 channels and one image per grid row (at most 65535); everything
    else goes to the strip kernel."""
    return 1 if C % 16 == 0 and N <= 65535 else 2


@pytest.fixture()
def lib():
    return _lib.load_library()


def test_route_entry_agrees_with_the_restated_rule(lib):
    taken = {1: 0, 2: 0}
    for N, C, stride, dtype in itertools.product((1, 2, 64, 65535, 65536, 100000), (4, 12, 16, 20, 32, 48, 64, 72, 96, 100, 256), (1, 2), (0, 1)):
        got = lib.jn_dw3x3_route(N, C, stride, dtype)
        assert got == rule(N, C, stride, dtype), (N, C, stride, dtype, got)
        taken[got] += 1
    assert taken[1] > 50 and taken[2] > 50
    for c in dc.ALL_CASES:      # every forward case's channels are whole blocks of 16: the rule never picks the strip kernel for them
        if c.kind == "fwd":
            assert lib.jn_dw3x3_route(dc.N, c.C, c.stride, c.dtype) == 1, c


# ---- refusals: every check runs before the first device call, so a made-up address is never touched -----------------------------
P = 4096      # stands for a device pointer


def _dw3x3(lib, **o):
    g = lambda k, d: o.get(k, d)
    C = g("C", 32)
    return lib.jn_dw3x3(g("inp", P), g("in_ld", C + 8), g("tab", P), g("w", P), g("out", P), g("out_ld", C + 4), g("N", 2), g("H", 6), g("W", 6), C,
                        g("stride", 1), g("dtype", 0), g("stats", None), None, 0, g("nrep", 32), g("route", 1), None)


def _dwpw(lib, **o):
    g = lambda k, d: o.get(k, d)
    C, cout = g("C", 32), g("cout", 32)
    return lib.jn_dwpw(g("inp", P), g("in_ld", C + 8), g("itab", P), g("w_dw", P), g("mtab", P), g("w_pw", P), g("out", P), g("out_ld", cout + 4),
                       g("res", None), g("res_ld", cout + 8), g("rtab", None), g("ptab", None), g("N", 2), g("H", 6), g("W", 6), C, cout,
                       g("stride", 1), g("dtype", 0), None, 0, None)


def _dw_bwd(lib, **o):
    g = lambda k, d: o.get(k, d)
    C = g("C", 32)
    return lib.jn_dw_bwd(g("g", P), g("g_ld", C + 8), g("z", P), g("z_ld", C + 8), g("x", P), g("x_ld", C + 8), g("otab", P), g("itab", P),
                         g("save", P), g("consts", P), g("w", P), g("gin", P), g("gin_ld", C + 4), g("accumulate", 0), g("gw", P), g("red", None),
                         g("N", 2), g("H", 6), g("W", 6), C, g("stride", 1), g("slots", 1), g("route", 1), g("use_wpart", 0), g("wpart", None),
                         g("max_wg", 0), None)


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    common = (dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=30), dict(C=8192), dict(stride=0), dict(stride=3), dict(N=4096, H=4096, W=2))
    for bad in common + (dict(inp=None), dict(tab=None), dict(w=None), dict(out=None), dict(in_ld=28), dict(out_ld=28), dict(in_ld=34), dict(out_ld=38),
                         dict(in_ld=8196), dict(dtype=2), dict(dtype=-1), dict(nrep=0), dict(nrep=33), dict(route=-1), dict(route=3)):
        assert _dw3x3(lib, **bad) == -1, bad
    for bad in common + (dict(inp=None), dict(itab=None), dict(w_dw=None), dict(mtab=None), dict(w_pw=None), dict(out=None), dict(in_ld=28),
                              dict(out_ld=28), dict(out_ld=38), dict(dtype=2), dict(cout=0), dict(cout=30), dict(res=P), dict(res=P, rtab=P),
                              dict(res=P, ptab=P), dict(res=P, rtab=P, ptab=P, res_ld=28), dict(res=P, rtab=P, ptab=P, res_ld=34)):
        assert _dwpw(lib, **bad) == -1, bad
    for bad in common + (dict(g=None), dict(z=None), dict(x=None), dict(otab=None), dict(itab=None), dict(save=None), dict(consts=None), dict(w=None),
                         dict(gin=None), dict(gw=None), dict(g_ld=28), dict(z_ld=34), dict(x_ld=28), dict(gin_ld=38), dict(slots=0), dict(slots=65),
                         dict(route=-1), dict(route=3), dict(max_wg=-1), dict(use_wpart=1), dict(red=P, accumulate=1), dict(red=P, route=2)):
        assert _dw_bwd(lib, **bad) == -1, bad
    for bad in (dict(N=0), dict(C=0), dict(C=30), dict(stride=3), dict(stride=0), dict(dtype=2)):
        a = dict(N=2, C=32, stride=1, dtype=0)
        a.update(bad)
        assert lib.jn_dw3x3_route(a["N"], a["C"], a["stride"], a["dtype"]) == -1, bad


def test_a_forced_route_refuses_a_launch_that_misses_its_preconditions(lib):
    # the LDS-tiled forward kernel: whole blocks of 16 channels, one image per grid row
    assert _dw3x3(lib, route=1, C=20) == -1
    assert _dw3x3(lib, route=1, C=40) == -1
    assert _dw3x3(lib, route=1, N=65536, H=1, W=1) == -1
    # the fused forward: what dwpw_supported refuses
    for C, cout, stride in ((20, 32, 1), (32, 40, 1), (80, 32, 1), (128, 128, 1), (32, 256, 1), (32, 48, 1), (32, 96, 1), (32, 16, 2), (32, 48, 2)):
        assert _dwpw(lib, C=C, cout=cout, stride=stride) == -1, (C, cout, stride)
    # the fused backward: whole blocks of 16 channels; the input layer's sums come from it alone
    assert _dw_bwd(lib, route=1, C=20) == -1
    assert _dw_bwd(lib, route=1, C=40) == -1
    assert _dw_bwd(lib, route=0, C=20, red=P) == -1
