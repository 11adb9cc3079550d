"""CPU side of the 1x1 conv kernel pins (tests/pw_cases.py, tests/test_gpu_pw_kernels.py):
 - every case is admissible: the forced route of every jn_pw case admits its launch (jn_pw_route, host code, no device call), the
   restated tile selection of pw_mfma_kernel agrees with the library on every MFMA case, and the shapes of the other two entries
   are the ones their launchers take;
 - the MFMA cases between them reach every (CT, KC, WM) the selection function returns for the type combinations in use;
 - every kernel family meets every edge and option the case list promises;
 - the bars mean something on the cases' inputs: plain fp32 arithmetic meets the fp32 bars with 4x to spare, the emulations of the
   split products and of bf16 storage meet theirs with 2x;
 - the bars bite: every mistake a kernel of this family can plausibly make puts the reference over a bar on every case it applies
   to;
 - the entries refuse bad arguments and unmet route preconditions before any device call."""
import ctypes
import itertools

import pytest
import torch

from jolineedle_amd import _lib
from tests import pw_cases as pc


@pytest.fixture()
def lib():
    return _lib.load_library()


def _unique(cases):
    """One case per distinct computation (routes and launch options share inputs and reference)."""
    seen, out = set(), []
    for c in cases:
        if pc._key(c) not in seen:
            seen.add(pc._key(c))
            out.append(c)
    return out


def _route(lib, c, route, variant=None):
    with pc.launch_env(c):
        return lib.jn_pw_route(*pc.route_args(c, route), variant)


# ---- the case list itself ---------------------------------------------------------------------------------------------------
def test_every_case_is_admissible(lib):
    v = (ctypes.c_int32 * 3)()
    for name, cases in pc.KERNELS.items():
        for c in cases:
            if c.kind == "pw":
                assert _route(lib, c, c.route, v) == c.route, (name, c)
                assert c.max_wg == 0 or c.route != pc.MFMA, c
                if c.route == pc.MFMA:
                    assert tuple(v) == pc.mfma_variant(c) and name == pc.mfma_name(c), (name, c, tuple(v))
                assert not c.identity or bool((pc.inputs(c)["tab"][:, 2] == 0).all()), c
                assert not c.defer or (c.slots == 1 and c.cin % 4 == 0), c
            elif c.kind == "bdx3":      # pw_x3_bwd_data_supported; its fp32 twin is a launch of the WIDE route
                assert (c.cout, c.cin) in ((256, 128), (256, 256), (256, 512), (128, 256)), c
                assert _route(lib, pc.f32_twin(c), pc.WIDE) == pc.WIDE, c
            else:
                wide = c.cin >= 128 and c.cout >= 128
                assert (not c.exact or wide) and (not c.use_wpart or (not wide and c.cin * c.cout <= pc.WPART_MAX)), c
                cn, ck = (min(4, -(-x // 16)) for x in (c.cout, c.cin))
                assert wide or name == f"pw_bwd_weight_kernel<{cn}, {ck}>", (name, c)
    for c in pc.ALL_CASES:      # a split case's fp32 twin runs the same computation
        if pc.is_split(c) and c.kind == "pw":
            assert _route(lib, pc.f32_twin(c), pc.XS) == pc.XS, c


def test_the_mfma_cases_reach_every_tile_variant_the_selection_returns(lib):
    """The selection over a grid of launches (channels 4 .. 272, pixel counts on both sides of both thresholds, the data-gradient
    hook on and off), per type combination in use, against what the cases reach."""
    v = (ctypes.c_int32 * 3)()
    reached = {}
    for name, cases in pc.KERNELS.items():
        if name.startswith("pw_mfma_kernel"):
            for c in cases:
                reached.setdefault((c.dt, c.transposed), set()).add(pc.mfma_variant(c))
    combos = ((0, 0), (0, 1), (1, 1), (2, 0), (3, 0))      # pw_mfma_types as the networks use them (kernels_conv.hip)
    assert set(reached) == set(combos)
    total = 0
    for dt, tr in combos:
        possible = set()
        for cin, cout, M, big in itertools.product(range(4, 204, 12), range(4, 276, 4), (6, pc.TINY_M + 16, pc.WT_SMALL_M + 16), (0, 1) if tr else (0,)):
            c = pc._case("pw", pc.MFMA, M, cin, cout, dt=dt, transposed=tr, wt_big=big)
            assert _route(lib, c, pc.MFMA, v) == pc.MFMA
            assert tuple(v) == pc.mfma_variant(c), (c, tuple(v))
            possible.add(tuple(v))
        assert reached[(dt, tr)] == possible, (dt, tr, sorted(possible - reached[(dt, tr)]), sorted(reached[(dt, tr)] - possible))
        total += len(possible)
    assert total == 16 + 20 + 8 + 7 + 7
    assert len([n for n in pc.KERNELS if n.startswith("pw_mfma_kernel")]) == total


def test_every_kernel_meets_every_edge_and_option():
    names = list(pc.KERNELS)
    count = lambda prefix: sum(n.startswith(prefix) for n in names)
    assert count("pw_narrow_kernel") == 6 and count("pw_xs_kernel") == 8 + 1 and count("pw_x3_kernel") == 8 + 8 + 2
    assert count("pw_dir_kernel") == 2 + 3 * 2 and count("w_split3_t_kernel") == 3
    assert count("pw_bwd_weight_kernel") == 16 and count("pw_bwd_weight_wide_kernel") == 2
    assert {(c.cin, c.cout) for c in pc.KERNELS["pw_narrow_kernel<2, 16>"]} == {(16, 32), (16, 24)}
    assert {(c.cin, c.cout) for c in pc.KERNELS["pw_narrow_kernel<8, 64>"]} == {(64, 128), (64, 120)}
    assert {(c.cin, c.cout) for n, cs in pc.KERNELS.items() if n.startswith("pw_dir_kernel") and "false, 2, true, true" in n for c in cs} == \
        {(64, 64), (128, 96), (192, 64), (256, 68), (512, 256), (320, 128)}
    forward_routes = {}
    for name, cases in pc.KERNELS.items():
        c0 = cases[0]
        opt = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in cases)
        if c0.kind == "bw":
            assert {c.M for c in cases} == ({300} if "wide" in name else {5, 65, 200}) and {c.slots for c in cases} == {1, 3}, name
            assert "wide" in name or (opt(use_wpart=0) and opt(use_wpart=1)), name
            continue
        if c0.kind == "bdx3":
            assert {c.slots for c in cases} == {1, 3} and {c.max_wg for c in cases} == {0, 1, 2} and opt(M=5), name
            continue
        assert opt(M=5) or c0.up or c0.M > pc.TINY_M, name
        if c0.route != pc.MFMA and not c0.up:      # the persistent loops: three tiles per workgroup, the last partial
            assert opt(max_wg=1) and opt(max_wg=2), name
        forward = not c0.transposed and c0.dt == 0
        if forward:
            r = forward_routes.setdefault(c0.route, set())
            for c in cases:
                r |= {k for k in ("defer1", "defer2", "nrep8", "skip1", "skip2", "stats") if
                      (k == "defer1" and c.defer == 1) or (k == "defer2" and c.defer == 2) or (k == "nrep8" and c.stats and c.nrep == 8) or
                      (k == "skip1" and c.skip == 1) or (k == "skip2" and c.skip == 2) or (k == "stats" and c.stats and c.nrep == 32)}
    for route in (pc.X3, pc.XS, pc.WIDE, pc.NARROW, pc.MFMA):      # deferred tables in both forms, nrep = 8, the skip flag: every forward route
        assert forward_routes[route] == {"defer1", "defer2", "nrep8", "skip1", "skip2", "stats"}, (route, forward_routes[route])
    for c in pc.ALL_CASES:
        if c.kind == "pw" and c.stats and c.nrep == 8 and c.max_wg == 0 and not c.skip and not c.defer:
            assert c.M >= 9 * 16 + 5, c      # more workgroups than replicas (the GPU test checks the replicas past nrep)


def test_the_persistent_loops_run_three_tiles_per_workgroup():
    tile = lambda n, c: (64 if int(n.split("<")[1].split(",")[0]) % 2 == 0 else 128) if n.startswith("pw_narrow") else \
        16 * 4 if n.startswith("pw_dir") else 16 * int(n.split(",")[2])
    for name, cases in pc.KERNELS.items():
        for c in cases:
            if c.kind == "pw" and c.max_wg and not c.up:
                bm = tile(name, c)
                tiles = -(-c.M // bm)
                assert tiles == 3 * c.max_wg and c.M % bm != 0, (name, c, bm)
            if c.kind == "bdx3" and c.max_wg:
                assert -(-c.M // 32) == 3 * c.max_wg and c.M % 32 != 0, c


# ---- the bars mean something --------------------------------------------------------------------------------------------------
def _margin_check(select, margin):
    worst = 0.0
    for c in _unique([c for c in pc.ALL_CASES if select(c)]):
        ref = pc.reference(c)
        got = pc.emulate(c)
        assert not pc.over_bars(c, got, ref, margin=margin), (c, pc.over_bars(c, got, ref, margin=margin))
        worst = max(worst, pc.distances(got[0], ref[0])[0])
    return worst


def test_fp32_arithmetic_meets_the_fp32_bars_with_4x_margin():
    plain = lambda c: not pc.is_bf16(c) and not pc.is_split(c) and not (c.kind == "bw" and c.cin >= 128 and not c.exact)
    print(f"fp32 arithmetic: worst relative L2 {_margin_check(plain, 4.0):.2e}")


def test_split_emulation_meets_the_bars_with_2x_margin():
    split = lambda c: pc.is_split(c) or (c.kind == "bw" and c.cin >= 128 and not c.exact)
    print(f"split products: worst relative L2 {_margin_check(split, 2.0):.2e}")


def test_bf16_emulation_meets_the_bf16_bars_with_2x_margin():
    print(f"bf16 pipe: worst relative L2 {_margin_check(pc.is_bf16, 2.0):.2e}")
    worst = max(pc.distances(pc.emulate(c)[0], pc.reference(c)[0])[1] for c in _unique([c for c in pc.ALL_CASES if pc.is_bf16(c) and c.dt != 2]))
    print(f"fp32 maps on the bf16 pipe: worst max-norm {worst:.2e} of max|ref|")
    # the max-norm bar of those cases is this measurement x 2
    assert worst <= pc.BF16_PIPE_MEASURED and 2 * pc.BF16_PIPE_MEASURED <= pc.BF16_PIPE_MAX <= 2.5 * pc.BF16_PIPE_MEASURED


# ---- the bars bite ------------------------------------------------------------------------------------------------------------
_pw = lambda c: c.kind == "pw"
MUTANTS = {
    "drop_last_k_quad": _pw,
    "drop_last_pixel": _pw,
    "tile_shift": lambda c: _pw(c) and c.cout >= 32,
    "slot_table": lambda c: c.kind in ("pw", "bw") and c.slots == 3 and not c.identity,
    "flag_ignored": lambda c: c.kind in ("pw", "bw"),
    "table_ignored": lambda c: c.kind in ("pw", "bw") and not c.identity,
    "seven_replicas": lambda c: c.defer != 0,
    "var_unclamped": lambda c: c.defer != 0,
    "over_limit_derived": lambda c: c.defer != 0,
    "no_accumulate": lambda c: _pw(c) and c.accumulate,
    "bias_after_act": lambda c: _pw(c) and c.bias and c.act,
    "stats_before_accumulate": lambda c: _pw(c) and c.stats and c.accumulate,
    "untransposed": lambda c: _pw(c) and c.transposed and c.cin == c.cout,
    "second_half_missing": lambda c: c.kind == "bdx3" and c.cin == 512,
    "missing_slot": lambda c: c.kind == "bw" and c.slots == 3,
    "missing_row": lambda c: c.kind == "bw",
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_of_the_reference_exceeds_a_bar_on_every_case_it_applies_to(mutant):
    cases = _unique([c for c in pc.ALL_CASES if MUTANTS[mutant](c)])
    assert cases
    for c in cases:
        key = pc._key(c)
        ref = pc.reference(key)
        if key.dt >= 2:      # (the reference of bf16 maps is taken from rounded inputs; a mutant of the plain one is compared with the plain one)
            ref = pc.compute(key)
        got = pc.compute(key, torch.float64, mutant=mutant)
        assert pc.over_bars(key, got, ref), (mutant, c, pc.distances(got[0], ref[0]))


def test_split_emulation_without_the_hi_lo_product_exceeds_a_bar_on_every_split_case():
    for c in _unique([c for c in pc.ALL_CASES if pc.is_split(c) or (c.kind == "bw" and c.cin >= 128 and not c.exact)]):
        got = pc.compute_split(c, drop_hi_lo=True)
        assert pc.over_bars(c, got, pc.reference(c)), (c, pc.distances(got[0], pc.reference(c)[0]))


# ---- refusals: every check runs before the first device call, so a made-up address is never touched -----------------------------
P = 4096      # stands for a device pointer
_KEEP = []    # descriptors handed to the library by address


def _pw_call(lib, **o):
    g = lambda k, d: o.get(k, d)
    cin, cout, M = g("cin", 32), g("cout", 24), g("W", 6)
    return lib.jn_pw(g("inp", P), g("in_ld", cin + 8), g("dtype_in", 0), g("tab", P), g("defer", None), g("w", P), g("bias", None), g("out", P),
                     g("out_ld", cout + 4), g("dtype_out", 0), g("N", 2), g("H", 1), M, cin, cout, g("bf16_mfma", 0), g("transposed", 0),
                     g("identity", 0), g("accumulate", 0), g("act", 0), g("stats", None), g("nrep", 32), None, 0, g("slots", 1), g("in_ss", 0),
                     g("out_ss", 0), g("tab_ss", 0), g("up", None), g("up_ld", cout + 4), g("route", pc.MFMA), g("max_wg", 0), None)


def _defer(lib, cin=32, **o):
    d = pc.defer_struct(pc._case("pw", pc.MFMA, 12, cin, 24), P, P, 2 * (cin + 16) + 6, 1)
    for k, v in o.items():
        if k.startswith("run"):
            setattr(d.run[int(k[3])], k[5:], v)
        else:
            setattr(d, k, v)
    _KEEP.append(d)
    return ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)


def test_entries_refuse_bad_arguments_before_any_device_call(lib):
    for bad in (dict(inp=None), dict(tab=None), dict(w=None), dict(out=None), dict(N=0), dict(H=0), dict(W=-1), dict(N=4096, H=4096, W=2), dict(cin=0),
                dict(cin=30), dict(cin=8192), dict(cout=0), dict(cout=22), dict(in_ld=28), dict(in_ld=34), dict(in_ld=8196), dict(out_ld=20),
                dict(out_ld=26), dict(dtype_in=2), dict(dtype_out=-1), dict(act=4), dict(act=-1), dict(nrep=0), dict(nrep=33), dict(route=-1),
                dict(route=7), dict(max_wg=-1), dict(max_wg=1), dict(slots=0), dict(slots=65), dict(slots=3), dict(slots=3, in_ss=480, out_ss=300),
                dict(slots=3, in_ss=482, out_ss=336), dict(in_ss=-4), dict(up=P), dict(up=P, route=pc.XS, cin=256, cout=128, up_ld=124),
                dict(up=P, route=pc.XS, cin=256, cout=128, dtype_out=1), dict(dtype_in=1), dict(dtype_in=1, dtype_out=1),
                dict(defer=_defer(lib), slots=3, in_ss=480, out_ss=336), dict(defer=_defer(lib, n_runs=0)), dict(defer=_defer(lib, n_runs=5)),
                dict(defer=_defer(lib, sums_dev=None)), dict(defer=_defer(lib, params_dev=None)), dict(defer=_defer(lib, dN=0)),
                dict(defer=_defer(lib, run1_c0=4)), dict(defer=_defer(lib, run3_c1=36)), dict(defer=_defer(lib, run0_hw=0.0)),
                dict(defer=_defer(lib, rep_stride=40)), dict(defer=_defer(lib, run0_g0=-1))):
        assert _pw_call(lib, **bad) == -1, bad
    bdx3 = lambda **o: lib.jn_pw_bwd_data_x3(o.get("gz", P), o.get("g_ld", 264), o.get("w", P), o.get("gx", P), o.get("gx_ld", 132), o.get("M", 6),
                                             o.get("cout", 256), o.get("cin", 128), o.get("slots", 1), o.get("max_wg", 0), None)
    for bad in (dict(gz=None), dict(w=None), dict(gx=None), dict(g_ld=252), dict(g_ld=262), dict(gx_ld=124), dict(M=0), dict(M=2 ** 24 + 1), dict(slots=0),
                dict(slots=65), dict(max_wg=-1), dict(cout=128, g_ld=136), dict(cout=256, cin=64, gx_ld=68), dict(cout=512, g_ld=520, cin=256, gx_ld=260),
                dict(cout=128, g_ld=136, cin=512, gx_ld=516)):
        assert bdx3(**bad) == -1, bad
    bw = lambda **o: lib.jn_pw_bwd_weight(o.get("gz", P), o.get("g_ld", o.get("cout", 24) + 8), o.get("x", P), o.get("x_ld", o.get("cin", 40) + 8),
                                          o.get("tab", P), o.get("gw", P), o.get("M", 6), o.get("cout", 24), o.get("cin", 40), o.get("slots", 1),
                                          o.get("gz_ss", 6 * (o.get("cout", 24) + 8)), o.get("use_wpart", 0), o.get("wpart", None), o.get("exact", 0), None)
    for bad in (dict(gz=None), dict(x=None), dict(tab=None), dict(gw=None), dict(g_ld=20), dict(g_ld=30), dict(x_ld=36), dict(M=0), dict(cout=22),
                dict(cin=0), dict(slots=0), dict(slots=65), dict(gz_ss=188), dict(gz_ss=194), dict(exact=1), dict(exact=2), dict(exact=-1),
                dict(use_wpart=1), dict(use_wpart=1, wpart=P, cout=128, cin=136, gz_ss=6 * 136), dict(use_wpart=1, wpart=P, cout=64, cin=260, gz_ss=6 * 72)):
        assert bw(**bad) == -1, bad
    for bad in (dict(N=0), dict(cin=30), dict(in_ld=28), dict(out_ld=26), dict(dtype_in=2), dict(act=4), dict(slots=0), dict(route=7), dict(route=-1)):
        a = dict(N=2, H=1, W=6, cin=32, cout=24, in_ld=40, out_ld=28, dtype_in=0, dtype_out=0, bf16_mfma=0, transposed=0, accumulate=0, has_bias=0, act=0,
                 slots=1, has_up=0, route=0)
        a.update(bad)
        assert lib.jn_pw_route(*a.values(), None) == -1, bad


def test_a_forced_route_refuses_a_launch_that_misses_its_preconditions(lib):
    for bad in (dict(route=pc.NARROW, cin=32, cout=48), dict(route=pc.NARROW, cin=32, cout=32, accumulate=1), dict(route=pc.NARROW, cin=32, cout=32, slots=3, in_ss=480, out_ss=432),
                dict(route=pc.NARROW, cin=32, cout=32, transposed=1), dict(route=pc.NARROW, cin=32, cout=32, bias=P), dict(route=pc.NARROW, cin=64, cout=32),
                dict(route=pc.XS), dict(route=pc.XS, cin=64, cout=256), dict(route=pc.XS, cin=256, cout=64), dict(route=pc.XS, cin=512, cout=128),
                dict(route=pc.XS, cin=128, cout=128, accumulate=1), dict(route=pc.XS, cin=128, cout=128, act=1),
                dict(route=pc.X3, cin=64, cout=256), dict(route=pc.X3, cin=128, cout=128, transposed=1), dict(route=pc.X3, cin=128, cout=128, bf16_mfma=1),
                dict(route=pc.X1, cin=128, cout=128), dict(route=pc.X1, cin=128, cout=128, dtype_in=1, dtype_out=0, bf16_mfma=1),
                dict(route=pc.X1, cin=128, cout=96, dtype_in=1, dtype_out=1, bf16_mfma=1),
                dict(route=pc.WIDE), dict(route=pc.WIDE, cin=96, cout=64), dict(route=pc.WIDE, cin=64, cout=32), dict(route=pc.WIDE, cin=576, cout=64),
                dict(route=pc.WIDE, cin=64, cout=64, bias=P), dict(route=pc.WIDE, cin=64, cout=64, bf16_mfma=1),
                dict(route=pc.MFMA, dtype_in=1), dict(route=pc.MFMA, dtype_out=1), dict(route=pc.MFMA, dtype_in=1, dtype_out=1),
                dict(route=pc.X3, cin=128, cout=128, up=P, up_ld=132), dict(route=pc.XS, cin=128, cout=64, up=P, up_ld=68),
                dict(route=pc.WIDE, cin=256, cout=128, up=P, up_ld=132), dict(route=pc.MFMA, cin=256, cout=128, up=P, up_ld=132),
                dict(route=0, cin=128, cout=128, up=P, up_ld=132)):
        assert _pw_call(lib, **bad) == -1, bad
