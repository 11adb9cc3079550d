"""CPU side of the pins of the stem, SPP, upsample, shortcut-sum, BatchNorm and embed_fpn kernels (tests/glue_cases.py,
tests/test_gpu_glue_kernels.py):
 - the case list holds every edge and option the kernels have;
 - every restatement equals the torch module it restates, in fp64 to 1e-12: Focus + 3 x 3 conv against the folded 6 x 6 stride-2
   form, the first-in-row-major arg-max against MaxPool2d's autograd on inputs full of ties, nearest upsampling and its autograd,
   BatchNorm2d's train-mode table and running statistics, the BatchNorm sums as parameter gradients, the K-slice sums against Linear;
 - the bars mean something on the cases' inputs: plain fp32 arithmetic stays within every bar (the two bars of this unit are 4 x what
   it measures here), an emulation of bf16 storage within the bf16 bars with 2x to spare;
 - the bars bite: ties sent to the last maximum, a neighbour pixel instead of the zero padding, a dropped last tile column, two
   channels swapped at C / 4 = 12, replicas past nrep summed and an empty K slice left unwritten put the reference over a bar, or
   break an exact comparison, on every case they apply to;
 - jn_spp_route (host code, no device call) agrees with the launch rule restated here;
 - the entries refuse bad arguments, and what their launchers cannot take, before any device call."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from jolineedle_amd import _lib
from tests import glue_cases as gc


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if gc._key(c) not in seen:
            seen.add(gc._key(c))
            out.append(c)
    return out


def _of(*kinds):
    return [c for c in gc.ALL_CASES if c.kind in kinds]


# ---- the case list itself ---------------------------------------------------------------------------------------------------
def test_every_kernel_meets_every_edge_and_option():
    assert len(gc.KERNELS) == 8 + 4 + 5 + 5 + 2 + 1 + 2
    has = lambda cases, **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in cases)
    for name, cases in gc.KERNELS.items():
        c0 = cases[0]
        if c0.kind in ("stem", "stemw"):
            vec = ", true" in name or "<true" in name
            assert all(gc.stem_vec(c) == vec for c in cases), name
            assert all((c.src == 1) == ("uint8_t" in name) and (c.dtype == 1) == ("bf16_t" in name) for c in cases), name
            assert {c.P for c in cases} == ({4, 68, 96} if vec else {30, 66, 68, 96}), name
            assert vec or (has(cases, P=68, align=1) and has(cases, P=68, align=2)), name      # an alignable shape forced onto the 4-byte path
            assert {c.cout for c in cases} == {16, 32, 48} and has(cases, pos=1) and has(cases, P=4 if vec else 30, pos=1), name
            assert all(has(cases, P=96, max_wg=m) for m in (0, 1, 5)), name
            assert all(gc.N * gc.stem_tiles(c)[0] * gc.stem_tiles(c)[1] >= 12 for c in cases if c.max_wg), name      # the workgroups walk
            if c0.kind == "stem":
                assert has(cases, stats=1, nrep=32, skip=0) and has(cases, stats=1, nrep=8) and has(cases, skip=1) and has(cases, skip=2), name
            else:
                assert {c.slots for c in cases} == {1, 3, 4} and all(has(cases, z=z, slots=s) for z in (0, 1) for s in (1, 4)), name
                assert all(has(cases, P=96, z=1, max_wg=m) for m in (1, 5)), name
        elif c0.kind in ("spp", "sppb"):
            assert {(c.H, c.W) for c in cases} == set(gc.SPP_SHAPES), name
            assert {c.C for c in cases} == ({16, 32} if c0.route == 1 else {8, 16, 24}), name
            assert (has(cases, skip=1) and has(cases, skip=2)) if c0.kind == "spp" else has(cases, slots=3), name
        elif c0.kind in ("up", "upb", "add"):
            assert {(c.H, c.W, c.C) for c in cases if c.H} == set((h, w, C) for h, w in gc.UP_SHAPES for C in gc.UP_CHANNELS), name
            if c0.kind == "upb":
                assert all(has(cases, accumulate=a, slots=s, ints=1) for a in (0, 1) for s in (1, 3)) and has(cases, ints=0), name
            else:
                assert has(cases, skip=1) and has(cases, skip=2), name
            if c0.kind == "add":
                assert has(cases, M=1) and (c0.dtype or has(cases, M=gc.ADD_LOOP_M, C=64)), name
        elif c0.kind == "bnf":
            assert {c.C for c in cases} == set(gc.BNF_CHANNELS) and {c.M for c in cases} == set(gc.BNF_COUNTS), name
            assert all(has(cases, **{k: v}) for k in ("t1", "save", "run") for v in (0, 1)) and has(cases, skip=2), name
        elif c0.kind == "bnb":
            assert {c.C for c in cases if not c.raw} == set(gc.BNB_CHANNELS), name
            for C in gc.BNB_CHANNELS:
                rpb = gc.bnb_rows_per_block(C)
                assert has(cases, C=C, M=rpb - 1) and has(cases, C=C, M=rpb + 1) and has(cases, C=C, M=33 * rpb + 3), (name, C)
            assert has(cases, C=16, M=1) and has(cases, C=16, M=2047) and has(cases, C=16, M=33 * 2048 + 3), name
            assert all(has(cases, raw=r, consts=1, slots=s) for r in (0, 1) for s in (1, 3)), name
        elif c0.kind == "ef":
            mfma = "mfma" in name
            assert all((c.C % 16 == 0 and c.K % 4 == 0) == mfma for c in cases), name
            assert {c.N for c in cases} == {1, 3, 65} and {c.C for c in cases} == ({16, 48, 64, 112} if mfma else {24, 40}), name
            ends = lambda c: [min(c.K, (ks + 1) * gc.ef_kper(c)) - min(c.K, ks * gc.ef_kper(c)) for ks in range(c.KS)]
            assert any(0 in ends(c) for c in cases) and has(cases, skip=2), name                      # an empty slice
            assert not mfma or (any(e % 64 for c in cases for e in ends(c) if e > 64) and any(0 < e < 64 for c in cases for e in ends(c))), name
            assert mfma or any(c.K % 4 for c in cases), name
    assert (gc.ADD_LOOP_M * 64 // 4) > 4096 * 256


def test_spp_inputs_have_ties_in_raw_channels_and_none_in_the_others():
    gap, ties = float("inf"), 0
    for c in _unique(_of("spp", "sppb")):
        a = gc.spp_activation(c)                                        # [S, N, h, H, W]
        flag = gc.inputs(c)["tab"][:, 2]                                # [S, h]
        assert bool((gc.inputs(c)["tab"][:, 0] > 0).all())
        for s in range(c.slots):
            per_channel = a[s].permute(1, 0, 2, 3).reshape(c.C, -1)     # a window never spans two images, but the bar holds across them too
            srt = per_channel.sort(1).values
            y = a[s].permute(1, 0, 2, 3)[flag[s] != 0]
            if srt.shape[1] > 1:
                diffs = srt[:, 1:] - srt[:, :-1]
                gap = min(gap, diffs[flag[s] != 0].min().item())
                ties += int((diffs[flag[s] == 0] == 0).sum())
            assert not y.numel() or (0.05 < y.min().item() and y.max().item() < 4.0), c      # silu of y in [0.1, 4]
    print(f"smallest gap between two activations of a transformed channel {gap:.2e}; tied neighbours in raw channels {ties}")
    assert gap > 1e-3 and ties > 1000


# ---- the restatements are the modules ----------------------------------------------------------------------------------------------
def test_folded_stem_conv_is_focus_plus_conv():
    for P, cout in ((4, 16), (30, 32), (66, 48)):
        g = torch.Generator().manual_seed(P)
        x = torch.rand(2, 3, P, P, generator=g, dtype=torch.float64)
        w_t = torch.randn(cout, 12, 3, 3, generator=g, dtype=torch.float64)
        a, b = gc.focus_conv(x, w_t), gc.folded_conv(x, gc.stem_pack(w_t))
        assert a.shape == b.shape == (2, cout, P // 2, P // 2)
        assert (a - b).abs().max().item() <= 1e-12 * a.abs().max().item()
        gz = torch.randn(a.shape, generator=g, dtype=torch.float64)      # and the weight gradient of the folded form is the module's, repacked
        w_leaf = w_t.clone().requires_grad_(True)
        (gc.focus_conv(x, w_leaf) * gz).sum().backward()
        gw = torch.nn.grad.conv2d_weight(F.pad(x, (2, 2, 2, 2)), (cout, 3, 6, 6), gz, stride=2).reshape(cout, 108).t()
        assert (gc.stem_pack(w_leaf.grad) - gw).abs().max().item() <= 1e-12 * gw.abs().max().item()


def test_first_maximum_in_row_major_order_is_maxpool_autograd_on_ties():
    for c in _unique(_of("sppb")):
        a, b = gc.reference(c)["g0"], gc.compute(gc._key(c), mutant="autograd")["g0"]
        assert torch.equal(a, b), c


def test_upsample_shortcut_and_linear_restatements_are_the_modules():
    for c in _unique(_of("up")):
        x = gc.inputs(c)["x"].double()
        want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
        assert torch.equal(gc.reference(c)["out"], want), c
    for c in _unique(_of("upb")):
        d = gc.inputs(c)
        for s in range(c.slots):
            leaf = torch.zeros(gc.N, c.C, c.H, c.W, dtype=torch.float64, requires_grad=True)
            (F.interpolate(leaf, scale_factor=2, mode="nearest") * d["g"][s].double().permute(0, 3, 1, 2)).sum().backward()
            want = leaf.grad.permute(0, 2, 3, 1) + (d["gsrc0"][s].double() if c.accumulate else 0)
            assert (gc.reference(c)["out"][s] - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0), c
    for c in _unique(_of("add")):
        d = {k: (gc._bf16(v) if c.dtype and k in ("z", "res") else v).double() for k, v in gc.inputs(c).items()}      # (bf16 maps: as stored)
        act = lambda x, t: torch.where(t[2] != 0, F.silu(x * t[0] + t[1]), x)
        want = act(d["z"], d["ztab"]) + act(d["res"], d["rtab"])
        assert (gc.reference(c)["out"] - want).abs().max().item() <= 1e-12 * want.abs().max().item(), c
    for c in _unique(_of("ef")):
        d = {k: v.double() for k, v in gc.inputs(c).items()}
        want = F.linear(d["e"], d["wt"].t())
        assert (gc.reference(c)["part"].sum(1) - want).abs().max().item() <= 1e-12 * want.abs().max().item(), c


def test_batchnorm_restatement_is_batchnorm2d_in_train_mode():
    for c in _unique(_of("bnf")):
        if c.M == 1:
            continue      # (BatchNorm2d refuses one value per channel)
        d = gc.inputs(c)
        bn = torch.nn.BatchNorm2d(c.C, eps=gc.BN_EPS, momentum=gc.BN_MOMENTUM).double().train()
        with torch.no_grad():
            bn.weight.copy_(d["gamma"])
            bn.bias.copy_(d["beta"])
            bn.running_mean.copy_(d["run_mean0"])
            bn.running_var.copy_(d["run_var0"])
            y = bn(d["x"].reshape(c.M, c.C, 1, 1)).reshape(c.M, c.C)
        sc, sh, mean, invstd, rm, rv = gc.reference(c)["bn"]
        # E[x^2] - mean^2 from the sums loses |E[x^2]| / (var + eps) of the 1e-16 the sums hold: 1e4 / 1.1e-3 on the channel with mean
        # 100 and deviation 0.01, 1 elsewhere; the tolerance is 1e-12 times that factor
        cond = ((d["x"] ** 2).mean(0) * invstd ** 2).clamp_min(1.0)
        assert bool(((d["x"] * sc + sh - y).abs().max(0).values <= 1e-12 * cond * y.abs().max(0).values.clamp_min(1.0)).all()), c
        assert bool(((rm - bn.running_mean).abs() <= 1e-12 * rm.abs().clamp_min(1.0)).all()), c
        assert bool(((rv - bn.running_var).abs() <= 1e-12 * cond * rv.abs().clamp_min(1.0)).all()), c
        assert bool((invstd[0] == 1.0 / torch.tensor(gc.BN_EPS, dtype=torch.float64).sqrt()) | (invstd[0] > 31.6))      # the constant channel: the clamp


def test_batchnorm_sums_are_the_parameter_gradients():
    for c in _unique(_of("bnb")):
        if c.M > 3000:
            continue
        d = {k: v.double() for k, v in gc.inputs(c).items()}
        ref = gc.reference(c)
        for s in range(c.slots):
            b = torch.zeros(c.C, dtype=torch.float64, requires_grad=True)      # d / d beta' and d / d gamma' of sum g silu(y + beta' + gamma' m)
            t = torch.zeros(c.C, dtype=torch.float64, requires_grad=True)
            y = d["z"][s] * d["tab"][s, 0] + d["tab"][s, 1]
            m = y.detach() if c.raw else (d["z"][s] - d["save"][s, :, 0]) * d["save"][s, :, 1]
            (d["g"][s] * F.silu(y + b + t * m)).sum().backward()
            for got, want in ((ref["red"][s, 0], b.grad), (ref["red"][s, 1], t.grad)):
                assert bool(((got - want).abs() <= 1e-12 * ref["red_abs"][s].max(0).values.clamp_min(1e-300)).all()), c


# ---- the bars mean something --------------------------------------------------------------------------------------------------------
def test_fp32_arithmetic_stays_within_every_bar():
    worst = dict(l2=0.0, dw=0.0, red=0.0, ef=0.0, bn=0.0)
    for c in _unique(gc.ALL_CASES):
        if c.dtype and c.kind != "stem":
            continue
        k = gc._key(c)
        ref, got = gc.reference(c), gc.compute(k, torch.float32)
        assert not gc.over_bars(k, got, ref), (c, gc.over_bars(k, got, ref))
        if "out" in ref:
            worst["l2"] = max(worst["l2"], gc.distances(got["out"], ref["out"])[0])
        if "dw" in ref:
            worst["dw"] = max(worst["dw"], gc.distances(got["dw"], ref["dw"])[1])
        if "red" in ref:
            worst["red"] = max(worst["red"], gc.red_distance(got["red"], ref))
        if "part" in ref:
            worst["ef"] = max(worst["ef"], gc.ef_distance(got["part"], ref))
        if "bn" in ref:
            worst["bn"] = max(worst["bn"], gc.bn_distance(got["bn"], ref["bn"], ref["terms"]))
        if "layers" in ref:
            worst["bn"] = max([worst["bn"]] + [gc.bn_distance(g, r, t) for g, r, t in zip(got["layers"], ref["layers"], ref["terms"]) if r is not None])
        if c.kind == "sppb":      # small integers: fp32 is exact
            assert torch.equal(got["g0"].double(), ref["g0"]), c
    print(f"fp32 arithmetic: worst relative L2 {worst['l2']:.2e}, dW {worst['dw']:.2e}, BatchNorm sums {worst['red']:.2e}; "
          f"embed_fpn partial sums {worst['ef']:.2e}, BatchNorm values {worst['bn']:.2e} of their |terms|")
    # the two bars of this unit are these measurements x 4, rounded up to one digit
    assert worst["ef"] <= gc.EF_FP32_MEASURED and 4 * gc.EF_FP32_MEASURED <= gc.EF_BAR <= 6 * gc.EF_FP32_MEASURED
    assert worst["bn"] <= gc.BN_FP32_MEASURED and 4 * gc.BN_FP32_MEASURED <= gc.BN_BAR <= 6 * gc.BN_FP32_MEASURED


def test_bf16_emulation_meets_the_bf16_bars_with_2x_margin():
    worst = 0.0
    for c in _unique([c for c in gc.ALL_CASES if c.dtype and c.kind in ("spp", "up", "add")]):
        ref, got = gc.reference(c), gc.compute_bf16(c)
        if c.kind == "spp":      # the bars are over the transformed channels; the raw ones are exact
            flag = gc.inputs(c)["tab"][0, 2] != 0
            assert torch.equal(got["pooled"][..., ~flag].double(), ref["pooled"][..., ~flag]), c
            got, ref = dict(pooled=got["pooled"][..., flag]), dict(pooled=ref["pooled"][..., flag])
        assert not gc.over_bars(c, got, ref, margin=2.0), (c, gc.over_bars(c, got, ref, margin=2.0))
        key = "pooled" if c.kind == "spp" else "out"
        worst = max(worst, gc.distances(got[key], ref[key])[1])
    print(f"bf16 emulation: worst max-norm {worst:.2e}")


# ---- the bars bite ------------------------------------------------------------------------------------------------------------
def _empty_slice(c):
    return any(min(c.K, ks * gc.ef_kper(c)) >= c.K for ks in range(c.KS))


MUTANTS = {
    "last_max": lambda c: c.kind == "sppb" and c.H * c.W > 1,                       # ties sent to the last maximum
    "neighbour": lambda c: c.kind in ("stem", "stemw"),                             # a neighbour pixel instead of the zero padding
    "drop_last_col": lambda c: c.kind in ("stem", "stemw") and gc.stem_tiles(c)[1] > 1,      # the last tile column dropped
    "swap": lambda c: c.kind == "bnb" and c.C == 48,                                # two channels swapped at C / 4 = 12
    "all_replicas": lambda c: c.kind == "bnall",                                    # replicas past nrep summed
    "empty_unwritten": lambda c: c.kind == "ef" and _empty_slice(c),                # the empty K slice left unwritten
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_planted_fault_exceeds_a_bar_or_breaks_an_exact_comparison(mutant):
    cases = _unique([c for c in gc.ALL_CASES if MUTANTS[mutant](c)])
    assert cases
    for c in cases:
        k = gc._key(c)
        ref, got = gc.reference(c), gc.compute(k, mutant=mutant)
        if mutant == "last_max":
            assert not torch.equal(got["g0"], ref["g0"]), c
        else:
            assert gc.over_bars(k, got, ref), (mutant, c)


# ---- the launch rule ------------------------------------------------------------------------------------------------------------
def rule(dtype, ld, h, H, W, n, bwd):
    """launch_spp / launch_spp_bwd: the quad kernel takes fp32 maps of whole blocks of 16 channels with 16-byte aligned pixels, forward
    up to 510 pixels (its LDS within 64 KB), backward up to 512 (the elements its threads cover); else the scalar kernel, 8 channels
    per workgroup, 4 where 8 need more than 48 KB (backward: 60 KB) of LDS; -1 where neither takes the launch."""
    if n > 65535 or ld < 4 * h or (bwd and dtype):
        return -1
    if not dtype and h % 16 == 0 and ld % 4 == 0 and H * W <= (512 if bwd else 510):
        return 1
    per = 16 if bwd else 8
    cb = 8 if H * W * 8 * per <= (60 if bwd else 48) * 1024 else 4
    return 2 if h % cb == 0 and H * W * cb * per <= 159 * 1024 else -1


@pytest.fixture()
def lib():
    return _lib.load_library()


def test_route_entry_agrees_with_the_restated_rule(lib):
    taken = {1: 0, 2: 0, -1: 0}
    for dtype, pad, h, hw, n, bwd in itertools.product((0, 1), (0, 2, 8), (4, 8, 12, 16, 24, 32, 48), ((1, 1), (3, 5), (14, 14), (22, 23), (22, 24), (23, 23),
                                                                                                     (28, 28), (40, 40), (56, 56), (80, 80)),
                                                       (1, 2, 65535, 65536), (0, 1)):
        got = lib.jn_spp_route(dtype, 4 * h + pad, h, hw[0], hw[1], n, bwd)
        assert got == rule(dtype, 4 * h + pad, h, hw[0], hw[1], n, bwd), (dtype, pad, h, hw, n, bwd, got)
        taken[got] += 1
    assert min(taken.values()) > 100, taken
    for c in _of("spp", "sppb"):      # the cases' own launches: the rule names the quad kernel wherever it is admitted
        named = lib.jn_spp_route(c.dtype, 4 * c.C + gc.IN_PAD, c.C, c.H, c.W, gc.N, int(c.kind == "sppb"))
        assert named == (1 if c.C % 16 == 0 and not c.dtype else 2), c


# ---- refusals: every check runs before the first device call, so a made-up address is never touched -----------------------------
P = 4096      # stands for a device pointer


def _g(o):
    return lambda k, d: o.get(k, d)


def _stem(lib, **o):
    g = _g(o)
    Pp, cout = g("P", 8), g("cout", 16)
    return lib.jn_stem(g("src", P), g("src_u8", 0), g("positions", None), g("pos_stride", 2), g("sample_stride", 3 * Pp * Pp), g("chan_stride", Pp * Pp),
                       g("row_stride", Pp), Pp, g("N", 2), cout, g("w", P), g("out", P), g("out_ld", cout + 4), g("out_dtype", 0), g("stats", None),
                       g("nrep", 32), None, 0, g("max_wg", 0), None)


def _stem_bwd(lib, **o):
    g = _g(o)
    Pp, cout = g("P", 8), g("cout", 16)
    return lib.jn_stem_bwd_weight(g("src", P), 0, g("positions", None), g("pos_stride", 2), g("pos_slot", 0), 3 * Pp * Pp, Pp * Pp, g("row_stride", Pp), Pp,
                                  g("N", 2), cout, g("g", P), g("g_ld", cout + 8), g("z", None), g("z_ld", cout + 8), g("otab", None), g("save", None),
                                  g("consts", None), g("gw", P), g("wpart", P), g("slots", 1), g("max_wg", 0), None)


def _spp(lib, **o):
    g = _g(o)
    h = g("h", 16)
    return lib.jn_spp(g("cat", P), g("dtype", 0), g("ld", 4 * h + 8), h, g("H", 7), g("W", 7), g("N", 2), g("tab", P), None, 0, g("route", 0), None)


def _spp_bwd(lib, **o):
    g = _g(o)
    h = g("h", 16)
    return lib.jn_spp_bwd(g("cat", P), g("gcat", P), g("ld", 4 * h + 8), h, g("H", 7), g("W", 7), g("N", 2), g("tab", P), g("slots", 1), g("route", 0), None)


def _upsample(lib, **o):
    g = _g(o)
    C = g("C", 8)
    return lib.jn_upsample(g("inp", P), g("in_ld", C + 8), g("out", P), g("out_ld", C + 4), g("dtype", 0), C, g("H", 3), g("W", 3), g("N", 2), None, 0, None)


def _upsample_bwd(lib, **o):
    g = _g(o)
    C = g("C", 8)
    return lib.jn_upsample_bwd(g("gdst", P), g("dst_ld", C + 8), g("gsrc", P), g("src_ld", C + 4), C, g("H", 3), g("W", 3), g("N", 2), g("accumulate", 0),
                               g("slots", 1), None)


def _addact(lib, **o):
    g = _g(o)
    C = g("C", 8)
    return lib.jn_addact(g("z", P), g("z_ld", C + 8), g("ztab", P), g("res", P), g("res_ld", C + 8), g("rtab", P), g("out", P), g("out_ld", C + 4),
                         g("dtype", 0), C, g("M", 10), None, 0, None)


def _bn_finalize(lib, **o):
    g = _g(o)
    C = g("C", 8)
    return lib.jn_bn_finalize(g("stats", P), g("rep_stride", 2 * C), g("count", 10.0), g("gamma", P), g("beta", P), g("run_mean", P), g("run_var", P),
                              g("save", P), g("tab0", P), g("tab1", None), C, g("eps", 1e-3), g("momentum", 0.03), None, 0, None)


def _bn_finalize_all(lib, **o):
    g = _g(o)
    n = g("n_stat", 8)
    return lib.jn_bn_finalize_all(g("stats", P), g("rep_stride", 2 * n), n, g("N", 2), g("hw", P), g("goff", P), g("boff", P), g("params", P), g("t0", P),
                                  g("t1", P), g("tab", P), g("tab_channels", 16), g("save", P), g("run_mean", P), g("run_var", P), 1e-3, 0.03, None, 0,
                                  g("defer_max_m", 1000), None)


def _bn_bwd_sums(lib, **o):
    g = _g(o)
    C = g("C", 16)
    return lib.jn_bn_bwd_sums(g("g", P), g("g_ld", C + 8), g("z", P), g("z_ld", C + 8), g("tab", P), g("save", P), C, g("M", 10), g("slots", 1), g("red", P),
                              g("gamma", P), g("beta", P), g("consts", P), g("g_gamma", P), g("g_beta", P), g("reduce", 1), g("raw", 0), None)


def _efpn(lib, **o):
    g = _g(o)
    return lib.jn_efpn_linear(g("e", P), g("wt", P), g("part", P), g("N", 2), g("K", 40), g("Co", 24), g("KS", 2), None, 0, None)


REFUSALS = {
    # stem: odd P, cout % 16 != 0, a null pointer, a count that is not positive
    _stem: (dict(P=7), dict(P=0), dict(P=-2), dict(cout=8), dict(cout=24), dict(cout=0), dict(N=0), dict(src=None), dict(w=None), dict(out=None),
            dict(out_ld=12), dict(out_ld=18), dict(out_dtype=2), dict(nrep=0), dict(nrep=33), dict(max_wg=-1), dict(row_stride=0), dict(chan_stride=0),
            dict(positions=P, pos_stride=1)),
    _stem_bwd: (dict(P=7), dict(P=0), dict(cout=8), dict(cout=24), dict(cout=160), dict(N=0), dict(src=None), dict(g=None), dict(gw=None), dict(wpart=None),
                dict(g_ld=12), dict(g_ld=18), dict(slots=0), dict(slots=65), dict(max_wg=-1), dict(z=P), dict(z=P, otab=P, save=P), dict(z=P, otab=P, save=P, consts=P, z_ld=12)),
    # SPP: h no multiple of the route's channel block, ld % 4 != 0 on the quad route, LDS above the grant, N > 65535
    _spp: (dict(h=12), dict(h=20, route=1), dict(h=24, route=1), dict(h=12, route=2), dict(ld=74, route=1), dict(dtype=1, route=1), dict(H=23, W=23, route=1),
           dict(H=100, W=100, h=8), dict(H=80, W=80, h=20), dict(N=65536), dict(N=0), dict(H=0), dict(W=0), dict(h=0), dict(ld=60), dict(cat=None), dict(tab=None),
           dict(route=3), dict(route=-1), dict(dtype=2)),
    _spp_bwd: (dict(h=12), dict(h=20, route=1), dict(h=12, route=2), dict(ld=74, route=1), dict(H=23, W=23, route=1), dict(H=100, W=100, h=8),
               dict(H=60, W=60, h=20), dict(N=65536), dict(N=0), dict(H=0), dict(h=0), dict(ld=60), dict(cat=None), dict(gcat=None), dict(tab=None), dict(slots=0),
               dict(slots=65), dict(route=3)),
    # upsample, shortcut sum: C % 4 != 0
    _upsample: (dict(C=6), dict(C=0), dict(in_ld=14, C=8), dict(out_ld=6), dict(out_ld=14), dict(H=0), dict(W=0), dict(N=0), dict(inp=None), dict(out=None),
                dict(dtype=2)),
    _upsample_bwd: (dict(C=6), dict(C=0), dict(dst_ld=14), dict(src_ld=6), dict(src_ld=14), dict(H=0), dict(N=0), dict(gdst=None), dict(gsrc=None), dict(slots=0),
                    dict(slots=65)),
    _addact: (dict(C=6), dict(C=0), dict(C=2052), dict(z_ld=14), dict(res_ld=6), dict(out_ld=14), dict(M=0), dict(z=None), dict(ztab=None), dict(res=None),
              dict(rtab=None), dict(out=None), dict(dtype=2)),
    _bn_finalize: (dict(C=0), dict(count=0.0), dict(rep_stride=14), dict(stats=None), dict(gamma=None), dict(beta=None), dict(tab0=None), dict(run_var=None),
                   dict(run_mean=None), dict(eps=0.0)),
    _bn_finalize_all: (dict(n_stat=0), dict(N=0), dict(rep_stride=14), dict(tab_channels=0), dict(stats=None), dict(hw=None), dict(goff=None), dict(boff=None),
                       dict(params=None), dict(t0=None), dict(t1=None), dict(tab=None), dict(save=None), dict(run_mean=None), dict(run_var=None),
                       dict(defer_max_m=-1)),
    # bn_bwd_reduce: C % 4 != 0 or C > 1024
    _bn_bwd_sums: (dict(C=18), dict(C=1028), dict(C=2048), dict(C=0), dict(M=0), dict(g_ld=12), dict(z_ld=12), dict(slots=0), dict(slots=65), dict(g=None),
                   dict(z=None), dict(tab=None), dict(save=None), dict(red=None), dict(gamma=None), dict(g_beta=None), dict(reduce=0, consts=None),
                   dict(reduce=1, raw=1)),
    # the scalar efpn form: Co > 256
    _efpn: (dict(Co=260), dict(Co=264, K=38), dict(Co=0), dict(N=0), dict(K=0), dict(KS=0), dict(e=None), dict(wt=None), dict(part=None), dict(N=65536)),
}


@pytest.mark.parametrize("entry", list(REFUSALS), ids=lambda f: f.__name__.strip("_"))
def test_entries_refuse_bad_arguments_before_any_device_call(lib, entry):
    for bad in REFUSALS[entry]:
        assert entry(lib, **bad) == -1, bad
    for a in ((0, 72, 16, 7, 7, 65536, 0), (0, 72, 16, 0, 7, 2, 0), (2, 72, 16, 7, 7, 2, 0), (0, 60, 16, 7, 7, 2, 0), (1, 72, 16, 7, 7, 2, 1)):
        assert lib.jn_spp_route(*a) == -1, a
