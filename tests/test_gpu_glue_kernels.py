"""Every kernel that runs between the convolutions of a train-mode pass on its own (csrc/kernels_conv.hip: stem, SPP, upsample,
shortcut sum, BatchNorm tables, embed_fpn linear; csrc/kernels_bwd.hip: the BatchNorm sums, the stem's weight gradient, the SPP and
upsample backward), through the context-free entries jn_stem, jn_stem_bwd_weight, jn_spp, jn_spp_bwd, jn_upsample, jn_upsample_bwd,
jn_addact, jn_bn_finalize, jn_bn_finalize_all, jn_bn_bwd_sums and jn_efpn_linear, against the fp64 restatements of tests/glue_cases.py
at the smallest shapes with an edge (cases, inputs and bars: that module; what the bars are worth on these inputs:
tests/test_glue_cases_cpu.py).

Per case: the bars, or the exact bits where the arithmetic is exact (max-pools of raw channels, the SPP backward's integer
gradients, the upsample copy, integer upsample gradients); the inputs and the channels past the count bit for bit as before; with
the skip flag at skip_when nothing written at all; statistics only in the replicas below nrep; the weight-gradient scratch all zero
afterwards; a second run with the same bits wherever an element has one writer, else to the order of the fp32 atomics (1e-5 of
max|dW|, 1e-5 of a BatchNorm sum's |terms|); fp64 statistics of two runs equal to rtol 1e-12.  Across routes and paths: SPP route 0
gives the bits of the route the rule names, the quad and the scalar SPP kernels the same bits forward and backward, the stem's
16-byte and 4-byte paths and its fp32 and uint8 sources the same bits, and max_wg changes no output bit and dW by at most 1e-5.

Measured on an MI355X, worst case per kernel against fp64 (every run prints them):
relative L2 / max |delta| over max |ref| of the output; then the batch statistics as a share of their bar, dW as max |delta| over
max |ref|, sums and BatchNorm values as |delta| over the sum of |terms|:
  stem_mfma_kernel<float, true, float | uint8_t>      1.92e-07 / 4.85e-07  stats 6.7e-03
  stem_mfma_kernel<float, false, float | uint8_t>     1.98e-07 / 5.19e-07  stats 5.8e-03
  stem_mfma_kernel<bf16_t, true, float | uint8_t>     1.68e-03 / 3.34e-03  stats 6.7e-03
  stem_mfma_kernel<bf16_t, false, float | uint8_t>    1.67e-03 / 3.33e-03  stats 5.8e-03
  stem_bwd_weight_kernel<true, float | uint8_t>       dW 5.81e-07          stem_bwd_weight_kernel<false, float | uint8_t>  dW 5.67e-07
  spp4_kernel<4>, spp_kernel<float>                   5.66e-08 / 1.27e-07 on transformed channels, raw channels to the bit
  spp_kernel<bf16_t>                                  1.68e-03 / 2.37e-03 on transformed channels, raw channels to the bit
  spp4_bwd_kernel<4>, spp_bwd_kernel                  the reference's bits on all 17 cases
  upsample_kernel<float | bf16_t>                     the input's bits        upsample_bwd_kernel  4.72e-08 / 8.73e-08 (integer gradients: bits)
  addact_kernel<float>                                6.12e-08 / 1.24e-07     addact_kernel<bf16_t>  1.74e-03 / 3.11e-03
  bn_finalize_kernel                                  1.19e-07 (bar 8e-7)     bn_finalize_all_kernel  9.97e-08
  bn_bwd_reduce_kernel, bn_bwd_consts_kernel          sums 2.20e-07 (bar 3e-6), consts and parameter gradients 2.47e-07, k 5.90e-08 (bar 1.19e-07)
  efpn_linear_mfma_kernel                             2.08e-07 (bar 5e-7)     efpn_linear_kernel  1.55e-07
(The uint8 source gives the figures of the fp32 one: the same bits.)  Route 0 took the quad SPP kernel on 15 launches and the scalar
one on 12, with their bits; the quad and the scalar kernel gave the same bits on all 15 launches both admit, forward and backward.
Stem: 84 launches on the 16-byte path against the 4-byte path, 58 with the fp32 against the uint8 source, 20 with max_wg = 1 or 5
against the launcher's grid: the same output bits throughout, dW at most 6.2e-07 of max|dW| apart.

The pin found no fault in a kernel's arithmetic: the tie rule of the SPP backward, the stem's persistent walk and its image window,
the butterfly of bn_bwd_reduce_kernel at C / 4 = 12 and the empty K slice all held.  Before this module existed the launchers took
arguments their kernels cannot serve, launched, and returned 0: launch_bn_bwd_reduce with C > 1024 (no thread active: the sums stayed
zero) or C % 4 != 0, launch_efpn_linear's scalar form with Co > 256 (all-zero partial sums), launch_spp and launch_spp_bwd with h
no multiple of their channel block (the remainder channels never pooled), with N > 65535 or with more LDS than a workgroup gets on
the scalar route, the stem launchers with an odd P or cout % 16 != 0, the upsample, shortcut-sum and copy launchers with C % 4 != 0.
They now return -1 before anything is launched (tests/test_glue_cases_cpu.py runs the list; no test launches such a shape), and the
network path checks every one of these return values."""
import collections

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import ptr
from tests import glue_cases as gc
from tests.kernel_helpers import _dev, _pattern

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Run = collections.namedtuple("Run", "res outs outs0 f64 f64_0 wpart inputs_intact")      # outs: name -> raw buffer after the launch; outs0: before


def _opt(t):
    return None if t is None else ptr(t)


def _bits(a, b):
    view = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
    return a.shape == b.shape and torch.equal(a.view(view[a.dtype]), b.view(view[b.dtype]))


def _flag(c):
    return torch.tensor([gc.SKIP_WHEN - 2 + c.skip], dtype=torch.int32, device=DEV) if c.skip else None


def _types(c):
    return (torch.bfloat16, gc.CANARY_BF16) if c.dtype else (torch.float32, gc.CANARY)


def _finish(rc, c, res, outs, outs0, ins, before, f64=None, f64_0=None, wpart=None):
    _lib.check(rc, f"{c}")
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return Run(res(), {k: v.cpu() for k, v in outs.items()}, {k: v.cpu() for k, v in outs0.items()}, cpu(f64), cpu(f64_0), cpu(wpart),
               all(torch.equal(a, b) for a, b in zip(ins, before)))


# ---- one launch of a case ---------------------------------------------------------------------------------------------------------------
def _run_stem(c):
    lib = _lib.load_library()
    d = gc.inputs(c)
    flat, off, ss, cs, rs, pos = gc.stem_image(c, bool(c.src))
    img = _dev(flat)
    base = img.data_ptr() + off * img.element_size()
    pos_d = None if pos is None else _dev(pos)
    OH, cout = c.P // 2, c.cout
    flag = _flag(c)
    if c.kind == "stem":
        dt, canary = _types(c)
        w = _dev(gc.stem_pack(d["w_t"]))
        out0 = torch.full((gc.N, OH, OH, cout + gc.OUT_PAD), canary, dtype=dt, device=DEV)
        out = out0.clone()
        f64_0 = _pattern(gc.NREP, 2 * cout) if c.stats else None
        f64 = None if f64_0 is None else f64_0.clone()
        ins = [img, w] + ([] if pos_d is None else [pos_d])
        before = [t.clone() for t in ins]
        rc = lib.jn_stem(base, c.src, _opt(pos_d), 2, ss, cs, rs, c.P, gc.N, cout, ptr(w), ptr(out), cout + gc.OUT_PAD, c.dtype, _opt(f64), c.nrep,
                         _opt(flag), gc.SKIP_WHEN, c.max_wg, None)

        def res():
            r = dict(out=out[..., :cout].float().cpu())
            if c.stats:
                r["stats"] = (f64 - f64_0).sum(0).reshape(cout, 2).t().cpu()
            return r
        return _finish(rc, c, res, dict(out=out), dict(out=out0), ins, before, f64, f64_0)
    S = c.slots
    pad = lambda t: _dev(gc.padded(t, cout + gc.IN_PAD))
    g, zz = pad(d["g"]), pad(d["zz"]) if c.z else None
    otab, save, consts = (_dev(d[k]) if c.z else None for k in ("otab", "save", "consts"))
    gw0 = _dev(d["gw0"])
    gw = gw0.clone()
    wpart = torch.zeros(gc.NREP, gc.WPART_MAX, device=DEV)
    ins = [t for t in (img, g, zz, otab, save, consts, pos_d) if t is not None]
    before = [t.clone() for t in ins]
    assert pos is None or pos.shape[0] == S
    rc = lib.jn_stem_bwd_weight(base, c.src, _opt(pos_d), 2, 2 * gc.N, ss, cs, rs, c.P, gc.N, cout, ptr(g), cout + gc.IN_PAD, _opt(zz), cout + gc.IN_PAD,
                                _opt(otab), _opt(save), _opt(consts), ptr(gw), ptr(wpart), S, c.max_wg, None)
    return _finish(rc, c, lambda: dict(dw=gw.cpu()), dict(gw=gw), dict(gw=gw0), ins, before, wpart=wpart)


def _run_spp(c, route):
    lib = _lib.load_library()
    d = gc.inputs(c)
    h, ld = c.C, 4 * c.C + gc.IN_PAD
    dt, canary = _types(c)
    tab = _dev(d["tab"])
    cat0 = torch.full((c.slots, gc.N, c.H, c.W, ld), canary, dtype=dt)
    cat0[..., :h] = d["x"].to(dt)
    cat0 = _dev(cat0)
    if c.kind == "spp":
        cat, flag = cat0.clone(), _flag(c)
        before = [tab.clone()]
        rc = lib.jn_spp(ptr(cat), c.dtype, ld, h, c.H, c.W, gc.N, ptr(tab), _opt(flag), gc.SKIP_WHEN, route, None)
        res = lambda: dict(pooled=cat[0, ..., h:4 * h].float().reshape(gc.N, c.H, c.W, 3, h).permute(3, 0, 1, 2, 4).cpu())
        return _finish(rc, c, res, dict(cat=cat), dict(cat=cat0), [tab], before)
    gcat0 = torch.full((c.slots, gc.N, c.H, c.W, ld), gc.CANARY)
    gcat0[..., :h] = d["g0"]
    for i in range(3):
        gcat0[..., (i + 1) * h:(i + 2) * h] = d["g"][i]
    gcat0 = _dev(gcat0)
    gcat = gcat0.clone()
    ins = [cat0, tab]
    before = [t.clone() for t in ins]
    rc = lib.jn_spp_bwd(ptr(cat0), ptr(gcat), ld, h, c.H, c.W, gc.N, ptr(tab), c.slots, route, None)
    return _finish(rc, c, lambda: dict(g0=gcat[..., :h].cpu()), dict(gcat=gcat), dict(gcat=gcat0), ins, before)


def _run_up(c):
    lib = _lib.load_library()
    d = gc.inputs(c)
    dt, canary = _types(c)
    C, flag = c.C, _flag(c)
    if c.kind == "up":
        x = _dev(gc.padded(d["x"], C + gc.IN_PAD, canary).to(dt))
        out0 = torch.full((gc.N, 2 * c.H, 2 * c.W, C + gc.OUT_PAD), canary, dtype=dt, device=DEV)
        out, ins = out0.clone(), [x]
        before = [x.clone()]
        rc = lib.jn_upsample(ptr(x), C + gc.IN_PAD, ptr(out), C + gc.OUT_PAD, c.dtype, C, c.H, c.W, gc.N, _opt(flag), gc.SKIP_WHEN, None)
    elif c.kind == "upb":
        g = _dev(gc.padded(d["g"], C + gc.IN_PAD))
        out0 = _dev(gc.padded(d["gsrc0"], C + gc.OUT_PAD)) if c.accumulate else torch.full((c.slots, gc.N, c.H, c.W, C + gc.OUT_PAD), gc.CANARY, device=DEV)
        out, ins = out0.clone(), [g]
        before = [g.clone()]
        rc = lib.jn_upsample_bwd(ptr(g), C + gc.IN_PAD, ptr(out), C + gc.OUT_PAD, C, c.H, c.W, gc.N, c.accumulate, c.slots, None)
    else:
        z, r = (_dev(gc.padded(d[k], C + gc.IN_PAD, canary).to(dt)) for k in ("z", "res"))
        zt, rt = _dev(d["ztab"]), _dev(d["rtab"])
        out0 = torch.full((c.M, C + gc.OUT_PAD), canary, dtype=dt, device=DEV)
        out, ins = out0.clone(), [z, r, zt, rt]
        before = [t.clone() for t in ins]
        rc = lib.jn_addact(ptr(z), C + gc.IN_PAD, ptr(zt), ptr(r), C + gc.IN_PAD, ptr(rt), ptr(out), C + gc.OUT_PAD, c.dtype, C, c.M, _opt(flag),
                           gc.SKIP_WHEN, None)
    return _finish(rc, c, lambda: dict(out=out[..., :C].float().cpu()), dict(out=out), dict(out=out0), ins, before)


def _run_bnf(c):
    lib = _lib.load_library()
    d = gc.inputs(c)
    C, flag = c.C, _flag(c)
    stats, gamma, beta = _dev(d["stats"]), _dev(d["gamma"]), _dev(d["beta"])
    outs0 = dict(tab0=torch.full((3, C), gc.CANARY, device=DEV))
    if c.t1:
        outs0["tab1"] = torch.full((3, C), gc.CANARY, device=DEV)
    if c.save:
        outs0["save"] = torch.full((C, 2), gc.CANARY, device=DEV)
    if c.run:
        outs0["run_mean"], outs0["run_var"] = _dev(d["run_mean0"]), _dev(d["run_var0"])
    outs = {k: v.clone() for k, v in outs0.items()}
    ins = [stats, gamma, beta]
    before = [t.clone() for t in ins]
    rc = lib.jn_bn_finalize(ptr(stats), stats.shape[1], float(c.M), ptr(gamma), ptr(beta), _opt(outs.get("run_mean")), _opt(outs.get("run_var")),
                            _opt(outs.get("save")), ptr(outs["tab0"]), _opt(outs.get("tab1")), C, gc.BN_EPS, gc.BN_MOMENTUM, _opt(flag), gc.SKIP_WHEN, None)

    def res():
        o = {k: v.cpu() for k, v in outs.items()}
        sv = o.get("save")
        return dict(bn=(o["tab0"][0], o["tab0"][1], None if sv is None else sv[:, 0], None if sv is None else sv[:, 1], o.get("run_mean"), o.get("run_var")))
    return _finish(rc, c, res, outs, outs0, ins, before)


def _run_bnall(c):
    lib = _lib.load_library()
    d = gc.inputs(c)
    n, tc, flag = d["n_stat"], d["tab_channels"], _flag(c)
    ins = [_dev(d[k]) for k in ("stats", "hw", "goff", "boff", "params", "t0", "t1")]
    before = [t.clone() for t in ins]
    outs0 = dict(tab=torch.full((3, tc), gc.CANARY, device=DEV), save=torch.full((n, 2), gc.CANARY, device=DEV), run_mean=_dev(d["run_mean0"]),
                 run_var=_dev(d["run_var0"]))
    outs = {k: v.clone() for k, v in outs0.items()}
    rc = lib.jn_bn_finalize_all(ptr(ins[0]), 2 * n, n, gc.N, *[ptr(t) for t in ins[1:]], ptr(outs["tab"]), tc, ptr(outs["save"]), ptr(outs["run_mean"]),
                                ptr(outs["run_var"]), gc.BN_EPS, gc.BN_MOMENTUM, _opt(flag), gc.SKIP_WHEN, gc.BNALL_DEFER_MAX_M, None)

    def res():
        o = {k: v.cpu() for k, v in outs.items()}
        layers, i0 = [], 0
        for hw_l, C, _ in gc.BNALL_LAYERS:
            idx = torch.arange(i0, i0 + C)
            t0 = d["t0"][idx].long()
            layers.append(None if hw_l <= 0 else (o["tab"][0, t0], o["tab"][1, t0], o["save"][idx, 0], o["save"][idx, 1], o["run_mean"][idx], o["run_var"][idx]))
            i0 += C
        return dict(layers=layers)
    return _finish(rc, c, res, outs, outs0, ins, before)


def _run_bnb(c):
    """Two launches: the reduce kernel alone onto preloaded accumulators, then (consts) both kernels in one call from zeroed ones; with a
    raw moment the consts kernel alone from the sums a consumer would have left."""
    lib = _lib.load_library()
    d = gc.inputs(c)
    C, S = c.C, c.slots
    g, z = (_dev(gc.padded(d[k], C + gc.IN_PAD)) for k in ("g", "z"))
    small = [_dev(d[k]) for k in ("tab", "save", "gamma", "beta")]
    tab, save, gamma, beta = small
    ins = [g, z] + small
    before = [t.clone() for t in ins]
    res, f64 = {}, None
    f64_0 = _pattern(S, gc.NREP, 2 * C)
    if not c.raw:
        f64 = f64_0.clone()
        _lib.check(lib.jn_bn_bwd_sums(ptr(g), C + gc.IN_PAD, ptr(z), C + gc.IN_PAD, ptr(tab), ptr(save), C, c.M, S, ptr(f64), None, None, None, None, None,
                                      1, 0, None), f"{c}")
    outs0, outs = {}, {}
    rc = 0
    if c.consts:
        outs0 = dict(consts=torch.full((S, C, 3), gc.CANARY, device=DEV), g_gamma=_dev(d["g_gamma0"]), g_beta=_dev(d["g_beta0"]))
        outs = {k: v.clone() for k, v in outs0.items()}
        red = _dev(gc.bnb_raw_sums(c).expand(S, gc.NREP, 2 * C)) if c.raw else torch.zeros(S, gc.NREP, 2 * C, dtype=torch.float64, device=DEV)
        rc = lib.jn_bn_bwd_sums(ptr(g), C + gc.IN_PAD, ptr(z), C + gc.IN_PAD, ptr(tab), ptr(save), C, c.M, S, ptr(red), ptr(gamma), ptr(beta),
                                ptr(outs["consts"]), ptr(outs["g_gamma"]), ptr(outs["g_beta"]), 0 if c.raw else 1, c.raw, None)

    def result():
        if f64 is not None:
            res["red"] = (f64 - f64_0).sum(1).reshape(S, C, 2).permute(0, 2, 1).cpu()
        res.update({k: v.cpu() for k, v in outs.items()})
        return res
    return _finish(rc, c, result, outs, outs0, ins, before, f64, None if f64 is None else f64_0)


def _run_ef(c):
    lib = _lib.load_library()
    d = gc.inputs(c)
    e, wt, flag = _dev(d["e"]), _dev(d["wt"]), _flag(c)
    part0 = torch.full((c.N, c.KS, c.C), gc.CANARY, device=DEV)
    part, ins = part0.clone(), [e, wt]
    before = [t.clone() for t in ins]
    rc = lib.jn_efpn_linear(ptr(e), ptr(wt), ptr(part), c.N, c.K, c.C, c.KS, _opt(flag), gc.SKIP_WHEN, None)
    return _finish(rc, c, lambda: dict(part=part.cpu()), dict(part=part), dict(part=part0), ins, before)


def _run(c, route=None):
    if c.kind in ("stem", "stemw"):
        return _run_stem(c)
    if c.kind in ("spp", "sppb"):
        return _run_spp(c, c.route if route is None else route)
    if c.kind in ("up", "upb", "add"):
        return _run_up(c)
    return {"bnf": _run_bnf, "bnall": _run_bnall, "bnb": _run_bnb, "ef": _run_ef}[c.kind](c)


# ---- what a launch may and may not have touched, and the exact comparisons -------------------------------------------------------------
def _written_channels(c):
    """name of the output buffer, channels the launch may write (the rest must keep their bits)."""
    if c.kind == "stem":
        return "out", slice(0, c.cout)
    if c.kind == "spp":
        return "cat", slice(c.C, 4 * c.C)
    if c.kind == "sppb":
        return "gcat", slice(0, c.C)
    if c.kind in ("up", "upb", "add"):
        return "out", slice(0, c.C)
    return None, None


def _check_untouched(c, r):
    assert r.inputs_intact, ("an input changed", c)
    name, sl = _written_channels(c)
    if name:
        mask = torch.ones(r.outs[name].shape[-1], dtype=torch.bool)
        mask[sl] = False
        assert _bits(r.outs[name][..., mask], r.outs0[name][..., mask]), ("channels outside the output changed", c)
    if c.skip == 2:
        for k in r.outs:
            assert _bits(r.outs[k], r.outs0[k]), ("a skipped launch wrote", k, c)
        assert r.f64 is None or torch.equal(r.f64, r.f64_0), ("a skipped launch wrote its statistics", c)
    if c.kind == "stem" and c.stats:
        assert torch.equal(r.f64[c.nrep:], r.f64_0[c.nrep:]), ("statistics in a replica past nrep", c)
    if r.wpart is not None:
        assert bool((r.wpart == 0).all()), ("the weight-gradient scratch was not left zero", c)


def _check_exact(c, r, ref):
    """The comparisons that have no bar: bits."""
    if c.kind == "spp":
        raw = gc.inputs(c)["tab"][0, 2] == 0
        want = ref["pooled"][..., raw].to(torch.bfloat16 if c.dtype else torch.float32).float()
        assert _bits(r.res["pooled"][..., raw].contiguous(), want.contiguous()), ("the max-pool of a raw channel is not the window maximum", c)
    elif c.kind == "sppb":
        assert _bits(r.res["g0"], ref["g0"].float()), ("a pooled gradient did not reach the first maximum of its window", c,
                                                       int((r.res["g0"].double() != ref["g0"]).sum()))
    elif c.kind == "up":
        assert _bits(r.res["out"], ref["out"].float()), ("the upsampled copy differs", c)
    elif c.kind == "upb" and c.ints:
        assert _bits(r.res["out"], ref["out"].float()), ("integer gradients: the sum of the four children is exact", c)
    elif c.kind == "bnf" and c.t1:
        assert _bits(r.outs["tab1"], r.outs["tab0"]), ("the alias table differs", c)
    if c.kind == "bnf":
        assert bool((r.outs["tab0"][2] == 1).all()), c
    if c.kind == "bnall":
        d, o = gc.inputs(c), r.outs
        live = torch.cat([torch.full((C,), hw_l > 0) for hw_l, C, _ in gc.BNALL_LAYERS])
        t0, t1 = d["t0"].long(), d["t1"].long()
        written = torch.zeros(d["tab_channels"], dtype=torch.bool)
        written[t0[live]] = True
        written[t1[live & (t1 >= 0)]] = True
        assert _bits(o["tab"][:, ~written], r.outs0["tab"][:, ~written]), ("a table column of no live channel changed", c)
        assert bool((o["tab"][2, written] == 1).all()), c
        both = live & (t1 >= 0)
        assert _bits(o["tab"][:, t1[both]], o["tab"][:, t0[both]]), ("an alias column differs", c)
        for k in ("save", "run_mean", "run_var"):
            assert _bits(o[k][~live], r.outs0[k][~live]), ("a layer that is not of this pass was written", k, c)


def _comparable(c, res, ref):
    """(got, ref) as over_bars takes them: SPP over the transformed channels only (the raw ones are held to their bits)."""
    if c.kind == "spp":
        tr = gc.inputs(c)["tab"][0, 2] != 0
        return dict(pooled=res["pooled"][..., tr]), dict(pooled=ref["pooled"][..., tr])
    if c.kind == "sppb":
        return {}, {}
    return res, ref


def _same_launch_twice(c, a, b, ref):
    """Two runs of one launch: the bits wherever an element has one writer, else the order of the atomics."""
    for k in a.outs:
        if k == "gw":
            d = (a.outs[k] - b.outs[k]).abs().max().item() / ref["dw"].abs().max().item()
            assert d <= gc.DW_ORDER, ("two runs differ in dW by more than the order of their atomics", c, d)
        elif k in ("consts", "g_gamma", "g_beta"):      # from sums whose fp32 part was added in the order the waves arrived
            d = (a.outs[k] - b.outs[k]).abs().double()
            if k == "consts":
                assert _bits(a.outs[k][..., 2].contiguous(), b.outs[k][..., 2].contiguous()), ("two runs differ in k", c)
                assert bool((d[..., :2] <= gc.DW_ORDER * ref["consts_abs"]).all()), ("two runs differ by more than the order of their atomics", k, c)
            else:
                assert bool((d <= gc.DW_ORDER * ref[k + "_abs"]).all()), ("two runs differ by more than the order of their atomics", k, c)
        else:
            assert _bits(a.outs[k], b.outs[k]), ("two runs differ", k, c)
    if a.f64 is not None and c.kind == "bnb":
        d = ((a.res["red"] - b.res["red"]).abs() / ref["red_abs"]).max().item()
        assert d <= gc.DW_ORDER, ("the sums of two runs differ by more than the order of their fp32 atomics", c, d)
    elif a.f64 is not None:
        assert torch.allclose(a.f64, b.f64, rtol=1e-12, atol=0), ("fp64 sums of two runs differ", c)


def _distances_line(c, res, ref, worst):
    parts = []

    def note(key, value, fmt="{:.2e}"):
        worst[key] = max(worst[key], value)
        parts.append(f"{key} " + fmt.format(value))
    for k in ("out", "pooled"):
        if k in ref:
            l2, mx = gc.distances(res[k], ref[k])
            note("rel L2", l2)
            note("max", mx)
    if "stats" in ref and "stats" in res:
        note("stats / bar", gc.stats_over_bar(res["stats"], ref["stats"], gc.N * (c.P // 2) ** 2))
    if "dw" in ref:
        note("dW", gc.distances(res["dw"], ref["dw"])[1])
    if "red" in ref and "red" in res:
        note("sums", gc.red_distance(res["red"], ref))
    if "consts" in ref and "consts" in res:
        cd, kd = gc.consts_distances(res, ref)
        note("consts", cd)
        note("k", kd)
    if "part" in ref:
        note("partials", gc.ef_distance(res["part"], ref))
    if "bn" in ref:
        note("BN values", gc.bn_distance(res["bn"], ref["bn"], ref["terms"]))
    if "layers" in ref:
        note("BN values", max(gc.bn_distance(g, r, t) for g, r, t in zip(res["layers"], ref["layers"], ref["terms"]) if r is not None))
    return " ".join(parts) if parts else "the reference's bits"


@pytest.mark.parametrize("name", list(gc.KERNELS))
def test_kernel_against_fp64_at_its_edges(name):
    worst = collections.defaultdict(float)
    cases = gc.KERNELS[name]
    for c in cases:
        r = _run(c)
        _check_untouched(c, r)
        if c.skip == 2:
            continue
        ref = gc.reference(c)
        _check_exact(c, r, ref)
        got, want = _comparable(c, r.res, ref)
        print(f"  {c}: " + _distances_line(c, got, want, worst))
        assert not gc.over_bars(c, got, want), (c, gc.over_bars(c, got, want))
        _same_launch_twice(c, r, _run(c), ref)
    print(f"{name}: {len(cases)} cases, " + ("worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) if worst else "the reference's bits"))


# ---- across routes and paths ------------------------------------------------------------------------------------------------------------
def _launches(*kinds):
    seen = {}
    for c in gc.ALL_CASES:
        if c.kind in kinds and c.skip != 2:
            seen.setdefault(c._replace(route=0), c)
    return list(seen)


def test_spp_route_0_launches_what_the_rule_names_and_both_kernels_give_the_same_bits():
    lib = _lib.load_library()
    taken, pairs = collections.Counter(), 0
    for c in _launches("spp", "sppb"):
        named = lib.jn_spp_route(c.dtype, 4 * c.C + gc.IN_PAD, c.C, c.H, c.W, gc.N, int(c.kind == "sppb"))
        assert named >= 1, c
        taken[(c.kind, named)] += 1
        a, b = _run(c, 0), _run(c, named)
        for k in a.outs:
            assert _bits(a.outs[k], b.outs[k]), ("route 0 and the route the rule names differ", k, c)
        if lib.jn_spp_route(c.dtype, 4 * c.C + gc.IN_PAD, c.C, c.H, c.W, gc.N, int(c.kind == "sppb")) == 1 and c.C % 8 == 0:
            q, s = _run(c, 1), _run(c, 2)
            for k in q.outs:
                assert _bits(q.outs[k], s.outs[k]), ("the quad and the scalar kernel differ", k, c)
            pairs += 1
    print(f"route 0 took (kind, route): launches {dict(taken)}; quad against scalar kernel: {pairs} launches with the same bits")
    assert pairs >= 12


def test_stem_paths_sources_and_workgroup_caps_give_the_same_bits():
    vec_pairs = src_pairs = cap_pairs = 0
    worst_dw = 0.0

    def same(a, b, c, what, same_grid=True):
        nonlocal worst_dw
        if "out" in a.outs:
            assert _bits(a.outs["out"], b.outs["out"]), (what, c)
            if a.f64 is not None and same_grid:
                assert torch.allclose(a.f64, b.f64, rtol=1e-12, atol=0), (what, "statistics", c)
            elif a.f64 is not None:      # another grid: a workgroup's fp32 partial sums span other tiles, and land in other replicas
                assert gc.stats_over_bar(a.res["stats"], b.res["stats"].double(), gc.N * (c.P // 2) ** 2) <= 1.0, (what, "statistics", c)
        else:
            d = (a.outs["gw"] - b.outs["gw"]).abs().max().item() / gc.reference(c)["dw"].abs().max().item()
            worst_dw = max(worst_dw, d)
            assert d <= gc.DW_ORDER, (what, c, d)
    for c in _launches("stem", "stemw"):
        if c.skip or c.dtype:
            continue
        base = _run(c)
        if gc.stem_vec(c) and not c.pos:              # the same images one element off, and with an odd row stride: the 4-byte path
            for align in (1, 2):
                same(base, _run(c._replace(align=align)), c, "16-byte against 4-byte path")
                vec_pairs += 1
        if not c.src:                                 # byte-exact images: k / 255 as fp32, and the bytes themselves
            same(base, _run(c._replace(src=1)), c, "fp32 against uint8 source")
            src_pairs += 1
        if c.max_wg:
            same(base, _run(c._replace(max_wg=0)), c, "max_wg against the launcher's grid", same_grid=False)
            cap_pairs += 1
    print(f"stem: {vec_pairs} 16-byte / 4-byte pairs, {src_pairs} fp32 / uint8 pairs, {cap_pairs} capped / uncapped pairs: the same output bits; "
          f"dW apart by at most {worst_dw:.2e} of max|dW|")
    assert vec_pairs >= 20 and src_pairs >= 40 and cap_pairs >= 8


def test_entries_refuse_bad_arguments():
    """With real device tensors: a refused call leaves its outputs alone.  (The checks need no device; tests/test_glue_cases_cpu.py runs
    the full list.)"""
    lib = _lib.load_library()
    can = lambda *s, dt=torch.float32: torch.full(s, gc.CANARY, dtype=dt, device=DEV)
    f = lambda *s: torch.rand(*s, device=DEV)
    outs = []
    # stem: odd P, cout % 16 != 0
    img, w, out = f(2, 3, 8, 8), f(108, 24), can(2, 4, 4, 28)
    outs.append(out)
    for P, cout in ((7, 16), (8, 24), (8, 8)):
        assert lib.jn_stem(ptr(img), 0, None, 2, 192, 64, 8, P, 2, cout, ptr(w), ptr(out), 28, 0, None, 32, None, 0, 0, None) == -1, (P, cout)
    gw, wpart = can(108, 24), torch.zeros(gc.NREP, gc.WPART_MAX, device=DEV)
    outs.append(gw)
    g = f(2, 4, 4, 32)
    for P, cout in ((7, 16), (8, 24)):
        assert lib.jn_stem_bwd_weight(ptr(img), 0, None, 2, 0, 192, 64, 8, P, 2, cout, ptr(g), 32, None, 32, None, None, None, ptr(gw), ptr(wpart), 1, 0,
                                      None) == -1, (P, cout)
    # SPP: h no multiple of the route's block, ld % 4 != 0 on the quad route
    cat, gcat, tab = can(2, 7, 7, 74), can(2, 7, 7, 74), f(3, 16)
    outs += [cat, gcat]
    for h, ld, route in ((12, 72, 0), (12, 72, 2), (16, 74, 1), (16, 72, 3)):
        assert lib.jn_spp(ptr(cat), 0, ld, h, 7, 7, 2, ptr(tab), None, 0, route, None) == -1, (h, ld, route)
        assert lib.jn_spp_bwd(ptr(cat), ptr(gcat), ld, h, 7, 7, 2, ptr(tab), 1, route, None) == -1, (h, ld, route)
    # upsample, shortcut sum: C % 4 != 0
    x, up, src = f(2, 3, 3, 16), can(2, 6, 6, 12), can(2, 3, 3, 12)
    outs += [up, src]
    assert lib.jn_upsample(ptr(x), 16, ptr(up), 12, 0, 6, 3, 3, 2, None, 0, None) == -1
    assert lib.jn_upsample_bwd(ptr(up), 12, ptr(src), 12, 6, 3, 3, 2, 0, 1, None) == -1
    assert lib.jn_addact(ptr(x), 16, ptr(tab), ptr(x), 16, ptr(tab), ptr(src), 12, 0, 6, 18, None, 0, None) == -1
    # bn_bwd_reduce: C % 4 != 0, C > 1024; the scalar efpn form: Co > 256
    red, big = torch.zeros(gc.NREP, 2 * 1028, dtype=torch.float64, device=DEV), f(3, 1036)
    sv = f(1028, 2)
    outs.append(red)
    for C in (18, 1028):
        assert lib.jn_bn_bwd_sums(ptr(big), 1036, ptr(big), 1036, ptr(f(3, 1028)), ptr(sv), C, 3, 1, ptr(red), None, None, None, None, None, 1, 0, None) == -1, C
    part = can(2, 2, 260)
    outs.append(part)
    assert lib.jn_efpn_linear(ptr(f(2, 40)), ptr(f(40, 260)), ptr(part), 2, 40, 260, 2, None, 0, None) == -1
    torch.cuda.synchronize()
    assert all(bool((o == gc.CANARY).all()) for o in outs if o is not red and o is not wpart) and bool((red == 0).all()) and bool((wpart == 0).all())
