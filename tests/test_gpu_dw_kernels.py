"""Every depthwise 3x3 kernel of csrc/kernels_conv.hip and csrc/kernels_bwd.hip on its own, through the context-free entries
jn_dw3x3, jn_dwpw and jn_dw_bwd with a forced route, against the fp64 restatement of tests/dw_cases.py at the smallest shapes with
a tile or channel-block edge (cases, inputs and bars: that module; what the bars are worth on these inputs:
tests/test_dw_cases_cpu.py).

Per case: the forced route within the bars; the channels past the count (leading dimensions C + 8 read, C + 4 written) and the
inputs bit for bit as before; with the skip flag at skip_when nothing written at all; statistics only in the replicas below nrep;
the weight-gradient scratch all zero afterwards; a second run with the same bits wherever every element has one writer (outputs,
data gradients, and dW with max_wg = 1, one slot and no scratch), else to the order of the fp32 atomics (1e-5 of max|dW|); fp64
statistics and RED sums of two runs equal to rtol 1e-12.  Across routes: route 0 gives the bits of the route the rule names; the
two forward routes agree within the relative-L2 bar; the two backward routes agree within the data-gradient and dW bars.

Measured on an MI355X, worst case per kernel against fp64 (every run prints them): relative L2 / max |delta| over max |ref| of
the output or data gradient; then the batch statistics as a share of their bar, dW as max |delta| over max |ref|, RED sums as
|delta| over the sum of |terms|:
  dw3x3_lds_kernel<1, 32, 8, float>   7.27e-08 / 1.62e-07  stats 1.4e-03      dw3x3_lds_kernel<1, 32, 8, bf16_t>  2.44e-03 / 4.15e-03  stats 4.0e-02
  dw3x3_lds_kernel<1, 16, 8, float>   7.50e-08 / 1.49e-07  stats 4.7e-03      dw3x3_lds_kernel<1, 16, 8, bf16_t>  2.35e-03 / 4.08e-03  stats 5.6e-02
  dw3x3_lds_kernel<2, 32, 4, float>   7.40e-08 / 1.57e-07  stats 1.0e-03      dw3x3_lds_kernel<2, 16, 4, bf16_t>  2.47e-03 / 4.92e-03  stats 4.3e-02
  dw3x3_lds_kernel<2, 16, 4, float>   7.24e-08 / 1.71e-07  stats 1.8e-03      dw3x3_kernel<1, bf16_t>             2.44e-03 / 4.15e-03  stats 5.6e-02
  dw3x3_kernel<1, float>              7.27e-08 / 1.62e-07  stats 3.2e-03      dw3x3_kernel<2, bf16_t>             2.47e-03 / 4.92e-03  stats 4.3e-02
  dw3x3_kernel<2, float>              7.40e-08 / 1.57e-07  stats 1.6e-03
  dwpw_eval_kernel<1, 4, 1, float>    1.61e-07 / 2.17e-07                     dwpw_eval_kernel<1, 4, 1, bf16_t>   2.56e-03 / 4.27e-03
  dwpw_eval_kernel<1, 4, 2, float>    1.63e-07 / 3.51e-07                     dwpw_eval_kernel<1, 4, 2, bf16_t>   2.53e-03 / 4.97e-03
  dwpw_eval_kernel<1, 4, 4, float>    1.69e-07 / 2.90e-07                     dwpw_eval_kernel<1, 4, 4, bf16_t>   2.33e-03 / 3.60e-03
  dwpw_eval_kernel<1, 4, 8, float>    1.76e-07 / 3.11e-07                     dwpw_eval_kernel<1, 4, 8, bf16_t>   2.32e-03 / 4.40e-03
  dwpw_eval_kernel<2, 2, 2, float>    1.70e-07 / 2.84e-07                     dwpw_eval_kernel<2, 2, 2, bf16_t>   2.41e-03 / 5.04e-03
  dwpw_eval_kernel<2, 2, 4, float>    1.70e-07 / 2.71e-07                     dwpw_eval_kernel<2, 2, 4, bf16_t>   2.50e-03 / 3.84e-03
  dwpw_eval_kernel<2, 2, 8, float>    1.78e-07 / 4.21e-07                     dwpw_eval_kernel<2, 2, 8, bf16_t>   2.46e-03 / 4.77e-03
  dw_bwd_fused_kernel<1, 32, 8, false>  9.03e-08 / 1.56e-07  dW 1.72e-07      dw_bwd_fused_kernel<1, 32, 8, true>  9.34e-08 / 2.25e-07  dW 2.93e-07  RED 7.68e-08
  dw_bwd_fused_kernel<1, 16, 8, false>  9.19e-08 / 1.29e-07  dW 1.62e-07      dw_bwd_fused_kernel<1, 16, 8, true>  9.21e-08 / 1.64e-07  dW 1.84e-07  RED 5.65e-08
  dw_bwd_fused_kernel<2, 16, 4, false>  7.87e-08 / 2.36e-07  dW 1.75e-07      dw_bwd_fused_kernel<2, 16, 4, true>  8.24e-08 / 2.86e-07  dW 2.02e-07  RED 5.90e-08
  bn_bwd_gz, dw_bwd_data<1>, dw_bwd_weight<1>  8.93e-08 / 1.96e-07  dW 1.49e-07
  bn_bwd_gz, dw_bwd_data<2>, dw_bwd_weight<2>  7.52e-08 / 2.36e-07  dW 1.88e-07
(bf16 maps: the max-norm bar is 5e-3 max|ref| + 1e-4 on outputs of about 0.01, i.e. about 1.5e-2 of max|ref|.)  Route 0 took the
LDS-tiled forward and the fused backward on all 120 launches, with their bits.  The LDS-tiled and the strip forward kernel gave the
same bits on all 54 launches: both add the nine taps in the same order.  Fused against unfused backward, 36 launches: data gradients
6.2e-08 of |ref| apart, dW 2.3e-07 of max|ref|.

Before this module existed, at C = 48 (C / 4 = 12, no power of two) the strip kernels' butterfly reductions mixed channels: dW of the
unfused route 0.50 (stride 1) and 0.44 (stride 2) of max|dW| from fp64, the forward strip kernel's statistics 4.5e+04 and 3.6e+04
times their bar; that kernel also spread its statistics over all 32 replicas whatever nrep said.  The fused backward's dW and RED sums, and the strip kernels' sums, changed from run to run in the last
fp32 bits (LDS float atomics in the order the waves arrived); they now add their four waves in wave order."""
import collections

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import ptr
from tests import dw_cases as dc
from tests.kernel_helpers import _bits, _dev, _pattern

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Run = collections.namedtuple("Run", "res raw raw0 f64 f64_0 gw wpart inputs_intact")


def _run(c, route):
    """One launch of the case through its entry with `route`."""
    lib = _lib.load_library()
    d = dc.inputs(c)
    OH, OW = dc.out_hw(c)
    dt = torch.bfloat16 if c.dtype else torch.float32
    canary = dc.CANARY_BF16 if c.dtype else dc.CANARY
    pad_in = lambda t, C: _dev(dc.padded(t, C + dc.IN_PAD, canary).to(dt))
    flag = torch.tensor([dc.SKIP_WHEN - 2 + c.skip], dtype=torch.int32, device=DEV) if c.skip else None
    f64 = f64_0 = gw = wpart = None
    res = {}
    if c.kind == "fwd":
        x, tab, w = pad_in(d["x"], c.C), _dev(d["tab"]), _dev(d["w"])
        ins = [x, tab, w]
        raw0 = torch.full((dc.N, OH, OW, c.C + dc.OUT_PAD), canary, dtype=dt, device=DEV)
        if c.stats:
            f64_0 = _pattern(dc.NREP, 2 * c.C)
            f64 = f64_0.clone()
    elif c.kind == "dwpw":
        x, itab, w, mtab, w_pw = pad_in(d["x"], c.C), _dev(d["tab"]), _dev(d["w"]), _dev(d["mtab"]), _dev(d["w_pw"])
        res_t, rtab, ptab = pad_in(d["res"], c.cout), _dev(d["rtab"]), _dev(d["ptab"])
        ins = [x, itab, w, mtab, w_pw, res_t, rtab, ptab]
        raw0 = torch.full((dc.N, OH, OW, c.cout + dc.OUT_PAD), canary, dtype=dt, device=DEV)
    else:
        g, z, x = pad_in(d["g"], c.C), pad_in(d["z"], c.C), pad_in(d["x"], c.C)
        small = [_dev(d[k]) for k in ("otab", "itab", "save", "consts", "w")]
        ins = [g, z, x] + small
        raw0 = _dev(dc.padded(d["gin0"], c.C + dc.OUT_PAD)) if c.accumulate else torch.full((c.slots, dc.N, c.H, c.W, c.C + dc.OUT_PAD), canary, device=DEV)
        gw = _dev(d["gw0"]).clone()
        if c.red:
            f64_0 = _pattern(c.slots, dc.NREP, 2 * c.C)
            f64 = f64_0.clone()
        if c.use_wpart:
            wpart = torch.full((dc.NREP, dc.WPART_MAX), canary, device=DEV)
    before = [t.clone() for t in ins]
    raw = raw0.clone()
    if c.kind == "fwd":
        rc = lib.jn_dw3x3(ptr(x), c.C + dc.IN_PAD, ptr(tab), ptr(w), ptr(raw), c.C + dc.OUT_PAD, dc.N, c.H, c.W, c.C, c.stride, c.dtype,
                          ptr(f64) if c.stats else None, ptr(flag) if c.skip else None, dc.SKIP_WHEN, c.nrep, route, None)
    elif c.kind == "dwpw":
        rc = lib.jn_dwpw(ptr(x), c.C + dc.IN_PAD, ptr(itab), ptr(w), ptr(mtab), ptr(w_pw), ptr(raw), c.cout + dc.OUT_PAD,
                         ptr(res_t) if c.res else None, c.cout + dc.IN_PAD, ptr(rtab) if c.res else None, ptr(ptab) if c.res else None, dc.N,
                         c.H, c.W, c.C, c.cout, c.stride, c.dtype, ptr(flag) if c.skip else None, dc.SKIP_WHEN, None)
    else:
        rc = lib.jn_dw_bwd(ptr(g), c.C + dc.IN_PAD, ptr(z), c.C + dc.IN_PAD, ptr(x), c.C + dc.IN_PAD, *[ptr(t) for t in small], ptr(raw),
                           c.C + dc.OUT_PAD, c.accumulate, ptr(gw), ptr(f64) if c.red else None, dc.N, c.H, c.W, c.C, c.stride, c.slots, route,
                           c.use_wpart, ptr(wpart) if c.use_wpart else None, c.max_wg, None)
    _lib.check(rc, f"{c}")
    torch.cuda.synchronize()
    n_out = c.cout if c.kind == "dwpw" else c.C
    res["out"] = raw[..., :n_out].float().cpu()
    if c.kind == "fwd" and c.stats:      # [2, C]: the replicas summed, (sum, sum of squares) per channel
        res["stats"] = (f64 - f64_0).sum(0).reshape(c.C, 2).t().cpu()
    if c.kind == "bwd":
        res["dw"] = gw.cpu()
        if c.red:
            res["red"] = (f64 - f64_0).sum(1).reshape(c.slots, c.C, 2).permute(0, 2, 1).cpu()
    return Run(res, raw.cpu(), raw0.cpu(), None if f64 is None else f64.cpu(), None if f64_0 is None else f64_0.cpu(),
               None if gw is None else gw.cpu(), None if wpart is None else wpart.cpu(), all(torch.equal(a, b) for a, b in zip(ins, before)))


def _single_writer(c):
    return c.max_wg == 1 and c.slots == 1 and not c.use_wpart


def _same_launch_twice(c, a, b, ref):
    """Two runs of one launch: the bits wherever an element has one writer, else the order of the atomics."""
    assert _bits(a.raw, b.raw), ("two runs differ", c)
    if c.kind == "bwd":
        if _single_writer(c):
            assert _bits(a.gw, b.gw), ("two runs differ in dW", c)
        else:
            d = (a.gw - b.gw).abs().max().item() / ref["dw"].abs().max().item()
            assert d <= dc.DW_ORDER, ("two runs differ in dW by more than the order of their atomics", c, d)
    if a.f64 is not None:
        assert torch.allclose(a.f64, b.f64, rtol=1e-12, atol=0), ("fp64 sums of two runs differ", c)


@pytest.mark.parametrize("name", list(dc.KERNELS))
def test_kernel_against_fp64_at_tile_and_channel_edges(name):
    worst = collections.defaultdict(float)
    cases = dc.KERNELS[name]
    for c in cases:
        r = _run(c, c.route)
        assert r.inputs_intact, c
        n_out = c.cout if c.kind == "dwpw" else c.C
        assert _bits(r.raw[..., n_out:], r.raw0[..., n_out:]), ("canary", c)
        if c.skip == 2:
            assert _bits(r.raw, r.raw0), ("a skipped launch wrote its output", c)
            assert r.f64 is None or torch.equal(r.f64, r.f64_0), ("a skipped launch wrote its statistics", c)
            continue
        if c.kind == "fwd" and c.stats:
            assert torch.equal(r.f64[c.nrep:], r.f64_0[c.nrep:]), ("statistics in a replica past nrep", c)
        if c.use_wpart:
            assert bool((r.wpart == 0).all()), ("the weight-gradient scratch was not left zero", c)
        ref = dc.reference(c)
        l2, mx = dc.distances(r.res["out"], ref["out"])
        worst["l2"], worst["max"] = max(worst["l2"], l2), max(worst["max"], mx)
        line = f"  {c}: rel L2 {l2:.2e} max {mx:.2e}"
        if "stats" in ref:
            OH, OW = dc.out_hw(c)
            st = dc.stats_over_bar(r.res["stats"], ref["stats"], dc.N * OH * OW)
            worst["stats"] = max(worst["stats"], st)
            line += f" stats {st:.2e} of their bar"
        if "dw" in ref:
            dw = dc.distances(r.res["dw"], ref["dw"])[1]
            worst["dw"] = max(worst["dw"], dw)
            line += f" dW {dw:.2e}"
        if "red" in ref:
            rd = dc.red_distance(r.res["red"], ref)
            worst["red"] = max(worst["red"], rd)
            line += f" RED {rd:.2e}"
        print(line)
        assert not dc.over_bars(c, r.res, ref), (c, dc.over_bars(c, r.res, ref))
        _same_launch_twice(c, r, _run(c, c.route), ref)
    print(f"{name}: {len(cases)} cases, worst relative L2 {worst['l2']:.2e}, worst max-norm {worst['max']:.2e}" +
          "".join(f", worst {k} {worst[k]:.2e}" + (" of their bar" if k == "stats" else "") for k in ("stats", "dw", "red") if k in worst))


def _launches(kind):
    """One case per distinct launch of the kind's fp32 and bf16 entries, whatever route it was listed under."""
    seen = {}
    for c in dc.ALL_CASES:
        if c.kind == kind and c.skip != 2:
            seen.setdefault(c._replace(route=0), c)
    return list(seen)


def test_route_0_launches_what_the_rule_names():
    lib = _lib.load_library()
    taken = collections.Counter()
    for c in _launches("fwd") + _launches("bwd"):
        named = lib.jn_dw3x3_route(dc.N, c.C, c.stride, c.dtype) if c.kind == "fwd" else 1      # the plan fuses every C % 16 == 0 layer
        assert named >= 1, c
        taken[(c.kind, c.stride, named)] += 1
        _same_launch_twice(c, _run(c, 0), _run(c, named), dc.reference(c))
    print("route 0 took (kind, stride, route): launches", dict(taken))


def test_forward_routes_agree():
    pairs = same = 0
    for c in _launches("fwd"):
        a, b = _run(c, 1).res["out"], _run(c, 2).res["out"]
        l2 = ((a - b).double().norm() / a.double().norm()).item()
        same += torch.equal(a, b)
        pairs += 1
        assert l2 <= dc.OUT_L2, (c, l2)
    # (both kernels add the nine taps of an output in the same order, rows then columns: nothing here makes their bits differ)
    print(f"LDS-tiled against strip kernel: {pairs} launches, {same} with the same bits")
    assert pairs >= 40


def test_backward_routes_agree():
    pairs = 0
    worst_dx = worst_dw = 0.0
    for c in _launches("bwd"):
        if c.red:
            continue
        ref = dc.reference(c)
        a, b = _run(c, 1).res, _run(c, 2).res
        dx = ((a["out"] - b["out"]).double().norm() / ref["out"].norm()).item()
        dw = (a["dw"] - b["dw"]).abs().max().item() / ref["dw"].abs().max().item()
        worst_dx, worst_dw = max(worst_dx, dx), max(worst_dw, dw)
        assert dx <= dc.OUT_L2 and dw <= dc.DW_MAX, (c, dx, dw)
        pairs += 1
    print(f"fused against unfused backward: {pairs} launches, data gradient apart by {worst_dx:.2e} of |ref|, dW by {worst_dw:.2e} of max|ref|")
    assert pairs >= 20


def test_entries_refuse_bad_arguments():
    """With real device tensors, as test_gpu_conv3_kernels.py::test_entry_refuses_bad_arguments: a refused call leaves its outputs
    alone.  (The checks need no device; tests/test_dw_cases_cpu.py runs the full list.)"""
    lib = _lib.load_library()
    c = dc.KERNELS["dw3x3_lds_kernel<1, 16, 8, float>"][0]
    d = dc.inputs(c)
    x, tab, w = _dev(dc.padded(d["x"], c.C + 8)), _dev(d["tab"]), _dev(d["w"])
    out = torch.full((dc.N, c.H, c.W, c.C + 4), dc.CANARY, device=DEV)
    args = lambda **o: [ptr(x), o.get("in_ld", c.C + 8), ptr(tab), ptr(w), ptr(out), c.C + 4, o.get("N", dc.N), c.H, c.W, o.get("C", c.C),
                        o.get("stride", 1), o.get("dtype", 0), None, None, 0, o.get("nrep", 32), o.get("route", 1), None]
    for bad in (dict(N=0), dict(C=14), dict(C=12), dict(in_ld=c.C + 2), dict(stride=3), dict(dtype=2), dict(nrep=0), dict(route=3), dict(route=-1)):
        assert lib.jn_dw3x3(*args(**bad)) == -1, bad
    a = args()
    a[0] = None
    assert lib.jn_dw3x3(*a) == -1
    cb = dc.KERNELS["dw_bwd_fused_kernel<1, 16, 8, false>"][0]
    db = dc.inputs(cb)
    t = {k: _dev(dc.padded(db[k], cb.C + 8)) for k in ("g", "z", "x")}
    s = {k: _dev(db[k]) for k in ("otab", "itab", "save", "consts", "w")}
    gin = torch.full((1, dc.N, cb.H, cb.W, cb.C + 4), dc.CANARY, device=DEV)
    gw = torch.full((9, cb.C), dc.CANARY, device=DEV)
    bargs = lambda **o: [ptr(t["g"]), cb.C + 8, ptr(t["z"]), cb.C + 8, ptr(t["x"]), cb.C + 8, ptr(s["otab"]), ptr(s["itab"]), ptr(s["save"]),
                         ptr(s["consts"]), ptr(s["w"]), ptr(gin), o.get("gin_ld", cb.C + 4), o.get("accumulate", 0), ptr(gw), o.get("red", None),
                         dc.N, cb.H, cb.W, o.get("C", cb.C), 1, o.get("slots", 1), o.get("route", 1), o.get("use_wpart", 0), None,
                         o.get("max_wg", 0), None]
    red = torch.zeros(dc.NREP, 2 * cb.C, dtype=torch.float64, device=DEV)
    for bad in (dict(C=12), dict(gin_ld=cb.C + 2), dict(slots=0), dict(route=3), dict(use_wpart=1), dict(max_wg=-1), dict(red=ptr(red), accumulate=1),
                dict(red=ptr(red), route=2)):
        assert lib.jn_dw_bwd(*bargs(**bad)) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == dc.CANARY).all()) and bool((gin == dc.CANARY).all()) and bool((gw == dc.CANARY).all()) and bool((red == 0).all())
