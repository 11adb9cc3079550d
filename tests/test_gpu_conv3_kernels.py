"""Every dense 3x3 kernel of csrc/kernels_conv3.hip on its own, through the context-free entries jn_conv3,
jn_conv3_bwd_data_s2 and jn_conv3_bwd_weight with a forced route, against the fp64 restatement of tests/conv3_cases.py at the
smallest shapes with a tile or channel-block edge (cases, inputs and bars: that module; what the bars are worth on these
inputs: tests/test_conv3_cases_cpu.py).

Per case: the forced route within the bars; the channels past the count (leading dimensions cin + 8 / cout + 4) and the
inputs bit for bit as before; a second run with the same bits (weight gradients: with one writer per element, else to the
order of their fp32 atomics, 1e-5 of max|dW|); with the skip flag at skip_when nothing written at all.  Per shape: route 0
gives the bits of the route jn_conv3_route names; the split route (2) is no further from fp64 than 1.5 x the fp32 route (1)
+ 1e-6 and differs from it.

Measured on an MI355X, worst case per kernel, relative L2 / max |delta| over max |ref| against fp64 (every run prints them):
  conv3_mfma_kernel<1, float, false>   5.90e-07 / 1.07e-06        conv3_bwd_weight_tr_kernel<1>          4.71e-06 / 5.77e-06
  conv3_x3_kernel<1, false>            4.98e-07 / 1.20e-06        conv3_bwd_weight_kernel<1, 4, true>    4.72e-06 / 5.77e-06
  conv3_mfma_kernel<2, float, false>   5.87e-07 / 1.15e-06        conv3_bwd_weight_kernel<1, 4, false>   4.32e-07 / 8.71e-07
  conv3_x3s2_kernel                    5.10e-07 / 1.09e-06        conv3_bwd_weight_tr_kernel<2>          4.55e-06 / 7.79e-06
  conv3_mfma_kernel<1, float, true>    5.96e-07 / 1.35e-06        conv3_bwd_weight_kernel<2, 4, true>    4.55e-06 / 7.91e-06
  conv3_x3_kernel<1, true>             5.07e-07 / 1.02e-06        conv3_bwd_weight_kernel<2, 4, false>   4.51e-07 / 8.10e-07
  conv3_bwd_data_s2_kernel             3.30e-07 / 7.74e-07        conv3_bf16_kernel<1>                   1.96e-03 / 4.02e-03
  conv3_x3_bwd_data_s2_kernel          2.70e-07 / 6.02e-07        conv3_bf16_kernel<2>                   1.97e-03 / 3.47e-03
Batch statistics: at most 2.4e-3 of their bar.  Split against fp32 route, max-norm: between 0.6 x and 1.9 x (5.97e-07 against
3.13e-07, the 10 x 12 stride-2 data gradient: inside 1.5 x + 1e-6)."""
import collections

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import ptr
from tests import conv3_cases as cc
from tests.kernel_helpers import _bits, _dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Run = collections.namedtuple("Run", "out stats raw raw0 stats_raw stats0 inputs_intact")


def _run(c, route):
    """One launch of the case through its entry with `route`."""
    lib = _lib.load_library()
    d = cc.inputs(c)
    (ld_a, c_a), (ld_b, c_b) = cc.lds(c)
    OH, OW = cc.out_hw(c)
    stats = stats0 = None
    if c.kind == "dw":
        gz, x, tab = _dev(cc.padded(d["gz"], ld_a)), _dev(cc.padded(d["x"], ld_b)), _dev(d["tab"])
        ins = [gz, x, tab]
        before = [t.clone() for t in ins]
        raw0 = _dev(d["prev"])
        raw = raw0.clone()
        rc = lib.jn_conv3_bwd_weight(ptr(gz), ld_a, ptr(x), ld_b, ptr(tab), ptr(raw), cc.N, c.H, c.W, c.cout, c.cin, c.stride, c.slots,
                                     route, c.max_wg, None)
        out = raw
    else:
        bf16 = c.kind == "bf16"
        canary = cc.CANARY_BF16 if bf16 else cc.CANARY
        dt = torch.bfloat16 if bf16 else torch.float32
        xin = _dev(cc.padded(d["x"], ld_a, canary).to(dt))
        w = _dev(d["w"])
        out_shape = (c.slots, cc.N) + ((c.H, c.W) if c.kind == "ds2" else (OH, OW)) + (ld_b,)
        raw0 = _dev(cc.padded(d["prev"], ld_b, canary).to(dt)) if c.accumulate else torch.full(out_shape, canary, dtype=dt, device=DEV)
        assert raw0.shape == out_shape
        raw = raw0.clone()
        ins = [xin, w]
        if c.kind == "ds2":
            before = [t.clone() for t in ins]
            rc = lib.jn_conv3_bwd_data_s2(ptr(xin), ld_a, ptr(w), ptr(raw), ld_b, cc.N, c.H, c.W, c.cout, c.cin, c.accumulate, c.slots,
                                          route, None)
        else:
            tab = _dev(d["tab"][0])
            ins.append(tab)
            before = [t.clone() for t in ins]
            if c.stats:      # the launch adds into the replicas: they start from a pattern, not from zero
                stats0 = (torch.arange(cc.NREP * 2 * c_b, dtype=torch.float64, device=DEV) % 7).reshape(cc.NREP, 2 * c_b)
                stats = stats0.clone()
            flag = torch.tensor([cc.SKIP_WHEN - 2 + c.skip], dtype=torch.int32, device=DEV) if c.skip else None
            rc = lib.jn_conv3(ptr(xin), ld_a, ptr(tab), ptr(w), ptr(raw), ld_b, cc.N, c.H, c.W, c.cin, c.cout, c.stride,
                              int(c.kind == "wt"), c.accumulate, ptr(stats) if c.stats else None, ptr(flag) if c.skip else None,
                              cc.SKIP_WHEN, c.slots, xin[0].numel(), raw[0].numel(), route, None)
        out = raw[..., :c_b]
    _lib.check(rc, f"{c}")
    torch.cuda.synchronize()
    sums = None
    if stats is not None:
        sums = (stats - stats0).sum(0).reshape(c_b, 2).t().cpu()      # [2, C]: the replicas summed, (sum, sum of squares) per channel
    return Run(out.float().cpu(), sums, raw.cpu(), raw0.cpu(), None if stats is None else stats.cpu(),
               None if stats0 is None else stats0.cpu(), all(torch.equal(a, b) for a, b in zip(ins, before)))


def _single_writer(c):
    return c.max_wg == 1 and c.slots == 1


@pytest.mark.parametrize("name", list(cc.KERNELS))
def test_kernel_against_fp64_at_tile_and_channel_edges(name):
    worst_l2 = worst_max = worst_stat = 0.0
    cases = cc.KERNELS[name]
    for c in cases:
        r = _run(c, c.route)
        assert r.inputs_intact, c
        _, c_b = cc.lds(c)[1]
        if c.kind != "dw":      # the channels past the count hold what they held
            assert _bits(r.raw[..., c_b:], r.raw0[..., c_b:]), ("canary", c)
        if c.skip == 2:
            assert _bits(r.raw, r.raw0), ("a skipped launch wrote its output", c)
            assert r.stats_raw is None or torch.equal(r.stats_raw, r.stats0), ("a skipped launch wrote its statistics", c)
            continue
        ref, ref_stats = cc.reference(c)
        l2, mx = cc.distances(r.out, ref)
        worst_l2, worst_max = max(worst_l2, l2), max(worst_max, mx)
        line = f"  {c}: rel L2 {l2:.2e} max {mx:.2e}"
        if c.stats:
            OH, OW = cc.out_hw(c)
            st = cc.stats_over_bar(r.stats, ref_stats, cc.N * OH * OW * c.slots)
            worst_stat = max(worst_stat, st)
            line += f" stats {st:.2e} of their bar"
            assert st <= 1.0, ("stats", c, st)
        print(line)
        assert not cc.over_bars(c, r.out, ref), (c, cc.over_bars(c, r.out, ref))
        again = _run(c, c.route)
        if c.kind != "dw" or _single_writer(c):
            assert _bits(again.raw, r.raw), ("two runs differ", c)
        else:
            d = (again.out - r.out).abs().max().item() / ref.abs().max().item()
            assert d <= cc.DW_ORDER, ("two runs differ by more than the order of their atomics", c, d)
    print(f"{name}: {len(cases)} cases, worst relative L2 {worst_l2:.2e}, worst max-norm {worst_max:.2e}" +
          (f", worst stats {worst_stat:.2e} of their bar" if worst_stat else ""))


def _shapes():
    """One case per distinct launch of the fp32-format entries, whatever route it was listed under."""
    seen = {}
    for c in cc.ALL_CASES:
        if c.kind != "bf16":
            seen.setdefault(c._replace(route=0), c)
    return list(seen)


def test_route_0_launches_what_the_route_entry_names(monkeypatch):
    monkeypatch.delenv("JN_NO_CONV3_X3", raising=False)
    lib = _lib.load_library()
    taken = collections.Counter()
    for c in _shapes():
        (ld_a, _), (ld_b, _) = cc.lds(c)
        named = lib.jn_conv3_route(cc.entry_kind(c), cc.N, c.H, c.W, c.cin, c.cout, c.stride, c.slots, ld_a, ld_b)
        assert named >= 1, c
        taken[(c.kind, c.stride, named)] += 1
        auto, forced = _run(c, 0), _run(c, named)
        if c.kind != "dw" or _single_writer(c):
            assert _bits(auto.raw, forced.raw), (c, named)
        else:      # several workgroups add into a dW element in the order they finish: the same kernel, not the same bits
            ref, _ = cc.reference(c)
            d = (auto.out - forced.out).abs().max().item() / ref.abs().max().item()
            assert d <= cc.DW_ORDER, (c, named, d)
        if auto.stats_raw is not None and c.skip != 2:      # fp64 atomics over the tiles: equal to their order
            assert torch.allclose(auto.stats_raw, forced.stats_raw, rtol=1e-12, atol=0), c
    print("route 0 took (kind, stride, route): shapes", dict(taken))


def test_split_route_is_as_close_to_fp64_as_the_fp32_route_and_is_another_kernel():
    pairs = 0
    for c in cc.ALL_CASES:
        if c.kind not in ("fwd", "wt", "ds2") or c.route != 2 or c.skip == 2:
            continue
        f32 = c._replace(route=1)
        assert f32 in cc.ALL_CASES, c      # the fp32 route's list holds every split case
        ref, _ = cc.reference(c)
        a, b = _run(c, 2), _run(f32, 1)
        e_split, e_f32 = cc.distances(a.out, ref)[1], cc.distances(b.out, ref)[1]
        print(f"  {c}: split {e_split:.2e} fp32 {e_f32:.2e}")
        assert not torch.equal(a.out, b.out), ("the forced routes gave the same bits", c)
        assert e_f32 < cc.OUT_MAX and e_split < cc.SPLIT_VS_F32[0] * e_f32 + cc.SPLIT_VS_F32[1], (c, e_split, e_f32)
        pairs += 1
    assert pairs >= 30


def test_entry_refuses_bad_arguments():
    """With real device tensors, as test_gpu_pw_bwd_fused128.py::test_entry_refuses_bad_arguments: a refused call leaves its
    output alone.  (The checks need no device; tests/test_conv3_cases_cpu.py runs the full list.)"""
    lib = _lib.load_library()
    c = cc.KERNELS["conv3_mfma_kernel<1, float, false>"][0]
    d = cc.inputs(c)
    x, tab, w = _dev(cc.padded(d["x"], c.cin + 8)), _dev(d["tab"][0]), _dev(d["w"])
    out = torch.full((1, cc.N, c.H, c.W, c.cout + 4), cc.CANARY, device=DEV)
    args = lambda **o: [ptr(x), o.get("in_ld", c.cin + 8), ptr(tab), ptr(w), ptr(out), c.cout + 4, o.get("N", cc.N), c.H, c.W,
                        o.get("cin", c.cin), c.cout, o.get("stride", 1), 0, 0, None, None, 0, o.get("slots", 1), 0, 0, o.get("route", 1), None]
    for bad in (dict(N=0), dict(cin=30), dict(in_ld=c.cin + 2), dict(stride=2), dict(stride=3), dict(slots=0), dict(route=4), dict(route=-1)):
        assert lib.jn_conv3(*args(**bad)) == -1, bad
    a = args()
    a[0] = None
    assert lib.jn_conv3(*a) == -1
    torch.cuda.synchronize()
    assert bool((out == cc.CANARY).all())
