"""Every 1x1 conv kernel of csrc/kernels_conv.hip, kernels_pwres.hip, kernels_pwxs.hip and the two weight-gradient kernels of
kernels_bwd_pw.hip on its own, through the context-free entries jn_pw, jn_pw_bwd_data_x3 and jn_pw_bwd_weight with a forced route,
against the fp64 restatement of tests/pw_cases.py at the smallest shapes with a tile or channel edge (cases, inputs and bars: that
module; what the bars are worth on these inputs: tests/test_pw_cases_cpu.py).

Per case: the forced route within the bars; the channels past the count (leading dimensions C + 8 read, C + 4 written), the rows past
M and the inputs bit for bit as before; the fused upsample an exact copy of the output, its buffer beyond the map untouched; with
the skip flag at skip_when nothing written at all; statistics only in the replicas below nrep; the weight-gradient scratch all zero
afterwards; a second run with the same bits in outputs and data gradients, statistics and weight gradients (several atomic writers)
within 1e-5 of their largest element.  Across routes: route 0 gives the bits of the route jn_pw_route names; the split routes (X3,
the split data gradient) are no further from fp64 than 1.5 x the fp32 route + 1e-6 on the same inputs.

Measured on an MI355X, worst case per family against fp64 (every run prints them per kernel): relative L2 / max |delta| over
max |ref|: pw_mfma_kernel fp32 2.4e-07 / 5.2e-07, on the bf16 pipe 2.9e-03 / 4.5e-03; pw_narrow_kernel 1.8e-07 / 3.6e-07; pw_xs_kernel
4.5e-07 / 1.2e-06; pw_x3_kernel 3.7e-07 / 8.9e-07, its bf16 single-plane form 2.8e-03 / 4.8e-03; pw_dir_kernel 4.5e-07 / 1.2e-06; the
split data gradients 2.3e-07 / 6.7e-07; pw_bwd_weight_kernel 1.3e-07 / 2.4e-07, the wide kernel 4.6e-06 / 5.4e-06 (split) and
2.8e-07 / 7.5e-07 (exact); batch statistics at most 2.3e-02 of their bar (0.32 in the bf16 single-plane form).  Route 0 took MFMA on
234 launches, X3 on 74, WIDE on 50 and X1 on 30, with the bits of the named route on all of them.  Split against fp32 route, 77
launches: at most 1.85 x its distance to fp64, inside 1.5 x + 1e-6.  No kernel missed a bar when this module was written."""
import collections
import ctypes

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import ptr
from tests import pw_cases as pc
from tests.kernel_helpers import _bits, _dev, _pattern

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Run = collections.namedtuple("Run", "res raw raw0 f64 f64_0 wpart up up0 inputs_intact")


def _rows(t, ld, canary, row_pad=pc.ROW_PAD, dt=torch.float32):
    """[S, M, C] inside [S, M + row_pad, ld], everything else canary."""
    S, M, C = t.shape
    buf = torch.full((S, M + row_pad, ld), canary, dtype=torch.float32)
    buf[:, :M, :C] = t
    return _dev(buf.to(dt))


def _run(c, route):
    """One launch of the case through its entry with `route`."""
    lib = _lib.load_library()
    d = pc.inputs(c)
    S, M = c.slots, c.M
    f64 = f64_0 = wpart = up = up0 = None
    res = {}
    if c.kind == "pw":
        n, h, w_ = pc.images(c)
        di, do, bf = pc.ENTRY_TYPES[c.dt]
        dt_in, dt_out = (torch.bfloat16 if di else torch.float32), (torch.bfloat16 if do else torch.float32)
        in_ld, out_ld = c.cin + pc.IN_PAD, c.cout + pc.OUT_PAD
        x = _rows(d["x"], in_ld, pc.CANARY_BF16 if di else pc.CANARY, dt=dt_in)
        tab, w, bias = _dev(d["tab"]), _dev(d["w"]), _dev(d["bias"])
        ins = [x, tab, w, bias]
        canary = pc.CANARY_BF16 if do else pc.CANARY
        raw0 = _rows(d["prev"], out_ld, canary, dt=dt_out) if c.accumulate else torch.full((S, M + pc.ROW_PAD, out_ld), canary, dtype=dt_out, device=DEV)
        if c.stats:
            f64_0 = _pattern(pc.NREP, 2 * c.cout)
            f64 = f64_0.clone()
        flag = torch.tensor([pc.SKIP_WHEN - 2 + c.skip], dtype=torch.int32, device=DEV) if c.skip else None
        if c.up:
            up0 = torch.full((n * 4 * h * w_ + pc.ROW_PAD, out_ld), pc.CANARY, device=DEV)
            up = up0.clone()
        defer = None
        if c.defer:
            sums, params = _dev(d["sums"]), _dev(d["params"])
            ins += [sums, params]
            defer = pc.defer_struct(c, sums.data_ptr(), params.data_ptr(), d["rep_stride"], 1 if c.defer == 1 else 0)
        before = [t.clone() for t in ins]
        raw = raw0.clone()
        with pc.launch_env(c):
            rc = lib.jn_pw(ptr(x), in_ld, di, ptr(tab), ctypes.cast(ctypes.pointer(defer), ctypes.c_void_p) if defer else None, ptr(w),
                           ptr(bias) if c.bias else None, ptr(raw), out_ld, do, n, h, w_, c.cin, c.cout, bf, c.transposed, c.identity, c.accumulate,
                           c.act, ptr(f64) if c.stats else None, c.nrep, ptr(flag) if c.skip else None, pc.SKIP_WHEN, S,
                           (M + pc.ROW_PAD) * in_ld, (M + pc.ROW_PAD) * out_ld, 3 * c.cin if S > 1 else 0, ptr(up) if c.up else None, out_ld,
                           route, c.max_wg, None)
        n_out = c.cout
    elif c.kind == "bdx3":      # dense slots (the entry's layout); the rows past the last slot hold the canary
        g_ld, gx_ld = c.cout + pc.IN_PAD, c.cin + pc.OUT_PAD
        x = _rows(d["x"].reshape(1, S * M, c.cout), g_ld, pc.CANARY)
        w = _dev(d["w"])
        ins = [x, w]
        raw0 = torch.full((1, S * M + pc.ROW_PAD, gx_ld), pc.CANARY, device=DEV)
        before = [t.clone() for t in ins]
        raw = raw0.clone()
        rc = lib.jn_pw_bwd_data_x3(ptr(x), g_ld, ptr(w), ptr(raw), gx_ld, M, c.cout, c.cin, S, c.max_wg, None)
        n_out = c.cin
    else:
        g_ld, x_ld = c.cout + pc.IN_PAD, c.cin + pc.IN_PAD
        gz = _rows(d["gz"], g_ld, pc.CANARY)      # g_z slots (M + 3) rows apart, x slots dense
        x = _rows(d["x"], x_ld, pc.CANARY, row_pad=0)
        tab = _dev(d["tab"])
        ins = [gz, x, tab]
        raw0 = _dev(d["prev"]).reshape(1, c.cout, c.cin)
        if c.use_wpart:
            wpart = torch.full((pc.NREP, pc.WPART_MAX), pc.CANARY, device=DEV)
        before = [t.clone() for t in ins]
        raw = raw0.clone()
        rc = lib.jn_pw_bwd_weight(ptr(gz), g_ld, ptr(x), x_ld, ptr(tab), ptr(raw), M, c.cout, c.cin, S, (M + pc.ROW_PAD) * g_ld, c.use_wpart,
                                  ptr(wpart) if c.use_wpart else None, c.exact, None)
        n_out = c.cin
    _lib.check(rc, f"{c}")
    torch.cuda.synchronize()
    if c.kind == "bdx3":
        res["out"] = raw[0, :S * M, :n_out].reshape(S, M, n_out).float().cpu()
    elif c.kind == "bw":
        res["out"] = raw[0].cpu()
    else:
        res["out"] = raw[:, :M, :n_out].float().cpu()
    res["stats"] = (f64 - f64_0).sum(0).reshape(c.cout, 2).t().cpu() if f64 is not None else None
    cpu = lambda t: None if t is None else t.cpu()
    return Run(res, raw.cpu(), raw0.cpu(), cpu(f64), cpu(f64_0), cpu(wpart), cpu(up), cpu(up0), all(torch.equal(a, b) for a, b in zip(ins, before)))


def _got(r):
    return r.res["out"], r.res["stats"]


def _same_launch_twice(c, a, b, ref):
    """Two runs of one launch: the bits wherever an element has one writer, else the order of the atomics."""
    if c.kind == "bw":
        d = (a.raw - b.raw).abs().max().item() / ref[0].abs().max().item()
        assert d <= pc.DW_ORDER, ("two runs differ in dW by more than the order of their atomics", c, d)
    else:
        assert _bits(a.raw, b.raw), ("two runs differ", c)
        assert a.up is None or _bits(a.up, b.up), ("two runs differ in the upsampled copy", c)
    if a.f64 is not None:
        d = ((a.f64 - a.f64_0) - (b.f64 - b.f64_0)).abs().max().item() / (a.f64 - a.f64_0).abs().max().item()
        assert d <= pc.STAT_ORDER, ("statistics of two runs differ", c, d)


def _check_untouched(c, r):
    assert r.inputs_intact, c
    if c.kind == "bw":
        return
    n_out, rows = (c.cin, c.slots * c.M) if c.kind == "bdx3" else (c.cout, c.M)
    assert _bits(r.raw[..., n_out:], r.raw0[..., n_out:]), ("canary in the channels past the count", c)
    assert _bits(r.raw[:, rows:], r.raw0[:, rows:]), ("canary in the rows past M", c)


def _check_upsample(c, r):
    n, h, w = pc.images(c)
    rows = n * 4 * h * w
    assert _bits(r.up[rows:], r.up0[rows:]) and _bits(r.up[:, c.cout:], r.up0[:, c.cout:]), ("canary around the upsampled copy", c)
    want = r.raw[0, :c.M, :c.cout].reshape(n, h, w, c.cout).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(rows, c.cout)
    assert _bits(r.up[:rows, :c.cout].contiguous(), want.contiguous()), ("the upsampled copy is not the output", c)


@pytest.mark.parametrize("name", list(pc.KERNELS))
def test_kernel_against_fp64_at_tile_and_channel_edges(name):
    worst = collections.defaultdict(float)
    cases = pc.KERNELS[name]
    for c in cases:
        r = _run(c, c.route)
        _check_untouched(c, r)
        if c.skip == 2:
            assert _bits(r.raw, r.raw0), ("a skipped launch wrote its output", c)
            assert r.f64 is None or torch.equal(r.f64, r.f64_0), ("a skipped launch wrote its statistics", c)
            assert r.up is None or _bits(r.up, r.up0), ("a skipped launch wrote the upsampled copy", c)
            continue
        if c.stats:
            assert torch.equal(r.f64[c.nrep:], r.f64_0[c.nrep:]), ("statistics in a replica past nrep", c)
        if c.use_wpart:
            assert bool((r.wpart == 0).all()), ("the weight-gradient scratch was not left zero", c)
        if c.up:
            _check_upsample(c, r)
        ref = pc.reference(c)
        l2, mx = pc.distances(r.res["out"], ref[0])
        worst["l2"], worst["max"] = max(worst["l2"], l2), max(worst["max"], mx)
        line = f"  {c}: rel L2 {l2:.2e} max {mx:.2e}"
        if ref[1] is not None:
            st = pc.stats_over_bar(r.res["stats"], ref[1], pc.pixels(c))
            worst["stats"] = max(worst["stats"], st)
            line += f" stats {st:.2e} of their bar"
        print(line)
        assert not pc.over_bars(c, _got(r), ref), (c, pc.over_bars(c, _got(r), ref))
        _same_launch_twice(c, r, _run(c, c.route), ref)
    print(f"{name}: {len(cases)} cases, worst relative L2 {worst['l2']:.2e}, worst max-norm {worst['max']:.2e}" +
          (f", worst statistics {worst['stats']:.2e} of their bar" if "stats" in worst else ""))


def test_route_0_launches_what_the_rule_names():
    lib = _lib.load_library()
    taken = collections.Counter()
    seen = set()
    for c in pc.ALL_CASES:
        key = c._replace(route=0) if c.kind == "pw" else None
        if key is None or c.skip == 2 or c.max_wg or key in seen:
            continue
        seen.add(key)
        with pc.launch_env(c):
            named = lib.jn_pw_route(*pc.route_args(c, 0), None)
        assert named >= 1, c
        taken[named] += 1
        a, b = _run(c, 0), _run(c, named)
        assert _bits(a.raw, b.raw) and (a.up is None or _bits(a.up, b.up)), ("route 0 differs from the route the rule names", c, named)
    print("route 0 took (route: launches)", dict(taken))
    # (with the planes present the rule never names XS, and no case has the 65536 pixels from which it names NARROW)
    assert set(taken) == {pc.X1, pc.X3, pc.WIDE, pc.MFMA}


def test_split_routes_stay_as_close_to_fp64_as_the_fp32_route():
    pairs = 0
    worst = 0.0
    seen = set()
    for c in pc.ALL_CASES:
        key = pc._key(c)._replace(stats=0, route=c.route)
        if not pc.is_split(c) or c.skip == 2 or key in seen:
            continue
        seen.add(key)
        ref = pc.reference(c)[0]
        split = pc.distances(_run(c, c.route).res["out"], ref)[1]
        twin = pc.f32_twin(c)
        f32 = pc.distances(_run(twin, twin.route).res["out"], pc.reference(twin)[0])[1]
        worst = max(worst, split / max(f32, 1e-12))
        assert split <= pc.SPLIT_VS_F32[0] * f32 + pc.SPLIT_VS_F32[1], (c, split, f32)
        pairs += 1
    print(f"split against fp32 route: {pairs} launches, worst ratio of the max-norm distances to fp64 {worst:.2f}")
    assert pairs >= 40


def test_entries_refuse_bad_arguments():
    """With real device tensors: a refused call leaves its outputs alone.  (The checks need no device; tests/test_pw_cases_cpu.py runs
    the full list.)"""
    lib = _lib.load_library()
    c = pc.KERNELS["pw_narrow_kernel<2, 32>"][0]
    d = pc.inputs(c)
    x, tab, w = _rows(d["x"], c.cin + 8, pc.CANARY), _dev(d["tab"]), _dev(d["w"])
    out = torch.full((1, c.M + 3, c.cout + 4), pc.CANARY, device=DEV)
    stats = torch.zeros(pc.NREP, 2 * c.cout, dtype=torch.float64, device=DEV)
    args = lambda **o: [ptr(x), o.get("in_ld", c.cin + 8), o.get("dtype_in", 0), ptr(tab), None, ptr(w), None, ptr(out), o.get("out_ld", c.cout + 4), 0,
                        o.get("N", 1), 1, c.M, o.get("cin", c.cin), c.cout, 0, o.get("transposed", 0), 0, o.get("accumulate", 0), o.get("act", 0), ptr(stats),
                        o.get("nrep", 32), None, 0, o.get("slots", 1), 0, 0, 0, None, 0, o.get("route", pc.NARROW), o.get("max_wg", 0), None]
    for bad in (dict(N=0), dict(cin=30), dict(in_ld=c.cin + 2), dict(out_ld=c.cout + 2), dict(dtype_in=2), dict(act=4), dict(nrep=0), dict(nrep=33), dict(route=7),
                dict(route=-1), dict(max_wg=-1), dict(route=pc.MFMA, max_wg=1), dict(slots=3), dict(accumulate=1), dict(transposed=1), dict(route=pc.XS),
                dict(route=pc.WIDE), dict(route=pc.X1)):
        assert lib.jn_pw(*args(**bad)) == -1, bad
    a = args()
    a[0] = None
    assert lib.jn_pw(*a) == -1
    cb = pc.KERNELS["pw_bwd_weight_kernel<2, 3>"][0]
    db = pc.inputs(cb)
    gz, xb, tb = _rows(db["gz"], cb.cout + 8, pc.CANARY), _rows(db["x"], cb.cin + 8, pc.CANARY, row_pad=0), _dev(db["tab"])
    gw = torch.full((cb.cout, cb.cin), pc.CANARY, device=DEV)
    bargs = lambda **o: [ptr(gz), o.get("g_ld", cb.cout + 8), ptr(xb), cb.cin + 8, ptr(tb), ptr(gw), cb.M, cb.cout, cb.cin, o.get("slots", 1),
                         o.get("gz_ss", (cb.M + 3) * (cb.cout + 8)), o.get("use_wpart", 0), None, o.get("exact", 0), None]
    for bad in (dict(g_ld=cb.cout + 2), dict(slots=0), dict(gz_ss=8), dict(use_wpart=1), dict(exact=1), dict(exact=2)):
        assert lib.jn_pw_bwd_weight(*bargs(**bad)) == -1, bad
    cd = pc.KERNELS["w_split3_t_kernel, pw_x3_kernel<256, 2, 2, 2, 3, float, false, true>"][0]
    dd = pc.inputs(cd)
    g3, w3 = _rows(dd["x"], cd.cout + 8, pc.CANARY), _dev(dd["w"])
    gx = torch.full((cd.M + 3, cd.cin + 4), pc.CANARY, device=DEV)
    dargs = lambda **o: [ptr(g3), o.get("g_ld", cd.cout + 8), ptr(w3), ptr(gx), cd.cin + 4, cd.M, o.get("cout", cd.cout), cd.cin, o.get("slots", 1),
                         o.get("max_wg", 0), None]
    for bad in (dict(g_ld=cd.cout + 2), dict(cout=128), dict(slots=0), dict(max_wg=-1)):
        assert lib.jn_pw_bwd_data_x3(*dargs(**bad)) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == pc.CANARY).all()) and bool((stats == 0).all()) and bool((gw == pc.CANARY).all()) and bool((gx == pc.CANARY).all())
