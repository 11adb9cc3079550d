"""Cases, inputs, fp64 reference and bars for the depthwise 3x3 kernels (csrc/kernels_conv.hip: dw3x3_lds_kernel, dw3x3_kernel,
dwpw_eval_kernel; csrc/kernels_bwd.hip: dw_bwd_fused_kernel and the unfused bn_bwd_gz / dw_bwd_data / dw_bwd_weight route), one
kernel at a time through the context-free entries jn_dw3x3 / jn_dwpw / jn_dw_bwd.

Shared by tests/test_dw_cases_cpu.py (the bars mean something on these inputs and bite on the mistakes a kernel can make) and
tests/test_gpu_dw_kernels.py (every kernel against the reference).  Fixed seeds, no committed tensors.

A case is (kind, route, stride, H, W, C, cout, dtype, slots, accumulate, stats, skip, nrep, use_wpart, max_wg, red, res):
 - kind "fwd": jn_dw3x3; "dwpw": jn_dwpw (cout = the 1x1 conv's output channels, res = with the shortcut); "bwd": jn_dw_bwd
   (red = with the input layer's BatchNorm sums);
 - route: the forced route of the entry (include/jnroll.h); dtype 0 = fp32 maps, 1 = bf16 maps;
 - H x W: the layer's INPUT map; the output map is (H + stride - 1) / stride x (W + stride - 1) / stride;
 - skip: 0 = no flag, 1 = a flag below skip_when (the launch runs), 2 = a flag at skip_when (nothing may change).

Shapes: the smallest with an edge of the TH x 16 output tile (TH = 8 at stride 1, 4 at stride 2).  Stride 1: 5x5 (one partial
tile), 17x18 (a third row tile, a second column tile, one row and two columns into them), 9x33 (a second row tile, a third column
tile).  Stride 2: 10x10 (one partial tile), 34x36 (to 17x18: a fifth row tile, a second column tile, the +1 halo row and column),
9x11 (to 5x6) and 33x35 (to 17x18): odd inputs, whose last 2 x 2 input block is half outside the map.  Channels 16 (one block
of 16), 32 (one of 32), 48 (three of 16; C / 4 = 12 is no power of two), 64 (two of 32).  Every kernel meets every spatial shape
of its stride at C = 32 (16 where it has no 32 form), every channel count it admits on the two-tile shape, and each of its
options once on the two-tile shape."""
import collections
import functools

import torch
import torch.nn.functional as F

from tests.conv3_cases import (BF16_ABS, BF16_L2, BF16_MAX, CANARY, CANARY_BF16, DW_MAX, DW_ORDER, NREP, OUT_L2, OUT_MAX,      # noqa: F401
                               SKIP_WHEN, STAT_ATOL, STAT_RTOL, distances, padded, stats_over_bar, transform)
from tests.kernel_helpers import _bf16, _dsilu, _nchw, _nhwc

Case = collections.namedtuple("Case", "kind route stride H W C cout dtype slots accumulate stats skip nrep use_wpart max_wg red res")

N = 2                       # images: the image stride is exercised
IN_PAD, OUT_PAD = 8, 4      # read-side leading dimensions C + 8, written-side C + 4
WPART_MAX = 16384           # JN_WPART_MAX: floats per replica of the weight-gradient scratch
TH = {1: 8, 2: 4}           # output rows of a tile; 16 output columns

# ---- the bars: those of conv3_cases.py (imported above), and one of this unit ------------------------------------------------
# The input layer's BatchNorm sums the fused backward forms (RED): per channel, |delta| over the channel's sum of |terms|.  Plain
# fp32 arithmetic, summing in pixel order, measured against fp64 on the cases of this file (test_dw_cases_cpu.py prints it):
RED_FP32_MEASURED = 5.8e-7   # (the 34 x 36 stride-2 cases; 2448 pixels per sum)
RED_BAR = 3e-6               # 4 x the above, rounded up to one digit: the margin the dense 3x3 pin gives fp32 arithmetic

SPATIAL = {1: ((5, 5), (17, 18), (9, 33)), 2: ((10, 10), (34, 36), (9, 11), (33, 35))}
TWO_TILES = {1: (17, 18), 2: (34, 36)}
CHANNELS = (16, 32, 48, 64)


def _case(kind, route, stride, hw, C, cout=0, dtype=0, slots=1, accumulate=0, stats=0, skip=0, nrep=NREP, use_wpart=0, max_wg=0, red=0,
          res=0):
    return Case(kind, route, stride, hw[0], hw[1], C, cout, dtype, slots, accumulate, stats, skip, nrep, use_wpart, max_wg, red, res)


def _cases(kind, route, stride, base_c, channels, options, **fixed):
    """Spatial edges at base_c, the other channel counts on the two-tile shape, then one case per option on the two-tile shape."""
    two = TWO_TILES[stride]
    cases = [_case(kind, route, stride, hw, base_c, **fixed) for hw in SPATIAL[stride]]
    # (forward: with statistics, the channel blocks' offsets into the sums; 8 replicas, which the workgroups of these counts outnumber)
    edge = dict(stats=1, nrep=8) if kind == "fwd" else {}
    cases += [_case(kind, route, stride, two, C, **dict(fixed, **edge)) for C in channels if C != base_c]
    cases += [_case(kind, route, stride, two, base_c, **dict(fixed, **o)) for o in options]
    return cases


_FWD_OPTS = (dict(stats=1), dict(stats=1, nrep=8), dict(stats=1, skip=1), dict(stats=1, skip=2))
_DWPW_OPTS = (dict(res=1), dict(skip=1), dict(res=1, skip=2))
_BWD_OPTS = (dict(accumulate=1), dict(slots=3), dict(slots=3, accumulate=1), dict(use_wpart=1), dict(max_wg=1), dict(max_wg=2),
             dict(slots=3, max_wg=2, use_wpart=1))
_RED_OPTS = (dict(slots=3), dict(use_wpart=1), dict(max_wg=1), dict(max_wg=2), dict(slots=3, max_wg=2, use_wpart=1))

# kernel name -> its cases.  The names are those of kernels_conv.hip and kernels_bwd.hip.
KERNELS = collections.OrderedDict()
for _t, _dt in (("float", 0), ("bf16_t", 1)):
    for _s, _cb, _chan in ((1, 32, (32, 64)), (1, 16, (16, 48)), (2, 32, (32, 64)), (2, 16, (16, 48))):
        if _dt and _s == 2:
            if _cb == 32:
                continue      # bf16 maps at stride 2: blocks of 16 whatever the channel count
            _chan = CHANNELS
        KERNELS[f"dw3x3_lds_kernel<{_s}, {_cb}, {TH[_s]}, {_t}>"] = _cases("fwd", 1, _s, 32 if 32 in _chan else 16, _chan, _FWD_OPTS, dtype=_dt)
    for _s in (1, 2):
        KERNELS[f"dw3x3_kernel<{_s}, {_t}>"] = _cases("fwd", 2, _s, 32, CHANNELS, _FWD_OPTS, dtype=_dt)
    for _s, _wm, _cts in ((1, 4, (1, 2, 4, 8)), (2, 2, (2, 4, 8))):
        for _ct in _cts:      # C = 16, 32, 64: one, two and four chunks of 16 channels
            KERNELS[f"dwpw_eval_kernel<{_s}, {_wm}, {_ct}, {_t}>"] = _cases("dwpw", 0, _s, 32, (16, 64), _DWPW_OPTS, cout=16 * _ct, dtype=_dt)
for _s, _cb, _chan in ((1, 32, (32, 64)), (1, 16, (16, 48)), (2, 16, CHANNELS)):
    _base = 32 if 32 in _chan else 16
    KERNELS[f"dw_bwd_fused_kernel<{_s}, {_cb}, {TH[_s]}, false>"] = _cases("bwd", 1, _s, _base, _chan, _BWD_OPTS)
    KERNELS[f"dw_bwd_fused_kernel<{_s}, {_cb}, {TH[_s]}, true>"] = _cases("bwd", 1, _s, _base, _chan, _RED_OPTS, red=1)
for _s in (1, 2):
    KERNELS[f"bn_bwd_gz_kernel, dw_bwd_data_kernel<{_s}>, dw_bwd_weight_kernel<{_s}>"] = _cases("bwd", 2, _s, 32, CHANNELS, _BWD_OPTS)

ALL_CASES = [c for cases in KERNELS.values() for c in cases]


def out_hw(c):
    return (c.H + c.stride - 1) // c.stride, (c.W + c.stride - 1) // c.stride


def n_tiles(c):
    """Output tiles of one channel block and slot."""
    OH, OW = out_hw(c)
    return N * -(-OH // TH[c.stride]) * -(-OW // 16)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _table(g, S, C, raw=True):
    """[S, 3, C]: scales in [0.5, 1.5]; shifts 0.5 randn: silu(shift) is far from 0; about a quarter of the channels is read raw
    (channel 1 always, so that every table has one)."""
    t = torch.empty(S, 3, C)
    t[:, 0] = 0.5 + torch.rand(S, C, generator=g)
    t[:, 1] = 0.5 * torch.randn(S, C, generator=g)
    t[:, 2] = (torch.rand(S, C, generator=g) < 0.75).float()
    t[:, 2, 1] = 0.0
    if not raw:
        t[:, 2] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def _inputs(kind, stride, H, W, C, cout, dtype, slots, red):
    c = _case(kind, 0, stride, (H, W), C, cout=cout)
    seed = ((((("fwd", "dwpw", "bwd").index(kind) * 3 + stride) * 64 + H) * 64 + W) * 128 + C) * 4096 + cout * 16 + dtype * 8 + slots * 2 + red
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    OH, OW = out_hw(c)
    # bf16 maps: rounding the OUTPUT alone costs up to 3.9e-3 of max|ref|, which leaves the max-norm bar 5e-3 max|ref| + 1e-4 no 2x
    # margin on outputs of order 1 (conv3_cases.py); the bf16 cases therefore have outputs of about 0.01, where the bar's
    # absolute part is worth another 5e-3 of max|ref|: small weights, and a shortcut whose two summands are small
    small = 1.0 / 512 if dtype else 1.0
    if kind == "fwd":
        return dict(x=r(N, H, W, C), tab=_table(g, 1, C)[0], w=r(9, C) / 3 * small)
    if kind == "dwpw":
        mtab, rtab, ptab = _table(g, 1, C, raw=False)[0], _table(g, 1, cout)[0], _table(g, 1, cout, raw=False)[0]
        rtab[1] *= small
        ptab[1] *= small
        return dict(x=r(N, H, W, C), tab=_table(g, 1, C)[0], w=r(9, C) / 3, mtab=mtab, w_pw=r(cout, C) / C ** 0.5 * small,
                    res=r(N, OH, OW, cout) * small, rtab=rtab, ptab=ptab)
    # the backward: tables, save and consts drawn as in tests/test_gpu_pw_bwd_fused128.py::_inputs, different per slot.  With RED
    # the input is a BatchNorm output: every channel is transformed
    S = slots
    return dict(g=r(S, N, OH, OW, C), z=r(S, N, OH, OW, C), x=r(S, N, H, W, C), otab=_table(g, S, C), itab=_table(g, S, C, raw=not red),
                save=torch.stack([0.3 * r(S, C), u(0.5, 2.0, S, C)], -1),      # (mean, invstd)
                consts=torch.stack([0.1 * r(S, C), 0.1 * r(S, C), u(0.5, 1.5, S, C)], -1),      # (c1, c2, k)
                w=r(9, C) / 3, gin0=r(S, N, H, W, C), gw0=0.1 * r(9, C))


def inputs(c):
    """The case's dense fp32 tensors (channels last); shared by all routes and options of a shape.  Do not modify."""
    return _inputs(c.kind, c.stride, c.H, c.W, c.C, c.cout, c.dtype, c.slots, c.red)


# ---- the reference: a plain restatement, fp64 by default ---------------------------------------------------------------
def _w4(w):
    """[9][C], tap = 3 ky + kx -> [C][1][3][3]."""
    return w.t().reshape(w.shape[1], 1, 3, 3)


def _halo(c):
    """(first output row of the second row tile, the input row its last tap above reads; likewise for columns)."""
    t = TH[c.stride]
    return t, (t - 1) * c.stride + 1, 16, 15 * c.stride + 1


def dwconv(c, x, tab, w, mutant=None):
    """Depthwise conv of the activated input: x [N, H, W, C] raw, tab [3, C], w [9, C] -> [N, C, OH, OW].  Mutants: "pad_silu"
    (the padding went through the transform too), "raw_transformed" (a channel with flag 0 transformed), "halo_row" / "halo_col"
    (the last output row / column of the first tile misses the input row / column past the tile), "drop_last_row" /
    "drop_last_col" (the last row / column of an odd stride-2 input never read)."""
    if mutant == "raw_transformed":
        tab = torch.stack([tab[0], tab[1], torch.ones_like(tab[2])])
    if mutant == "pad_silu":
        a, pad = _nchw(transform(F.pad(x, (0, 0, 1, 1, 1, 1)), tab)), 0
    else:
        a, pad = _nchw(transform(x, tab)), 1
    if mutant == "drop_last_row":
        a = a.clone()
        a[:, :, -1, :] = 0
    if mutant == "drop_last_col":
        a = a.clone()
        a[:, :, :, -1] = 0
    out = F.conv2d(a, _w4(w), stride=c.stride, padding=pad, groups=c.C)
    if mutant in ("halo_row", "halo_col"):
        o_r, i_r, o_c, i_c = _halo(c)
        a2 = a.clone()
        out = out.clone()
        if mutant == "halo_row":
            a2[:, :, i_r, :] = 0
            out[:, :, o_r - 1, :] = F.conv2d(a2, _w4(w), stride=c.stride, padding=pad, groups=c.C)[:, :, o_r - 1, :]
        else:
            a2[:, :, :, i_c] = 0
            out[:, :, :, o_c - 1] = F.conv2d(a2, _w4(w), stride=c.stride, padding=pad, groups=c.C)[:, :, :, o_c - 1]
    return out


def _dw_transposed(c, gz, w, mutant=None):
    """Data gradient [N, C, H, W] of g_z [N, C, OH, OW]: g_in[iy][ix] = sum g_z[(iy + 1 - ky) / S][(ix + 1 - kx) / S] w[ky][kx] where
    divisible.  Mutants: "unmirrored" (the forward conv's taps), "parity" (stride 2: the parity classes of the input pixels
    swapped), "gz_halo_row" / "gz_halo_col" (the input rows / columns of the first tile miss g_z of the tile past it)."""
    OH, OW = out_hw(c)
    w4 = _w4(w)
    if mutant == "unmirrored":
        w4 = w4.flip(2, 3)
    full = F.conv_transpose2d(gz, w4, stride=c.stride, groups=c.C)      # no padding: [(OH - 1) S + 3] rows, input row iy at iy + 1
    o = 0 if mutant == "parity" else 1
    full = F.pad(full, (0, 2, 0, 2))
    gin = full[:, :, o:o + c.H, o:o + c.W]
    if mutant in ("gz_halo_row", "gz_halo_col"):
        o_r, _, o_c, _ = _halo(c)
        g2 = gz.clone()
        gin = gin.clone()
        if mutant == "gz_halo_row":
            g2[:, :, o_r, :] = 0
            gin[:, :, :o_r * c.stride, :] = _dw_transposed(c, g2, w)[:, :, :o_r * c.stride, :]
        else:
            g2[:, :, :, o_c] = 0
            gin[:, :, :, :o_c * c.stride] = _dw_transposed(c, g2, w)[:, :, :, :o_c * c.stride]
    return gin


def _pixel_order_sum(t):
    """[N, H, W, C] -> [C], one pixel after the other (what an fp32 accumulator does; torch.sum adds pairwise)."""
    acc = torch.zeros(t.shape[-1], dtype=t.dtype)
    for row in t.reshape(-1, t.shape[-1]):
        acc = acc + row
    return acc


def compute(c, dtype=torch.float64, mutant=None, tensors=None):
    """The case's results in `dtype` arithmetic (from `tensors` in place of the case's own inputs, if given), a dict of
      "out":   fwd / dwpw: the output [N, OH, OW, C']; bwd: the input gradient [S, N, H, W, C];
      "stats": fwd with stats: (sum, sum of squares) of the output per channel, [2, C];
      "dw":    bwd: the weight gradient [9, C], added to gw0 over all slots;
      "red":   bwd with red: per slot and input channel (sum dx silu'(y_in), sum dx silu'(y_in) y_in), [S, 2, C], and "red_abs", the
               sums of the absolute terms (the scale of the RED bar)."""
    d = {k: v.to(dtype) for k, v in (tensors or inputs(c)).items()}
    if c.kind == "fwd":
        out = _nhwc(dwconv(c, d["x"], d["tab"], d["w"], mutant))
        res = dict(out=out)
        if c.stats:
            res["stats"] = torch.stack([out.sum((0, 1, 2)), (out * out).sum((0, 1, 2))])
        return res
    if c.kind == "dwpw":
        dd = _nhwc(dwconv(c, d["x"], d["tab"], d["w"], mutant))
        y = dd * d["mtab"][0] + d["mtab"][1]
        out = (y * torch.sigmoid(y)) @ d["w_pw"].t()
        if c.res:
            v = out * d["ptab"][0] + d["ptab"][1]
            out = v * torch.sigmoid(v) + transform(d["res"], d["rtab"])
        return dict(out=out)
    gins, reds, red_abs = [], [], []
    dw = torch.zeros(9, c.C, dtype=dtype) if mutant == "no_accumulate" else d["gw0"].clone()
    for s in range(c.slots):
        t = 0 if mutant == "slot_table" and s == 2 else s
        otab, itab, save, consts = d["otab"][t], d["itab"][t], d["save"][t], d["consts"][t]
        if mutant == "raw_transformed":
            itab = torch.stack([itab[0], itab[1], torch.ones_like(itab[2])])
        y = d["z"][s] * otab[0] + otab[1]
        zhat = (d["z"][s] - save[:, 0]) * save[:, 1]
        gz = consts[:, 2] * (d["g"][s] * _dsilu(y) - consts[:, 0] - (0 if mutant == "no_c2" else zhat * consts[:, 1]))
        gz = _nchw(gz)
        dx = _dw_transposed(c, gz, d["w"], mutant)
        if mutant == "pad_silu":
            a, pad = _nchw(transform(F.pad(d["x"][s], (0, 0, 1, 1, 1, 1)), itab)), 0
        else:
            a, pad = _nchw(transform(d["x"][s], itab)), 1
        if mutant == "drop_last_row":
            a, dx = a.clone(), dx.clone()
            a[:, :, -1, :] = 0
            dx[:, :, -1, :] = 0
        if mutant == "drop_last_col":
            a, dx = a.clone(), dx.clone()
            a[:, :, :, -1] = 0
            dx[:, :, :, -1] = 0
        gw = torch.nn.grad.conv2d_weight(a, (c.C, 1, 3, 3), gz.contiguous(), stride=c.stride, padding=pad, groups=c.C)
        dw = dw + gw.reshape(c.C, 9).t()
        dx = _nhwc(dx)
        if c.red:
            y_in = d["x"][s] * itab[0] + itab[1]
            t1 = dx * _dsilu(y_in)
            t2 = t1 * y_in
            if mutant == "red_missing_pixel":
                t1, t2 = t1.clone(), t2.clone()
                t1[-1, -1, -1] = 0
                t2[-1, -1, -1] = 0
            add = _pixel_order_sum if dtype == torch.float32 else (lambda t: t.sum((0, 1, 2)))
            reds.append(torch.stack([add(t1), add(t2)]))
            red_abs.append(torch.stack([t1.abs().sum((0, 1, 2)), t2.abs().sum((0, 1, 2))]))
        gins.append(dx + d["gin0"][s] if c.accumulate and mutant != "no_accumulate" else dx)
    res = dict(out=torch.stack(gins), dw=dw)
    if c.red:
        res["red"], res["red_abs"] = torch.stack(reds), torch.stack(red_abs)
    return res


def _key(c):
    """The case without what does not change its results."""
    return c._replace(route=0, skip=0, nrep=NREP, use_wpart=0, max_wg=0)


@functools.lru_cache(maxsize=None)
def _reference(key):
    return compute(key)


def reference(c):
    """fp64, computed once per distinct computation; shared by the routes and options.  Do not modify."""
    return _reference(_key(c))


def compute_bf16(c):
    """bf16 storage: the maps (input, shortcut, output) hold bf16, everything between them is fp32.  The statistics are those
    of the fp32 accumulators."""
    d = inputs(c)
    rounded = dict(d, x=_bf16(d["x"]))
    if c.kind == "dwpw":
        rounded["res"] = _bf16(d["res"])
    res = compute(c, torch.float32, tensors=rounded)
    res["out"] = _bf16(res["out"])
    return res


# ---- distances -----------------------------------------------------------------------------------------------------------
def red_distance(got, ref):
    """Worst |delta| per slot, moment and channel over that channel's sum of |terms|."""
    return ((got.double() - ref["red"]).abs() / ref["red_abs"]).max().item()


def over_bars(c, got, ref, margin=1.0):
    """[] when every result of `got` is within the case's bars divided by `margin`, else the offending (name, distance, bar)
    triples.  `got` and `ref` are dicts as compute returns them."""
    bad = []
    l2, mx = distances(got["out"], ref["out"])
    bl2, bmx, babs = (BF16_L2, BF16_MAX, BF16_ABS) if c.dtype else (OUT_L2, OUT_MAX, 0.0)
    scale = ref["out"].abs().max().item()
    if not l2 * margin <= bl2:
        bad.append(("relative L2", l2, bl2))
    if not mx * margin <= bmx + babs / scale:
        bad.append(("max-norm / max|ref|", mx, bmx + babs / scale))
    if "stats" in ref:
        OH, OW = out_hw(c)
        st = stats_over_bar(got["stats"], ref["stats"], N * OH * OW)
        if not st * margin <= 1.0:
            bad.append(("statistics / their bar", st, 1.0))
    if "dw" in ref:
        dmx = distances(got["dw"], ref["dw"])[1]
        if not dmx * margin <= DW_MAX:
            bad.append(("dW max-norm / max|ref|", dmx, DW_MAX))
    if "red" in ref:
        rd = red_distance(got["red"], ref)
        if not rd * margin <= RED_BAR:
            bad.append(("RED sums / sum |terms|", rd, RED_BAR))
    return bad
