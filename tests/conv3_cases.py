"""Cases, inputs, fp64 reference and bars for the dense 3x3 kernels (csrc/kernels_conv3.hip), one kernel at a time through
the context-free entries jn_conv3 / jn_conv3_bwd_data_s2 / jn_conv3_bwd_weight.

Shared by tests/test_conv3_cases_cpu.py (the bars mean something on these inputs and bite on the mistakes a kernel can make)
and tests/test_gpu_conv3_kernels.py (every kernel against the reference).  Fixed seeds, no committed tensors.

A case is (kind, route, stride, H, W, cin, cout, slots, accumulate, stats, skip, max_wg):
 - kind "fwd": forward; "wt": data gradient of a stride-1 layer (jn_conv3, transposed); "ds2": data gradient of a stride-2
   layer; "dw": weight gradient; "bf16": forward of the bf16 inference kernel (route 3 of jn_conv3);
 - route: the forced route of the entry (include/jnroll.h);
 - H x W: the layer's INPUT map (stride 2: the output map is H / 2 x W / 2);
 - cin, cout: the FORWARD layer's channels for "fwd", "bf16", "ds2" and "dw".  For "wt" they are the entry's: cin = the
   forward layer's output channels (those of g_z), cout = its input channels.  A channel pair (a, b) of the list below is
   (cin, cout) for "fwd" / "bf16" / "dw" and (Co, Ci) — the contracted, then the produced channels — for both data gradients;
 - skip: 0 = no flag, 1 = a flag below skip_when (the launch runs), 2 = a flag at skip_when (nothing may change).

Shapes: the smallest at which a tile or channel-block edge exists.  Spatial 5x5 (one partial tile), 17x18 (one row and two
columns into a second 16 x 16 tile, a third 8-row and a fifth 4-row tile), 9x33 (fp32 routes: a second 8-row tile, a third
16-column tile); stride 2 from 10x10, 34x36 (17x18 class grids, the +1 g_z halo row and column at the border) and 10x12.
Channels (32, 32) one split K chunk and half a block of 64; (64, 96) two chunks, a block and a half; (128, 64) eight fp32 /
four split chunks; (20, 36) the partial fp32 K chunk of 16 (fp32 routes and the weight-gradient kernel without transposed
reads).  Every kernel meets every spatial edge at (32, 32), every channel pair it admits on the two-tile shape, and each of
its options once on the two-tile shape at (32, 32)."""
import collections
import functools

import torch
import torch.nn.functional as F

from tests.fp64_bars import STAT_ATOL, STAT_RTOL      # noqa: F401  (re-exported: the stats bar of the GPU test)
from tests.kernel_helpers import _bf16, _nchw, _nhwc

Case = collections.namedtuple("Case", "kind route stride H W cin cout slots accumulate stats skip max_wg")

N = 2                       # images: the image stride is exercised
IN_PAD, OUT_PAD = 8, 4      # in_ld = cin + 8, out_ld = cout + 4 (g_ld / gin_ld / x_ld likewise: read side + 8, written side + 4)
CANARY = 77777.0            # what the channels past the count hold (bf16-exact: 77777 is not, so the bf16 buffers take CANARY_BF16)
CANARY_BF16 = 77824.0
SKIP_WHEN = 2
NREP = 32                   # JN_NREP: statistics replicas

# ---- the bars: all from the project's existing tests, none from the kernels -------------------------------------------
OUT_L2 = 2e-5               # outputs and data gradients: relative L2 (test_wide_data_gradient_on_the_bf16_pipe_matches_the_fp32_pipe)
OUT_MAX = 1e-4              # ... and max |delta| / max |ref|
DW_MAX = 1e-4               # weight gradients: max |delta| / max |ref| (test_split_weight_gradients_stay_close_to_fp32_mfma)
DW_EXACT_L2 = 2e-5          # the exact-products route additionally: relative L2
DW_ORDER = 1e-5             # two runs of a weight gradient with several writers per element: max |delta| / max |dW|
BF16_L2 = 1e-2              # bf16 inference kernel: relative L2 (test_gpu_encoder_fp64.py)
BF16_MAX, BF16_ABS = 5e-3, 1e-4      # ... and max |delta| <= BF16_MAX max|ref| + BF16_ABS
SPLIT_VS_F32 = (1.5, 1e-6)  # route 2 is no further from fp64 than 1.5 x route 1 + 1e-6, max-norm

SPATIAL_S1 = ((5, 5), (17, 18))
SPATIAL_S1_F32 = ((9, 33),)
SPATIAL_S2 = ((10, 10), (34, 36), (10, 12))
TWO_TILES = {1: (17, 18), 2: (34, 36)}
PAIRS = ((64, 96), (128, 64))      # beside (32, 32), which the spatial cases carry
PAIR_F32 = (20, 36)


def _case(kind, route, stride, hw, pair, slots=1, accumulate=0, stats=0, skip=0, max_wg=0):
    return Case(kind, route, stride, hw[0], hw[1], pair[0], pair[1], slots, accumulate, stats, skip, max_wg)


def _conv_cases(kind, route, stride, options):
    """Spatial edges at (32, 32), channel edges on the two-tile shape, then one case per option on the two-tile shape."""
    f32 = route == 1
    spatial = (SPATIAL_S1 + (SPATIAL_S1_F32 if f32 else ())) if stride == 1 else SPATIAL_S2
    two = TWO_TILES[stride]
    cases = [_case(kind, route, stride, hw, (32, 32)) for hw in spatial]
    if kind == "ds2":      # pairs are (Co, Ci): the case holds the forward layer's (cin, cout)
        cases = [c._replace(cin=c.cout, cout=c.cin) for c in cases]
    for pair in PAIRS + ((PAIR_F32,) if f32 else ()):
        cases.append(_case(kind, route, stride, two, pair[::-1] if kind == "ds2" else pair))
    for opt in options:
        cases.append(_case(kind, route, stride, two, (32, 32), **opt))
    return cases


_FWD_OPTS = (dict(accumulate=1), dict(stats=1), dict(stats=1, skip=1), dict(stats=1, skip=2))
_GRAD_OPTS = (dict(accumulate=1), dict(slots=3), dict(slots=3, accumulate=1))

# kernel name -> its cases.  The names are those of kernels_conv3.hip.
KERNELS = collections.OrderedDict([
    ("conv3_mfma_kernel<1, float, false>", _conv_cases("fwd", 1, 1, _FWD_OPTS)),
    ("conv3_x3_kernel<1, false>", _conv_cases("fwd", 2, 1, _FWD_OPTS)),
    ("conv3_mfma_kernel<2, float, false>", _conv_cases("fwd", 1, 2, _FWD_OPTS)),
    ("conv3_x3s2_kernel", _conv_cases("fwd", 2, 2, _FWD_OPTS[1:])),                      # admits no accumulate
    ("conv3_mfma_kernel<1, float, true>", _conv_cases("wt", 1, 1, _GRAD_OPTS + _FWD_OPTS[1:])),
    ("conv3_x3_kernel<1, true>", _conv_cases("wt", 2, 1, _GRAD_OPTS + _FWD_OPTS[1:])),
    ("conv3_bwd_data_s2_kernel", _conv_cases("ds2", 1, 2, _GRAD_OPTS)),
    ("conv3_x3_bwd_data_s2_kernel", _conv_cases("ds2", 2, 2, _GRAD_OPTS)),
])

_DW_OPTS = (dict(max_wg=1), dict(max_wg=2), dict(slots=3), dict(slots=3, max_wg=1), dict(slots=3, max_wg=2))
for _s in (1, 2):
    _two = TWO_TILES[_s]
    _spatial = SPATIAL_S1 if _s == 1 else SPATIAL_S2
    for _route, _name in ((1, f"conv3_bwd_weight_tr_kernel<{_s}>"), (2, f"conv3_bwd_weight_kernel<{_s}, 4, true>"),
                          (3, f"conv3_bwd_weight_kernel<{_s}, 4, false>")):
        _c = [_case("dw", _route, _s, hw, (32, 32)) for hw in _spatial + (SPATIAL_S1_F32 if _s == 1 and _route == 3 else ())]
        _c += [_case("dw", _route, _s, _two, p) for p in PAIRS + ((PAIR_F32,) if _route != 1 else ())]
        _c += [_case("dw", _route, _s, _two, (32, 32), **o) for o in _DW_OPTS]
        KERNELS[_name] = _c
for _s in (1, 2):      # bf16 inference kernel: 5x5 and 17x18 outputs, both strides, two channel pairs; its one option on the two-tile shape
    KERNELS[f"conv3_bf16_kernel<{_s}>"] = (
        [_case("bf16", 3, _s, (5 * _s, 5 * _s), p) for p in ((32, 32), (64, 96))] +
        [_case("bf16", 3, _s, TWO_TILES[_s], p) for p in ((32, 32), (64, 96))] +
        [_case("bf16", 3, _s, TWO_TILES[_s], (32, 32), skip=k) for k in (1, 2)])

ALL_CASES = [c for cases in KERNELS.values() for c in cases]


def out_hw(c):
    return c.H // c.stride, c.W // c.stride


def entry_kind(c):
    """`kind` of jn_conv3_route."""
    return {"fwd": 0, "bf16": 0, "wt": 1, "ds2": 2, "dw": 3}[c.kind]


def lds(c):
    """(first, second) leading dimension in the order of the entry's arguments, and the channels they carry."""
    if c.kind in ("fwd", "bf16", "wt"):
        return (c.cin + IN_PAD, c.cin), (c.cout + OUT_PAD, c.cout)      # (in, out)
    if c.kind == "ds2":
        return (c.cout + IN_PAD, c.cout), (c.cin + OUT_PAD, c.cin)      # (g_z, g_in)
    return (c.cout + IN_PAD, c.cout), (c.cin + IN_PAD, c.cin)           # (g_z, x): both read


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _seed(c):
    return (((("fwd", "bf16", "wt", "ds2", "dw").index(c.kind if c.kind != "bf16" else "fwd") * 3 + c.stride) * 64 + c.H) * 64 + c.W) * 4096 \
        + c.cin * 7 + c.cout * 3 + c.slots


@functools.lru_cache(maxsize=None)
def _inputs(kind, stride, H, W, cin, cout, slots):
    c = Case(kind, 0, stride, H, W, cin, cout, slots, 0, 0, 0, 0)
    g = torch.Generator().manual_seed(_seed(c))
    r = lambda *s: torch.randn(*s, generator=g)
    OH, OW = out_hw(c)

    def table(S, C):      # scales in [0.5, 1.5]; shifts 0.5 randn: silu(shift) is far from 0; a quarter of the channels is read raw
        t = torch.empty(S, 3, C)
        t[:, 0] = 0.5 + torch.rand(S, C, generator=g)
        t[:, 1] = 0.5 * r(S, C)
        t[:, 2] = (torch.rand(S, C, generator=g) < 0.75).float()
        return t
    if kind in ("fwd", "bf16"):
        d = dict(x=r(slots, N, H, W, cin), tab=table(1, cin), w=r(9, cout, cin) / (9 * cin) ** 0.5, prev=r(slots, N, OH, OW, cout))
        if kind == "bf16":
            # Rounding the OUTPUT to bf16 alone costs up to half an ulp of the top binade, 1.95e-3 .. 3.9e-3 of max|ref| depending
            # on where max|ref| sits in it, so on outputs of order 1 the max-norm bar 5e-3 max|ref| + 1e-4 leaves a correct kernel
            # no 2x margin on ANY input.  The cases are therefore small maps (max|ref| about 0.02, where the bar's absolute part
            # is worth another 5e-3 of max|ref|), with weights of one sign: the outputs get a common part that grows with K where
            # the operands' rounding errors grow with sqrt(K), as in a trained layer.  The relative-L2 bar is scale-free.
            d["w"] = d["w"].abs() / 256
    elif kind == "wt":      # x = g_z over cin = Co channels; w is the forward weight [9][Co][Ci] = [9][cin][cout]
        d = dict(x=r(slots, N, H, W, cin), tab=table(1, cin), w=r(9, cin, cout) / (9 * cin) ** 0.5, prev=r(slots, N, H, W, cout))
    elif kind == "ds2":
        d = dict(x=r(slots, N, OH, OW, cout), w=r(9, cout, cin) / (9 * cout) ** 0.5, prev=r(slots, N, H, W, cin))
    else:
        d = dict(gz=r(slots, N, OH, OW, cout), x=r(slots, N, H, W, cin), tab=table(slots, cin), prev=0.1 * r(9, cout, cin))
    return d


def inputs(c):
    """The case's dense fp32 tensors (slots first, channels last); shared by all routes and options of a shape.  Do not modify."""
    return _inputs(c.kind, c.stride, c.H, c.W, c.cin, c.cout, c.slots)


def padded(t, ld, canary=CANARY):
    """`t` [..., C] inside a buffer [..., ld] whose other channels hold the canary."""
    buf = torch.full(t.shape[:-1] + (ld,), canary, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    return buf


# ---- the reference: a plain restatement, fp64 by default ---------------------------------------------------------------
def transform(x, tab):
    """a = flag ? silu(scale x + shift) : x; x [..., C], tab [3, C]."""
    y = x * tab[0] + tab[1]
    return torch.where(tab[2] != 0, y * torch.sigmoid(y), x)


def _w4(w):
    """[9][a][b], tap = 3 ky + kx -> [a][b][3][3]."""
    return w.reshape(3, 3, w.shape[1], w.shape[2]).permute(2, 3, 0, 1)


def activated(c, d, dtype, mutant=None):
    """The transformed input of every slot, [S, N, C, H, W], and the conv padding to use with it.  Mutant "pad_silu": the
    padding went through the transform too."""
    x, tab = d["x"].to(dtype), d["tab"].to(dtype)
    outs = []
    for s in range(x.shape[0]):
        t = tab[min(s, tab.shape[0] - 1)]
        if mutant == "slot_table" and s == 2:
            t = tab[0]
        if mutant == "pad_silu":
            outs.append(_nchw(transform(F.pad(x[s], (0, 0, 1, 1, 1, 1)), t)))
        else:
            outs.append(_nchw(transform(x[s], t)))
    return torch.stack(outs), (0 if mutant == "pad_silu" else 1)


def conv_products(c, a, w, pad, mutant=None):
    """What the case's kernel computes from the activated input a [S, N, C, H, W] (ds2: g_z) and the weight, without
    `prev`: [S, N, OH, OW, C'] (dw: [9, cout, cin]).  Linear in a and in w, so the split emulations can call it per plane."""
    S = a.shape[0]
    flat = a.reshape((S * N,) + a.shape[2:])
    if c.kind in ("fwd", "bf16"):
        z = F.conv2d(flat, _w4(w), stride=c.stride, padding=pad)
    elif c.kind == "wt":
        if mutant == "unmirrored":      # the forward conv's taps with the transposed weight
            z = F.conv2d(flat, _w4(w).transpose(0, 1), padding=pad)
        else:
            z = F.conv_transpose2d(flat, _w4(w), padding=2 - pad)      # (pad 0 on a map padded by 1 = crop 2)
    elif c.kind == "ds2":
        if mutant == "drop_last_row":
            flat = flat.clone()
            flat[:, :, -1, :] = 0
        if mutant == "drop_last_col":
            flat = flat.clone()
            flat[:, :, :, -1] = 0
        z = F.conv_transpose2d(flat, _w4(w), stride=2, padding=1, output_padding=1)
    else:
        raise AssertionError(c.kind)
    return _nhwc(z).reshape(S, N, z.shape[2], z.shape[3], z.shape[1])


def dw_products(c, a, gz, pad, mutant=None):
    """dW [9, cout, cin] = sum over slots, images and pixels of g_z[p][o] a[p (+) tap][k]; a [S, N, cin, H(+2), W(+2)],
    gz [S, N, OH, OW, cout]."""
    S = a.shape[0]
    flat = a.reshape((S * N,) + a.shape[2:])
    if mutant == "missing_row":      # the last input row never reaches the sum
        flat = flat.clone()
        flat[:, :, flat.shape[2] - 1 - (1 - pad), :] = 0
    g = _nchw(gz.reshape((S * N,) + gz.shape[2:]))
    gw = torch.nn.grad.conv2d_weight(flat, (c.cout, c.cin, 3, 3), g.contiguous(), stride=c.stride, padding=pad)
    return gw.permute(2, 3, 0, 1).reshape(9, c.cout, c.cin)


def compute(c, dtype=torch.float64, mutant=None):
    """The case's result in `dtype` arithmetic: (out [S, N, OH, OW, C'] or dW [9, cout, cin], stats or None); stats =
    (sum z, sum z^2) per channel over all pixels, [2, C']."""
    d = inputs(c)
    if c.kind == "dw":
        a, pad = activated(c, d, dtype, mutant)
        out = dw_products(c, a, d["gz"].to(dtype), pad, mutant)
    elif c.kind == "ds2":
        a = _nchw_slots(d["x"].to(dtype))
        out = conv_products(c, a, d["w"].to(dtype), 1, mutant)
    else:
        a, pad = activated(c, d, dtype, mutant)
        out = conv_products(c, a, d["w"].to(dtype), pad, mutant)
    if (c.accumulate or c.kind == "dw") and mutant != "no_accumulate":
        out = out + d["prev"].to(dtype)
    stats = torch.stack([out.sum((0, 1, 2, 3)), (out * out).sum((0, 1, 2, 3))]) if c.stats else None
    return out, stats


def _nchw_slots(t):
    return t.permute(0, 1, 4, 2, 3)


@functools.lru_cache(maxsize=None)
def _reference(key):
    return compute(key)


def reference(c):
    """fp64, computed once per (shape, accumulate, stats); shared by the routes.  Do not modify."""
    return _reference(c._replace(route=0, skip=0, max_wg=0))


# ---- emulations of the kernels' number formats (CPU) ---------------------------------------------------------------------
def split3(t):
    """An fp32 tensor as three bf16 planes (jn_split.h): h = bf16(v), m = bf16(v - h), l = bf16(v - h - m)."""
    h = _bf16(t)
    m = _bf16(t - h)
    return h, m, _bf16(t - h - m)


X3_W, X3_X = (2, 0, 1, 1, 0, 0), (0, 2, 1, 0, 1, 0)      # the six products of jn_split.h as (plane of w, plane of x), in issue order


def compute_split(c, drop_hi_lo=False):
    """The split routes in fp32 arithmetic: operands in bf16 planes, the products of jn_split.h summed in fp32, small ones
    first.  Outputs and data gradients: three planes, six products.  Weight gradients: two planes, h l + l h + h h.
    drop_hi_lo: the mutant that forgets the product of one operand's high plane with the other's next plane: (g h, a l)
    of the two-plane form, (w h, x m) of the three-plane form, each about 2^-9 of the sum.  (The three-plane form's (w h, x l)
    is about 2^-17 of it, below every bar of this file, like the three products the scheme drops by design.)"""
    d = inputs(c)
    f32 = torch.float32
    if c.kind == "dw":
        a, pad = activated(c, d, f32)
        ah, al = _bf16(a), _bf16(a - _bf16(a))
        g = d["gz"]
        gh, gl = _bf16(g), _bf16(g - _bf16(g))
        out = torch.zeros(9, c.cout, c.cin)
        for gp, ap in ((gh, al), (gl, ah), (gh, ah)):
            if drop_hi_lo and gp is gh and ap is al:
                continue
            out = out + dw_products(c, ap, gp, pad)
        return out + d["prev"], None
    if c.kind == "ds2":
        a, pad = _nchw_slots(d["x"]), 1
    else:
        a, pad = activated(c, d, f32)
    xp, wp = split3(a), split3(d["w"])
    out = None
    for e in range(6):
        if drop_hi_lo and X3_W[e] == 0 and X3_X[e] == 1:
            continue
        p = conv_products(c, xp[X3_X[e]], wp[X3_W[e]], pad)
        out = p if out is None else out + p
    if c.accumulate:
        out = out + d["prev"]
    stats = torch.stack([out.sum((0, 1, 2, 3)), (out * out).sum((0, 1, 2, 3))]) if c.stats else None
    return out, stats


def compute_bf16(c):
    """The bf16 inference kernel: activations rounded before and after the transform, weight and output rounded, fp32 sums."""
    d = inputs(c)
    rounded = dict(d, x=_bf16(d["x"]))
    a, pad = activated(c, rounded, torch.float32)
    return _bf16(conv_products(c, _bf16(a), _bf16(d["w"]), pad)), None


# ---- distances -----------------------------------------------------------------------------------------------------------
def distances(got, ref):
    """(relative L2, max |delta| / max |ref|) of `got` against the fp64 `ref`."""
    got = got.double()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


def bars(c):
    """(relative-L2 bar, max-norm bar relative to max|ref|, absolute allowance of the max-norm bar) of the case's kernel."""
    if c.kind == "bf16":
        return BF16_L2, BF16_MAX, BF16_ABS
    if c.kind == "dw":
        return (DW_EXACT_L2 if c.route == 3 else float("inf")), DW_MAX, 0.0
    return OUT_L2, OUT_MAX, 0.0


def over_bars(c, got, ref, margin=1.0):
    """[] when `got` is within the case's bars divided by `margin`, else the offending (name, distance, bar) triples."""
    l2, mx = distances(got, ref)
    bl2, bmx, babs = bars(c)
    scale = ref.abs().max().item()
    bad = []
    if not l2 * margin <= bl2:
        bad.append(("relative L2", l2, bl2))
    if not mx * margin <= bmx + babs / scale:
        bad.append(("max-norm / max|ref|", mx, bmx + babs / scale))
    return bad


def stat_moments(sums, count):
    """(mean, var) per channel from (sum z, sum z^2) [2, C]."""
    mean = sums[0] / count
    return mean, sums[1] / count - mean * mean


def stats_over_bar(sums, ref_sums, count):
    """Worst |got - ref| / (STAT_ATOL + STAT_RTOL |ref|) over the mean and the variance of every channel (<= 1 passes)."""
    worst = 0.0
    for g, r in zip(stat_moments(sums.double(), count), stat_moments(ref_sums, count)):
        worst = max(worst, ((g - r).abs() / (STAT_ATOL + STAT_RTOL * r.abs())).max().item())
    return worst
