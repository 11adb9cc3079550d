"""Cases, inputs, fp64 references and bars for the kernels that run between the convolutions of a train-mode pass
(csrc/kernels_conv.hip: stem_mfma_kernel, spp_kernel, spp4_kernel, upsample_kernel, addact_kernel, bn_finalize_kernel,
bn_finalize_all_kernel, efpn_linear_kernel, efpn_linear_mfma_kernel; csrc/kernels_bwd.hip: bn_bwd_reduce_kernel, bn_bwd_consts_kernel,
wpart_reduce_kernel, stem_bwd_weight_kernel, spp_bwd_kernel, spp4_bwd_kernel, upsample_bwd_kernel), one kernel at a time through the
context-free entries jn_stem, jn_stem_bwd_weight, jn_spp, jn_spp_bwd, jn_upsample, jn_upsample_bwd, jn_addact, jn_bn_finalize,
jn_bn_finalize_all, jn_bn_bwd_sums and jn_efpn_linear.

Shared by tests/test_glue_cases_cpu.py (the restatements are the torch modules, the bars mean something on these inputs and bite on
the mistakes such kernels make) and tests/test_gpu_glue_kernels.py (every kernel against the reference).  Fixed seeds, no committed
tensors.  N = 2 images, read-side leading dimensions C + 8, written-side C + 4, as in the other kernel pins.

A case is a Case tuple; the fields a family does not use stay at their defaults:
 - kind: "stem" / "stemw" (P, cout, src, align, pos, dtype, stats, nrep, skip, max_wg, slots, z), "spp" / "sppb" (route, H, W, C = the
   slice width h, dtype, slots, skip), "up" / "upb" / "add" (H, W, C, dtype, slots, accumulate, skip, ints, M), "bnf" (C, M = the count,
   t1, save, run, skip), "bnall" (skip), "bnb" (C, M, slots, raw, consts), "ef" (N, K, C = Co, KS, skip);
 - skip: 0 = no flag, 1 = a flag below skip_when (the launch runs), 2 = a flag at skip_when (nothing may change);
 - src: 0 = fp32 image, 1 = uint8; align: 0 = rows as allocated, 1 = the base one element off, 2 = an odd row stride (both force
   the 4-byte path); pos: 0 = no positions, 1 = patches inside larger images whose other pixels hold 1e3 (uint8: 255).

Shapes are the smallest with an edge.  Stem (tiles of 16 x 32 output pixels forward, 8 x 32 backward, OH = P / 2): P = 4 (one tile,
almost all padding), 30 (P % 4 != 0: the 4-byte path; one partial tile), 66 (4-byte path; a second column tile of one pixel, a third
row tile of one), 68 (16-byte path; 2 x 3 tiles), 96 (16-byte path; 2 x 3 full tiles: with N = 2 the 12 tiles max_wg = 1 and 5 make
one workgroup, then five, walk).  SPP: 1 x 1, 3 x 5 (smaller than every window), 7 x 7 (the 13-window passes both borders everywhere),
14 x 14 (the workload's), 13 x 20.  Upsample and the shortcut sum: 1 x 1, 3 x 5, 7 x 7 at C = 4, 20, 64, and M = 65600 at C = 64
(the grid-stride loop of addact_kernel runs twice).  BatchNorm sums: C = 16 ... 1024 at M = 1, one row below and above a workgroup's
rows, and past 32 workgroups (the replica index wraps).  embed_fpn linear: N = 1, 3, 65 agents, Co = 16 ... 112, K slices that end
off a multiple of 64, are short, or empty."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from tests.conv3_cases import (BF16_ABS, BF16_L2, BF16_MAX, CANARY, CANARY_BF16, DW_MAX, DW_ORDER, NREP, OUT_L2, OUT_MAX,      # noqa: F401
                               SKIP_WHEN, STAT_ATOL, STAT_RTOL, distances, padded, stats_over_bar, transform)
from tests.dw_cases import RED_BAR
from tests.kernel_helpers import _bf16, _dsilu

_FIELDS = "kind route P H W C cout K KS N M src align pos dtype stats nrep skip max_wg slots z accumulate ints t1 save run raw consts"
Case = collections.namedtuple("Case", _FIELDS)
_DEFAULTS = dict(route=0, P=0, H=0, W=0, C=0, cout=0, K=0, KS=0, N=2, M=0, src=0, align=0, pos=0, dtype=0, stats=0, nrep=NREP, skip=0, max_wg=0,
                 slots=1, z=0, accumulate=0, ints=0, t1=0, save=0, run=0, raw=0, consts=0)


def _case(kind, **kw):
    return Case(kind, **dict(_DEFAULTS, **kw))


N = 2                       # images: the image stride is exercised
IN_PAD, OUT_PAD = 8, 4      # read-side leading dimensions C + 8, written-side C + 4
WPART_MAX = 16384           # JN_WPART_MAX: floats per replica of the weight-gradient scratch
NREP_DEFER = 8              # JN_NREP_DEFER: replicas a layer with a deferred table accumulates into
BN_EPS, BN_MOMENTUM = 1e-3, 0.03
ST_TY, ST_TX, SB_TY, SB_TX = 16, 32, 8, 32      # the stem's tiles in output pixels, forward and weight gradient
GRID = 5                    # pos = 1: images of GRID x GRID patches; the patches read sit at odd indices, so none is first or last

# ---- the bars: those of conv3_cases.py and dw_cases.py (imported above), and three of this unit -----------------------------------
# Measured as RED_BAR was: plain fp32 arithmetic in the natural order against fp64 on the cases of this file
# (test_glue_cases_cpu.py prints the figures), the bar 4 x that, rounded up to one digit.
# embed_fpn partial sums, one k after the other: per (agent, slice, output), |delta| over the sum of |terms|
EF_FP32_MEASURED = 1.1e-7    # (N = 65, K = 36 in 4 slices, 112 outputs)
EF_BAR = 5e-7
# BatchNorm table, saved and running statistics (fp32 BatchNorm over the fp32 data: mean, then the mean of the squared deviations),
# per value |delta| over the sum of its |terms| (scale: itself; shift: |beta| + |mean scale|; mean: the mean of |x|; invstd: itself;
# running values: (1 - m) |old| + m |new|)
BN_FP32_MEASURED = 2.0e-7    # (the shift of the 300-value cases)
BN_BAR = 8e-7
K_RTOL = 2.0 ** -23         # consts[2] = gamma * invstd, one fp32 product of fp32 inputs: half an ulp, doubled


# ==== stem =========================================================================================================================
def _stem_cases(odt, vec, src, bwd=False):
    kind = "stemw" if bwd else "stem"
    mk = lambda P, **o: _case(kind, P=P, **dict(dict(cout=32, dtype=odt, src=src, align=0 if (vec or P % 4) else 1), **o))
    edge = 68 if vec else 66
    cases = [mk(P) for P in ((4, 68, 96) if vec else (30, 66))]
    if not vec:
        cases += [mk(68, align=1), mk(68, align=2)]
    walk = dict(align=0 if vec else 1)
    if not bwd:
        cases += [mk(edge, cout=c, stats=1, nrep=8) for c in (16, 48)]
        cases += [mk(edge, pos=1), mk(edge, pos=1, stats=1), mk(4 if vec else 30, pos=1), mk(edge, stats=1), mk(edge, stats=1, nrep=8),
                  mk(edge, stats=1, skip=1), mk(edge, stats=1, skip=2)]
        cases += [mk(96, stats=1, max_wg=m, **walk) for m in (1, 5)] + ([] if vec else [mk(96, **walk)])
    else:
        cases += [mk(edge, cout=c) for c in (16, 48)]
        cases += [mk(edge, z=1), mk(edge, pos=1), mk(edge, pos=1, z=1, slots=3), mk(4 if vec else 30, pos=1, z=1), mk(edge, slots=3),
                  mk(edge, slots=4, z=1), mk(edge, slots=4)]
        cases += [mk(96, z=1, max_wg=m, **walk) for m in (1, 5)] + [mk(96, slots=3, max_wg=5, **walk)] + ([] if vec else [mk(96, **walk)])
    return cases


def stem_vec(c):
    """Whether stem_rows_aligned lets the launch fetch 4-element groups."""
    return c.P % 4 == 0 and c.align == 0


def stem_tiles(c):
    th, tw = (SB_TY, SB_TX) if c.kind == "stemw" else (ST_TY, ST_TX)
    OH = c.P // 2
    return -(-OH // th), -(-OH // tw)


def _interior(i):
    """The i-th patch position (y, x) of a pos = 1 image: odd indices of the GRID x GRID patches, no two adjacent."""
    spots = [(1, 1), (1, 3), (3, 1), (3, 3)]
    return spots[i % 4]


def stem_pack(w_t):
    """The engine's layout conversion (api_ctx.hip, PK_STEM): the Focus conv's weight [oc][q * 3 + c][ky][kx], Focus order top-left,
    bottom-left, top-right, bottom-right (q = py + 2 px), -> [(c * 6 + dy) * 6 + dx][oc] with dy = 2 ky + py, dx = 2 kx + px."""
    cout = w_t.shape[0]
    w = w_t.reshape(cout, 2, 2, 3, 3, 3)                 # [oc][px][py][c][ky][kx]
    return w.permute(3, 4, 2, 5, 1, 0).reshape(108, cout)      # [c][ky][py][kx][px][oc]


def focus_conv(x, w_t):
    """The module: Focus slicing (yolox network_blocks.Focus), then the 3 x 3 conv with padding 1.  x [n, 3, P, P] -> [n, cout, P/2, P/2]."""
    tl, tr, bl, br = x[..., ::2, ::2], x[..., ::2, 1::2], x[..., 1::2, ::2], x[..., 1::2, 1::2]
    return F.conv2d(torch.cat((tl, bl, tr, br), dim=1), w_t, padding=1)


def _w6(w):
    """[108][cout], k = 36 c + 6 dy + dx -> [cout][3][6][6]."""
    return w.t().reshape(w.shape[1], 3, 6, 6)


def folded_conv(x, w, around=None):
    """The kernel's form: the 6 x 6 stride-2 conv of the patch with zero padding 2.  `around` [n, 3, P + 4, P + 4]: what lies around
    the patch in its image instead of the zeros (the mutant "neighbour")."""
    if around is None:
        return F.conv2d(x, _w6(w), stride=2, padding=2)
    full = around.clone()
    full[..., 2:-2, 2:-2] = x
    return F.conv2d(full, _w6(w), stride=2)


@functools.lru_cache(maxsize=None)
def _stem_inputs(P, cout, pos, slots, bwd):
    g = torch.Generator().manual_seed(((P * 64 + cout) * 2 + pos) * 8 + slots + (100003 if bwd else 0))
    S = slots if pos else 1           # without positions every slot reads the same images
    OH = P // 2
    d = dict(bytes=torch.randint(0, 256, (S, N, 3, P, P), generator=g, dtype=torch.uint8),
             w_t=torch.randn(cout, 12, 3, 3, generator=g) / 108 ** 0.5)
    if bwd:
        r = lambda *s: torch.randn(*s, generator=g)
        u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
        otab = torch.stack([u(0.5, 1.5, slots, cout), 0.5 * r(slots, cout), torch.ones(slots, cout)], 1)
        d.update(g=r(slots, N, OH, OH, cout), zz=r(slots, N, OH, OH, cout), otab=otab,
                 save=torch.stack([0.3 * r(slots, cout), u(0.5, 2.0, slots, cout)], -1),
                 consts=torch.stack([0.1 * r(slots, cout), 0.1 * r(slots, cout), u(0.5, 1.5, slots, cout)], -1), gw0=0.1 * r(108, cout))
    return d


def stem_image(c, as_u8):
    """(storage, element offset of image 0, sample / channel / row strides, positions [S, N, 2] or None): what the entry reads for the
    case.  pos = 1: the patch of slot s sits at _interior(s + n) of image n (at most four slots), everything else holds 1e3 (uint8: 255)."""
    d = inputs(c)
    by = d["bytes"]
    val = (lambda t: t) if as_u8 else (lambda t: t.float() / 255)
    dt = torch.uint8 if as_u8 else torch.float32
    P = c.P
    if c.pos:
        img = torch.full((N, 3, GRID * P, GRID * P), 255 if as_u8 else 1e3, dtype=dt)
        pos = torch.empty(by.shape[0], N, 2, dtype=torch.int64)
        for s in range(by.shape[0]):
            for n in range(N):
                y, x = _interior(s + n)
                pos[s, n, 0], pos[s, n, 1] = y, x
                img[n, :, y * P:(y + 1) * P, x * P:(x + 1) * P] = val(by[s, n])
        return img.reshape(-1), 0, 3 * (GRID * P) ** 2, (GRID * P) ** 2, GRID * P, pos
    rs = P + 1 if c.align == 2 else P
    img = torch.full((N, 3, P, rs), 255 if as_u8 else 1e3, dtype=dt)
    img[..., :P] = val(by[0])
    off = 1 if c.align == 1 else 0
    flat = torch.cat([torch.zeros(off, dtype=dt), img.reshape(-1)])
    return flat, off, 3 * P * rs, P * rs, rs, None


def _stem_gz(c, d, s, mutant=None):
    if not c.z:
        return d["g"][s]
    otab, save, consts = d["otab"][s], d["save"][s], d["consts"][s]
    y = d["zz"][s] * otab[0] + otab[1]
    zhat = (d["zz"][s] - save[:, 0]) * save[:, 1]
    return consts[:, 2] * (d["g"][s] * _dsilu(y) - consts[:, 0] - zhat * consts[:, 1])


def _compute_stem(c, dtype, mutant):
    """Mutants: "neighbour" (a pixel of the image instead of the zero padding: 1e3 around a pos = 1 patch, else the patch's own border
    repeated), "drop_last_col" (the last column tile never computed / never added)."""
    d = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inputs(c).items()}
    w = stem_pack(d["w_t"])
    x = d["bytes"].to(dtype) / 255                                     # [S or 1, N, 3, P, P]
    OH = c.P // 2
    tx = SB_TX if c.kind == "stemw" else ST_TX
    last_col = (stem_tiles(c)[1] - 1) * tx

    def around(xs):
        if mutant != "neighbour":
            return None
        return torch.full((N, 3, c.P + 4, c.P + 4), 1e3, dtype=dtype) if c.pos else F.pad(xs, (2, 2, 2, 2), mode="replicate")
    if c.kind == "stem":
        out = folded_conv(x[0], w, around(x[0])).permute(0, 2, 3, 1).contiguous()
        if mutant == "drop_last_col":
            out[:, :, last_col:] = 0
        res = dict(out=out)
        if c.stats:
            res["stats"] = torch.stack([out.sum((0, 1, 2)), (out * out).sum((0, 1, 2))])
        return res
    dw = d["gw0"].clone()
    for s in range(c.slots):
        xs = x[s if c.pos else 0]
        gz = _stem_gz(c, d, s).permute(0, 3, 1, 2).contiguous()
        if mutant == "drop_last_col":
            gz[..., last_col:] = 0
        ar = around(xs)
        full = F.pad(xs, (2, 2, 2, 2)) if ar is None else ar
        if ar is not None:
            full = full.clone()
            full[..., 2:-2, 2:-2] = xs
        gw = torch.nn.grad.conv2d_weight(full, (c.cout, 3, 6, 6), gz, stride=2)
        dw = dw + gw.reshape(c.cout, 108).t()
    return dict(dw=dw)


# ==== SPP ==========================================================================================================================
SPP_SHAPES = ((1, 1), (3, 5), (7, 7), (14, 14), (13, 20))
SPP_K = (5, 9, 13)


def _spp_cases(kind, route, dtype=0):
    mk = lambda hw, h, **o: _case(kind, route=route, H=hw[0], W=hw[1], C=h, dtype=dtype, **o)
    cases = [mk(hw, 16) for hw in SPP_SHAPES]
    cases += [mk((14, 14), h) for h in ((32,) if route == 1 else (8, 24))]
    if kind == "spp":
        cases += [mk((7, 7), 16, skip=1), mk((7, 7), 16, skip=2)]
    else:
        cases += [mk((7, 7), 16, slots=3), mk((13, 20), 16, slots=3)]
    return cases


@functools.lru_cache(maxsize=None)
def _spp_inputs(H, W, h, slots):
    g = torch.Generator().manual_seed(((H * 64 + W) * 64 + h) * 8 + slots)
    S, n = slots, N * H * W
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    flag = (torch.rand(S, h, generator=g) < 0.75).float()
    flag[:, 1] = 0.0                                                   # every table has a raw channel
    # transformed channels: z a random permutation of a 0.01-spaced lattice, scale > 0 and shift such that y lies in [0.1, 4]
    smax = min(1.5, 3.9 / (0.01 * max(n - 1, 1)))
    sc = smax * u(0.7, 1.0, S, h)
    z0 = u(-1.0, 1.0, S, h)
    span = sc * 0.01 * (n - 1)
    sh = 0.1 + u(0.0, 1.0, S, h) * (3.9 - span) - sc * z0
    lattice = torch.stack([torch.stack([z0[s, c] + 0.01 * torch.randperm(n, generator=g) for c in range(h)], -1) for s in range(S)])
    raw = torch.randint(0, 3, (S, n, h), generator=g).float()           # raw channels: {0, 1, 2}, ties everywhere
    z = torch.where(flag[:, None, :] != 0, lattice, raw).reshape(S, N, H, W, h)
    ints = lambda: torch.randint(-3, 4, (S, N, H, W, h), generator=g).float()
    return dict(x=z, tab=torch.stack([sc, sh, flag], 1), g0=ints(), g=torch.stack([ints(), ints(), ints()]))      # g: [3][S, ...]


def spp_activation(c, dtype=torch.float64, tensors=None):
    """[S, N, h, H, W]."""
    d = tensors or inputs(c)
    return torch.stack([transform(d["x"][s].to(dtype), d["tab"][s].to(dtype)) for s in range(c.slots)]).permute(0, 1, 4, 2, 3)


def route_first(a, g, k, last=False):
    """The pooled gradient g of the k-window max-pool of a (both [n, C, H, W]) sent to the FIRST maximum of every window in row-major
    order (last: to the last one, the mutant).  A restatement without autograd: windows unfolded, -inf padding."""
    n, C, H, W = a.shape
    p = k // 2
    win = F.unfold(F.pad(a, (p, p, p, p), value=-math.inf).reshape(n * C, 1, H + 2 * p, W + 2 * p), k)      # [nC, k k, H W]
    mask = win == win.max(1, keepdim=True).values
    if last:
        mask = mask.flip(1)
    one = mask & (mask.cumsum(1) == 1)
    if last:
        one = one.flip(1)
    full = F.fold(one.to(a.dtype) * g.reshape(n * C, 1, H * W), (H + 2 * p, W + 2 * p), k)
    return full[:, 0, p:p + H, p:p + W].reshape(n, C, H, W)


def _compute_spp(c, dtype, mutant, tensors=None):
    """bf16 maps: the reference pools the bf16 values the kernel is handed (a rounded lattice has ties and gaps of one bf16 step: the
    forward does not care), so that the bars hold what the kernel adds: fp32 arithmetic and the rounding of its output."""
    d = tensors or inputs(c)
    if c.dtype and tensors is None:
        d = dict(d, x=_bf16(d["x"]))
    a = spp_activation(c, dtype, d)                                     # [S, N, h, H, W]
    flat = a.reshape((-1,) + a.shape[2:])
    nhwc = lambda t: t.reshape(a.shape).permute(0, 1, 3, 4, 2)
    if c.kind == "spp":
        return dict(pooled=torch.stack([nhwc(F.max_pool2d(flat, k, 1, k // 2)) for k in SPP_K])[:, 0])      # [3][N, H, W, h]
    g0 = d["g0"].to(dtype)
    if mutant == "autograd":      # torch's own backward instead of the restatement
        leaf = flat.clone().requires_grad_(True)
        loss = sum((F.max_pool2d(leaf, k, 1, k // 2) * d["g"][i].to(dtype).permute(0, 1, 4, 2, 3).reshape(flat.shape)).sum() for i, k in enumerate(SPP_K))
        grad = torch.autograd.grad(loss, leaf)[0]
    else:
        grad = sum(route_first(flat, d["g"][i].to(dtype).permute(0, 1, 4, 2, 3).reshape(flat.shape), k, last=mutant == "last_max")
                   for i, k in enumerate(SPP_K))
    return dict(g0=g0 + nhwc(grad))


# ==== upsample, shortcut sum ===========================================================================================================
UP_SHAPES = ((1, 1), (3, 5), (7, 7))
UP_CHANNELS = (4, 20, 64)
ADD_LOOP_M = 65600           # M * C / 4 above 4096 * 256 at C = 64: the grid-stride loop runs twice


def _up_cases(kind, dtype=0):
    mk = lambda hw, C, **o: _case(kind, H=hw[0], W=hw[1], C=C, dtype=dtype, M=N * hw[0] * hw[1], **o)
    cases = [mk(hw, C) for hw in UP_SHAPES for C in UP_CHANNELS]
    if kind == "upb":
        cases = [c._replace(ints=1) for c in cases]
        cases += [mk((7, 7), 20, accumulate=1, ints=1), mk((7, 7), 20, slots=3, ints=1), mk((7, 7), 20, slots=3, accumulate=1, ints=1)]
        cases += [mk((7, 7), 20), mk((3, 5), 64, accumulate=1), mk((7, 7), 4, slots=3, accumulate=1)]
    else:
        cases += [mk((3, 5), 20, skip=1), mk((3, 5), 20, skip=2)]
    if kind == "add":
        cases += [_case(kind, C=C, dtype=dtype, M=1) for C in UP_CHANNELS]
        if not dtype:
            cases.append(_case(kind, C=64, M=ADD_LOOP_M))
    return cases


def _mixed_table(g, C, shift_scale=1.0):
    t = torch.empty(3, C)
    t[0] = 0.5 + torch.rand(C, generator=g)
    t[1] = 0.5 * torch.randn(C, generator=g) * shift_scale
    t[2] = (torch.rand(C, generator=g) < 0.75).float()
    t[2, 1 % C] = 0.0
    t[2, 0] = 1.0
    return t


@functools.lru_cache(maxsize=None)
def _up_inputs(kind, H, W, C, dtype, slots, ints, M):
    g = torch.Generator().manual_seed((((("up", "upb", "add").index(kind) * 64 + H) * 64 + W) * 128 + C) * 64 + dtype * 32 + slots * 2 + ints + M * 7)
    r = lambda *s: torch.randn(*s, generator=g)
    if kind == "up":
        return dict(x=r(N, H, W, C).to(torch.bfloat16).float())      # bf16-exact: the copy is held to the bits with either storage
    if kind == "upb":
        mk = (lambda *s: torch.randint(-4, 5, s, generator=g).float()) if ints else r
        return dict(g=mk(slots, N, 2 * H, 2 * W, C), gsrc0=mk(slots, N, H, W, C))
    # bf16 maps: outputs of about 0.03, where the absolute part of the max-norm bar leaves a 2x margin (dw_cases.py)
    small = 1.0 / 64 if dtype else 1.0
    return dict(z=r(M, C) * small, res=r(M, C) * small, ztab=_mixed_table(g, C, small), rtab=_mixed_table(g, C, small))


def _compute_up(c, dtype, mutant, tensors=None):
    d = tensors or inputs(c)
    if c.kind == "add" and c.dtype and tensors is None:      # bf16 maps: the reference adds the bf16 values the kernel is handed (as _compute_spp)
        d = dict(d, z=_bf16(d["z"]), res=_bf16(d["res"]))
    d = {k: v.to(dtype) for k, v in d.items()}
    if c.kind == "up":
        return dict(out=d["x"].repeat_interleave(2, 1).repeat_interleave(2, 2))
    if c.kind == "upb":
        s = d["g"]
        pooled = s[:, :, 0::2, 0::2] + s[:, :, 0::2, 1::2] + s[:, :, 1::2, 0::2] + s[:, :, 1::2, 1::2]      # the kernel's order: dy, then dx
        return dict(out=pooled + d["gsrc0"] if c.accumulate else pooled)
    return dict(out=transform(d["z"], d["ztab"]) + transform(d["res"], d["rtab"]))


def compute_bf16(c):
    """bf16 storage: the maps hold bf16, everything between them is fp32."""
    d = inputs(c)
    if c.kind == "spp":
        res = _compute_spp(c, torch.float32, None, dict(d, x=_bf16(d["x"])))
        return dict(pooled=_bf16(res["pooled"]))
    if c.kind == "add":
        res = _compute_up(c, torch.float32, None, dict(d, z=_bf16(d["z"]), res=_bf16(d["res"])))
    else:
        res = _compute_up(c, torch.float32, None, dict(d, x=_bf16(d["x"])))
    return dict(out=_bf16(res["out"]))


# ==== BatchNorm tables =================================================================================================================
BNF_CHANNELS = (1, 20, 33, 64)
BNF_COUNTS = (1, 300, 4096)
BNALL_LAYERS = ((49, 5, 0), (0, 3, 0), (700, 6, 1), (9, 4, 1))      # (hw, channels, with an alias column): N * hw = 98, -, 1400, 18
BNALL_DEFER_MAX_M = 1000     # the 700-pixel layer is above it: all 32 replicas count


def _bnf_cases():
    mk = lambda C, M, **o: _case("bnf", C=C, M=M, **dict(dict(t1=1, save=1, run=1), **o))
    cases = [mk(C, 300) for C in BNF_CHANNELS] + [mk(33, M) for M in BNF_COUNTS if M != 300]
    cases += [mk(33, 300, t1=0), mk(33, 300, save=0), mk(33, 300, run=0), mk(33, 300, t1=0, save=0, run=0), mk(33, 300, skip=1), mk(33, 300, skip=2)]
    return cases


def _bn_data(g, n, C):
    """[n, C] fp64: channel 0 constant (its variance cancels to a hair around zero: the clamp, invstd = 1 / sqrt(eps)), channel 1 with
    mean 100 and standard deviation 0.01, the rest with means and deviations of order 1."""
    x = (torch.randn(n, C, generator=g, dtype=torch.float64) * (0.2 + 2 * torch.rand(C, generator=g, dtype=torch.float64)) +
         2 * torch.randn(C, generator=g, dtype=torch.float64))
    x[:, 0] = 3.7
    if C > 1:
        x[:, 1] = 100 + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)
    return x.float().double()          # fp32-exact data: the fp32 restatement reads the same numbers


def _replica_sums(x, nrep, stride, fill=0.0):
    """(sum, sum of squares) of the rows of x [n, C] spread over the first nrep of the NREP replicas, [NREP, stride] fp64; the other
    replicas and the columns past 2 C hold `fill`."""
    n, C = x.shape
    st = torch.full((NREP, stride), fill, dtype=torch.float64)
    st[:nrep, :2 * C] = 0.0
    for r in range(nrep):
        rows = x[r::nrep]
        st[r, 0:2 * C:2] = rows.sum(0)
        st[r, 1:2 * C:2] = (rows * rows).sum(0)
    return st


@functools.lru_cache(maxsize=None)
def _bnf_inputs(C, M):
    g = torch.Generator().manual_seed(C * 8192 + M)
    x = _bn_data(g, M, C)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=x, stats=_replica_sums(x, NREP, 2 * C + 6), gamma=0.5 + torch.rand(C, generator=g), beta=0.5 * r(C), run_mean0=r(C),
                run_var0=0.5 + torch.rand(C, generator=g))


@functools.lru_cache(maxsize=None)
def _bnall_inputs():
    g = torch.Generator().manual_seed(4242)
    n_stat = sum(l[1] for l in BNALL_LAYERS)
    tab_channels = n_stat + 10
    stats = torch.zeros(NREP, 2 * n_stat, dtype=torch.float64)
    xs, hw, t0, t1 = [], [], [], []
    i0 = 0
    perm = torch.randperm(tab_channels, generator=g).tolist()
    for hw_l, C, alias in BNALL_LAYERS:
        big = N * hw_l > BNALL_DEFER_MAX_M
        x = _bn_data(g, max(N * hw_l, 1), C)
        # a small layer's replicas past JN_NREP_DEFER hold the canary: they must be ignored
        stats[:, 2 * i0:2 * (i0 + C)] = _replica_sums(x, NREP if big else NREP_DEFER, 2 * C, fill=0.0 if big else CANARY)
        xs.append(x)
        hw += [float(hw_l)] * C
        t0 += [perm.pop() for _ in range(C)]
        t1 += [perm.pop() if alias and j % 2 == 0 else -1 for j in range(C)]
        i0 += C
    params = torch.randn(2 * n_stat + 5, generator=g)                  # weights (of order 1) in a shuffled first part, biases after a gap
    params[:n_stat] = 0.5 + torch.rand(n_stat, generator=g)
    goff, boff = torch.randperm(n_stat, generator=g), n_stat + 5 + torch.randperm(n_stat, generator=g)
    return dict(xs=xs, stats=stats, hw=torch.tensor(hw), t0=torch.tensor(t0, dtype=torch.int32), t1=torch.tensor(t1, dtype=torch.int32),
                goff=goff.to(torch.int32), boff=boff.to(torch.int32), params=params,
                run_mean0=torch.randn(n_stat, generator=g), run_var0=0.5 + torch.rand(n_stat, generator=g), n_stat=n_stat, tab_channels=tab_channels)


def bn_from_sums(s1, s2, count, gamma, beta, rm0, rv0):
    """Train-mode BatchNorm from the fp64 totals, in fp64: (scale, shift, mean, invstd, new running mean, new running variance)."""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    sc = gamma * invstd
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return sc, beta - mean * sc, mean, invstd, (1 - BN_MOMENTUM) * rm0 + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * rv0 + BN_MOMENTUM * unbiased


def bn_two_pass(x, gamma, beta, rm0, rv0, dtype):
    """The same from the data, mean first, then the mean of the squared deviations: BatchNorm in `dtype` arithmetic, rows in order."""
    x, gamma, beta, rm0, rv0 = (t.to(dtype) for t in (x, gamma, beta, rm0, rv0))
    n = x.shape[0]
    mean = x.cumsum(0)[-1] / n
    var = ((x - mean) ** 2).cumsum(0)[-1] / n
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    sc = gamma * invstd
    unbiased = var * n / (n - 1.0) if n > 1 else var
    return sc, beta - mean * sc, mean, invstd, (1 - BN_MOMENTUM) * rm0 + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * rv0 + BN_MOMENTUM * unbiased


BN_NAMES = ("scale", "shift", "mean", "invstd", "run_mean", "run_var")


def bn_terms(x, ref, gamma, beta, rm0, rv0):
    """The sum of |terms| of each of the six values of bn_from_sums, per channel: the scale of BN_BAR."""
    sc, sh, mean, invstd, _, _ = ref
    n = x.shape[0]
    var = (1.0 / invstd ** 2 - BN_EPS).clamp_min(0.0)
    unbiased = var * n / (n - 1.0) if n > 1 else var
    mean_abs = x.abs().mean(0)
    return (sc.abs(), beta.abs().double() + (mean * sc).abs(), mean_abs, invstd, (1 - BN_MOMENTUM) * rm0.abs().double() + BN_MOMENTUM * mean_abs,
            (1 - BN_MOMENTUM) * rv0.abs().double() + BN_MOMENTUM * unbiased)


def bn_distance(got, ref, terms):
    """Worst |delta| / sum of |terms| over the six values (got: any of them None = not produced)."""
    worst = 0.0
    for g, r, t in zip(got, ref, terms):
        if g is not None:
            worst = max(worst, ((g.double() - r).abs() / t).max().item())
    return worst


def _compute_bnf(c, dtype, mutant):
    d = inputs(c)
    if c.kind == "bnf":
        if dtype == torch.float32:
            vals = bn_two_pass(d["x"], d["gamma"], d["beta"], d["run_mean0"], d["run_var0"], dtype)
        else:
            C = c.C
            tot = d["stats"].sum(0)
            vals = bn_from_sums(tot[0:2 * C:2], tot[1:2 * C:2], float(c.M), d["gamma"].double(), d["beta"].double(), d["run_mean0"].double(),
                                d["run_var0"].double())
        return dict(bn=vals, terms=bn_terms(d["x"], vals, d["gamma"], d["beta"], d["run_mean0"], d["run_var0"]))
    # bnall: per channel; None where the layer is not of this pass.  Mutant "all_replicas": a small layer summed over all 32
    out, terms = [], []
    i0 = 0
    for (hw_l, C, _), x in zip(BNALL_LAYERS, d["xs"]):
        idx = torch.arange(i0, i0 + C)
        gamma, beta = d["params"][d["goff"][idx].long()], d["params"][d["boff"][idx].long()]
        rm0, rv0 = d["run_mean0"][idx], d["run_var0"][idx]
        if hw_l <= 0:
            out.append(None)
            terms.append(None)
        elif dtype == torch.float32:
            out.append(bn_two_pass(x, gamma, beta, rm0, rv0, dtype))
            terms.append(bn_terms(x, out[-1], gamma, beta, rm0, rv0))
        else:
            nrep = NREP if (N * hw_l > BNALL_DEFER_MAX_M or mutant == "all_replicas") else NREP_DEFER
            tot = d["stats"][:nrep, 2 * i0:2 * (i0 + C)].sum(0)
            out.append(bn_from_sums(tot[0::2], tot[1::2], float(N * hw_l), gamma.double(), beta.double(), rm0.double(), rv0.double()))
            terms.append(bn_terms(x, out[-1], gamma, beta, rm0, rv0))
        i0 += C
    return dict(layers=out, terms=terms)


# ==== BatchNorm backward sums ==========================================================================================================
BNB_CHANNELS = (16, 48, 64, 256, 512, 1024)


def bnb_rows_per_block(C):
    """launch_bn_bwd_reduce: 256 / (C / 4) rows at a time, 32 times."""
    return (256 // (C // 4)) * 32


def _bnb_cases():
    mk = lambda C, M, **o: _case("bnb", C=C, M=M, **o)
    cases = []
    for C in BNB_CHANNELS:
        rpb = bnb_rows_per_block(C)
        for M in ((1,) if C in (16, 48) else ()) + (rpb - 1, rpb + 1, 33 * rpb + 3):
            cases.append(mk(C, M, consts=1 if M != 1 else 0))
    cases += [mk(C, bnb_rows_per_block(C) + 1, slots=3, consts=k) for C in (48, 64) for k in (0, 1)]
    cases += [mk(C, 77, raw=1, consts=1, slots=s) for C in (20, 256) for s in (1, 3)]       # consts alone, from a consumer's sums against y
    return cases


@functools.lru_cache(maxsize=None)
def _bnb_inputs(C, M, slots, raw):
    g = torch.Generator().manual_seed(((C * 131072 + M) * 4 + slots) * 2 + raw)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    S = slots
    gamma = u(0.5, 1.5, C)
    gamma[2 % C] = 0.0                                                  # a dead channel: k = 0, and with a raw moment d gamma reported as 0
    beta = 0.5 * r(C)
    save = torch.stack([0.3 * r(S, C), u(0.5, 2.0, S, C)], -1)          # (mean, invstd)
    if raw:                                                             # a consumer's sums are against y = gamma zhat + beta: that table
        tab = torch.stack([gamma * save[..., 1], beta - save[..., 0] * gamma * save[..., 1], torch.ones(S, C)], 1)
    else:                                                               # the reduce kernel takes any table: drawn freely
        tab = torch.stack([u(0.5, 1.5, S, C), 0.5 * r(S, C), torch.ones(S, C)], 1)
    z = r(S, M, C)
    if M == 1:      # a sum of ONE term is relative to that term alone, and silu' crosses zero at y = -1.278, where its relative error in
        z, tab[:, 1] = z.abs(), tab[:, 1].abs()      # any finite precision is unbounded: the single row stays at y > 0
    return dict(g=r(S, M, C), z=z, tab=tab, save=save, gamma=gamma, beta=beta, g_gamma0=0.1 * r(C), g_beta0=0.1 * r(C))


def _order_sum(t, dtype):
    """[M, C] -> [C]; fp32: one row after the other (what an accumulator does; torch.sum adds pairwise)."""
    return t.cumsum(0)[-1] if dtype == torch.float32 else t.sum(0)


def _compute_bnb(c, dtype, mutant):
    """"red" [S, 2, C]: (sum gy, sum gy zhat), or with raw (sum gy, sum gy y); "red_abs" the sums of the absolute terms; with consts:
    "consts" [S, C, 3], "g_gamma", "g_beta" [C] and their scales.  Mutant "swap" (C / 4 = 12: two channels of the butterfly swapped)."""
    d = {k: v.to(dtype) for k, v in inputs(c).items()}
    reds, red_abs = [], []
    for s in range(c.slots):
        y = d["z"][s] * d["tab"][s, 0] + d["tab"][s, 1]
        gy = d["g"][s] * _dsilu(y)
        t2 = gy * (y if c.raw else (d["z"][s] - d["save"][s, :, 0]) * d["save"][s, :, 1])
        reds.append(torch.stack([_order_sum(gy, dtype), _order_sum(t2, dtype)]))
        red_abs.append(torch.stack([gy.abs().sum(0), t2.abs().sum(0)]))
    red, red_abs = torch.stack(reds), torch.stack(red_abs)
    if mutant == "swap":
        red = red.clone()
        red[..., [4, 16]] = red[..., [16, 4]]
    res = dict(red=red, red_abs=red_abs)
    if c.consts:
        s1, s2, a1, a2 = red[:, 0], red[:, 1], red_abs[:, 0], red_abs[:, 1]
        if c.raw:
            live = d["gamma"] != 0
            gm = torch.where(live, d["gamma"], torch.ones_like(d["gamma"]))
            s2 = torch.where(live, (s2 - d["beta"] * s1) / gm, torch.zeros_like(s2))
            a2 = torch.where(live, (a2 + d["beta"].abs() * a1) / gm.abs(), torch.zeros_like(a2))
        res["consts"] = torch.stack([s1 / c.M, s2 / c.M, (d["gamma"] * d["save"][..., 1]).expand_as(s1)], -1)
        res["consts_abs"] = torch.stack([a1 / c.M, a2 / c.M], -1)
        res["g_beta"], res["g_gamma"] = d["g_beta0"] + s1.sum(0), d["g_gamma0"] + s2.sum(0)
        res["g_beta_abs"], res["g_gamma_abs"] = d["g_beta0"].abs() + a1.sum(0), d["g_gamma0"].abs() + a2.sum(0)
    return res


def bnb_raw_sums(c):
    """raw = 1: what a consumer's fused kernel left in the replicas, [S, NREP, 2 C] fp64: the fp64 sums split over the replicas."""
    ref = reference(c)["red"]                                           # [S, 2, C]
    w = torch.rand(NREP, 1, generator=torch.Generator().manual_seed(c.C), dtype=torch.float64)
    w = w / w.sum()
    flat = ref.permute(0, 2, 1).reshape(c.slots, 1, 2 * c.C)            # channel c at [2 c], [2 c + 1]
    return flat * w


# ==== embed_fpn linear =================================================================================================================
def _ef_cases(mfma):
    mk = lambda n, K, Co, KS, **o: _case("ef", N=n, K=K, C=Co, KS=KS, **o)
    if mfma:
        # (K, KS): 200 / 2 -> slices of 100, off a multiple of 64; 40 / 4 -> slices of 12, short; 36 / 4 -> slices of 12, the fourth empty
        cases = [mk(3, K, 48, KS) for K, KS in ((200, 2), (40, 4), (36, 4))]
        cases += [mk(n, 200, 48, 2) for n in (1, 65)] + [mk(3, 200, Co, 2) for Co in (16, 64, 112)] + [mk(65, 36, 112, 4)]
        cases += [mk(3, 200, 48, 2, skip=1), mk(3, 200, 48, 2, skip=2)]
    else:
        # (K, KS): 37 / 3 -> slices of 13, 13, 11; 200 / 2; 5 / 4 -> slices of 2, 2, 1 and an empty one
        cases = [mk(3, K, Co, KS) for Co in (24, 40) for K, KS in ((37, 3), (200, 2), (5, 4))] + [mk(1, 37, 24, 3), mk(65, 37, 40, 3)]
        cases += [mk(3, 37, 24, 3, skip=1), mk(3, 37, 24, 3, skip=2)]
    return cases


def ef_kper(c):
    """K indices per slice: the MFMA form rounds it up to whole quads."""
    kper = -(-c.K // c.KS)
    return (kper + 3) // 4 * 4 if c.C % 16 == 0 and c.K % 4 == 0 else kper


@functools.lru_cache(maxsize=None)
def _ef_inputs(n, K, Co):
    g = torch.Generator().manual_seed((n * 4096 + K) * 256 + Co)
    return dict(e=torch.randn(n, K, generator=g).clamp_min(0.0), wt=torch.randn(K, Co, generator=g) / K ** 0.5)      # e: a ReLU output


def _compute_ef(c, dtype, mutant):
    """"part" [N, KS, Co] and "part_abs", the sums of the absolute terms.  Mutant "empty_unwritten": an empty slice keeps the canary."""
    d = {k: v.to(dtype) for k, v in inputs(c).items()}
    kper = ef_kper(c)
    part, part_abs = torch.zeros(c.N, c.KS, c.C, dtype=dtype), torch.zeros(c.N, c.KS, c.C, dtype=dtype)
    for ks in range(c.KS):
        kb, ke = min(c.K, ks * kper), min(c.K, (ks + 1) * kper)
        if ke > kb:
            terms = d["e"][:, kb:ke, None] * d["wt"][None, kb:ke, :]      # [N, k, Co]
            part[:, ks] = terms.cumsum(1)[:, -1] if dtype == torch.float32 else terms.sum(1)
            part_abs[:, ks] = terms.abs().sum(1)
        elif mutant == "empty_unwritten":
            part[:, ks] = CANARY
    return dict(part=part, part_abs=part_abs)


def ef_distance(got, ref):
    """Worst |delta| per (agent, slice, output) over the sum of |terms|; an empty slice must hold exact zeros."""
    delta, scale = (got.double() - ref["part"].double()).abs(), ref["part_abs"].double()
    if bool((delta[scale == 0] != 0).any()):
        return math.inf
    return (delta[scale > 0] / scale[scale > 0]).max().item() if bool((scale > 0).any()) else 0.0


# ==== the case table ===================================================================================================================
# kernel name -> its cases.  The names are those of kernels_conv.hip and kernels_bwd.hip.
KERNELS = collections.OrderedDict()
for _ot, _odt in (("float", 0), ("bf16_t", 1)):
    for _vec in (True, False):
        for _st, _src in (("float", 0), ("uint8_t", 1)):
            KERNELS[f"stem_mfma_kernel<{_ot}, {str(_vec).lower()}, {_st}>"] = _stem_cases(_odt, _vec, _src)
for _vec in (True, False):
    for _st, _src in (("float", 0), ("uint8_t", 1)):
        KERNELS[f"stem_bwd_weight_kernel<{str(_vec).lower()}, {_st}>, wpart_reduce_kernel"] = _stem_cases(0, _vec, _src, bwd=True)
KERNELS["spp4_kernel<4>"] = _spp_cases("spp", 1)
KERNELS["spp_kernel<float>"] = _spp_cases("spp", 2)
KERNELS["spp_kernel<bf16_t>"] = _spp_cases("spp", 2, dtype=1)
KERNELS["spp4_bwd_kernel<4>"] = _spp_cases("sppb", 1)
KERNELS["spp_bwd_kernel"] = _spp_cases("sppb", 2)
KERNELS["upsample_kernel<float>"] = _up_cases("up")
KERNELS["upsample_kernel<bf16_t>"] = _up_cases("up", dtype=1)
KERNELS["upsample_bwd_kernel"] = _up_cases("upb")
KERNELS["addact_kernel<float>"] = _up_cases("add")
KERNELS["addact_kernel<bf16_t>"] = _up_cases("add", dtype=1)
KERNELS["bn_finalize_kernel"] = _bnf_cases()
KERNELS["bn_finalize_all_kernel"] = [_case("bnall"), _case("bnall", skip=1), _case("bnall", skip=2)]
KERNELS["bn_bwd_reduce_kernel, bn_bwd_consts_kernel"] = _bnb_cases()
KERNELS["efpn_linear_mfma_kernel"] = _ef_cases(True)
KERNELS["efpn_linear_kernel"] = _ef_cases(False)

ALL_CASES = [c for cases in KERNELS.values() for c in cases]


def inputs(c):
    """The case's dense tensors; shared by all routes and options of a shape.  Do not modify."""
    if c.kind in ("stem", "stemw"):
        return _stem_inputs(c.P, c.cout, c.pos, c.slots, c.kind == "stemw")
    if c.kind in ("spp", "sppb"):
        return _spp_inputs(c.H, c.W, c.C, c.slots)
    if c.kind in ("up", "upb", "add"):
        return _up_inputs(c.kind, c.H, c.W, c.C, c.dtype if c.kind == "add" else 0, c.slots, c.ints, c.M if c.kind == "add" else 0)
    if c.kind == "bnf":
        return _bnf_inputs(c.C, c.M)
    if c.kind == "bnall":
        return _bnall_inputs()
    if c.kind == "bnb":
        return _bnb_inputs(c.C, c.M, c.slots, c.raw)
    return _ef_inputs(c.N, c.K, c.C)


def compute(c, dtype=torch.float64, mutant=None):
    """The case's results in `dtype` arithmetic, a dict (see the _compute_* of the family)."""
    if c.kind in ("stem", "stemw"):
        return _compute_stem(c, dtype, mutant)
    if c.kind in ("spp", "sppb"):
        return _compute_spp(c, dtype, mutant)
    if c.kind in ("up", "upb", "add"):
        return _compute_up(c, dtype, mutant)
    if c.kind in ("bnf", "bnall"):
        return _compute_bnf(c, dtype, mutant)
    if c.kind == "bnb":
        return _compute_bnb(c, dtype, mutant)
    return _compute_ef(c, dtype, mutant)


def _key(c):
    """The case without what does not change its results."""
    k = c._replace(route=0, skip=0, nrep=NREP, max_wg=0, src=0, align=0, t1=0, save=0, run=0)
    return k._replace(dtype=0) if c.kind not in ("add", "spp") else k


@functools.lru_cache(maxsize=None)
def _reference(key):
    return compute(key)


def reference(c):
    """fp64, computed once per distinct computation; shared by the routes and options.  Do not modify."""
    return _reference(_key(c))


# ---- distances -----------------------------------------------------------------------------------------------------------
def red_distance(got, ref):
    """Worst |delta| per slot, moment and channel over that channel's sum of |terms|."""
    return ((got.double() - ref["red"]).abs() / ref["red_abs"]).max().item()


def consts_distances(got, ref):
    """(c1 and c2 and the two parameter gradients: worst |delta| over the sum of |terms|; k: worst relative distance)."""
    cs = got["consts"].double()
    scale = ref["consts_abs"]
    d12 = (cs[..., :2] - ref["consts"][..., :2]).abs()
    worst = 0.0 if not bool((scale > 0).any()) else (d12[scale > 0] / scale[scale > 0]).max().item()
    if bool((d12[scale == 0] != 0).any()):
        worst = math.inf
    for k in ("g_beta", "g_gamma"):
        worst = max(worst, ((got[k].double() - ref[k]).abs() / ref[k + "_abs"]).max().item())
    kk = ref["consts"][..., 2]
    dk = (cs[..., 2] - kk).abs()
    krel = (dk / kk.abs().clamp_min(1e-30)).max().item() if bool((dk != 0).any()) else 0.0
    return worst, krel


def over_bars(c, got, ref, margin=1.0):
    """[] when every result of `got` is within the case's bars divided by `margin`, else the offending (name, distance, bar)
    triples.  `got` and `ref` are dicts as compute returns them.  (The exact comparisons — raw SPP channels, the SPP backward, the
    upsample copies, integer gradients — are the callers': they have no margin.)"""
    bad = []

    def out_bars(g, r, name=""):
        l2, mx = distances(g, r)
        bl2, bmx, babs = (BF16_L2, BF16_MAX, BF16_ABS) if c.dtype else (OUT_L2, OUT_MAX, 0.0)
        scale = r.abs().max().item()
        if not l2 * margin <= bl2:
            bad.append((name + "relative L2", l2, bl2))
        if not mx * margin <= bmx + babs / scale:
            bad.append((name + "max-norm / max|ref|", mx, bmx + babs / scale))
    if "out" in ref:
        out_bars(got["out"], ref["out"])
    if "pooled" in ref:
        out_bars(got["pooled"], ref["pooled"], "pooled ")
    if "stats" in ref and "stats" in got:
        st = stats_over_bar(got["stats"], ref["stats"], N * (c.P // 2) ** 2)
        if not st * margin <= 1.0:
            bad.append(("statistics / their bar", st, 1.0))
    if "dw" in ref:
        dmx = distances(got["dw"], ref["dw"])[1]
        if not dmx * margin <= DW_MAX:
            bad.append(("dW max-norm / max|ref|", dmx, DW_MAX))
    if "red" in ref and "red" in got:
        rd = red_distance(got["red"], ref)
        if not rd * margin <= RED_BAR:
            bad.append(("sums / sum |terms|", rd, RED_BAR))
    if "consts" in ref and "consts" in got:
        cd, kd = consts_distances(got, ref)
        if not cd * margin <= RED_BAR:
            bad.append(("consts and parameter gradients / sum |terms|", cd, RED_BAR))
        if not kd <= K_RTOL:
            bad.append(("k = gamma invstd, relative", kd, K_RTOL))
    if "part" in ref:
        ed = ef_distance(got["part"], ref)
        if not ed * margin <= EF_BAR:
            bad.append(("partial sums / sum |terms|", ed, EF_BAR))
    if "bn" in ref:
        bd = bn_distance(got["bn"], ref["bn"], ref["terms"])
        if not bd * margin <= BN_BAR:
            bad.append(("BatchNorm values / sum |terms|", bd, BN_BAR))
    if "layers" in ref:
        for i, (g, r, t) in enumerate(zip(got["layers"], ref["layers"], ref["terms"])):
            if r is not None:
                bd = bn_distance(g, r, t)
                if not bd * margin <= BN_BAR:
                    bad.append((f"BatchNorm values of layer {i} / sum |terms|", bd, BN_BAR))
    return bad
