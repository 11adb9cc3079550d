"""Cases, inputs, fp64 reference and bars for the 1x1 (pointwise) conv kernels (csrc/kernels_conv.hip: pw_mfma_kernel,
pw_narrow_kernel; csrc/kernels_pwres.hip: pw_dir_kernel; csrc/kernels_pwxs.hip: pw_xs_kernel, pw_x3_kernel and the three weight
splitters; csrc/kernels_bwd_pw.hip: pw_bwd_weight_kernel, pw_bwd_weight_wide_kernel), one kernel at a time through the context-free
entries jn_pw / jn_pw_bwd_data_x3 / jn_pw_bwd_weight (include/jnroll.h).

Shared by tests/test_pw_cases_cpu.py (every case is admissible, the MFMA cases reach every tile variant, the bars mean something on
these inputs and bite on the mistakes a kernel can make) and tests/test_gpu_pw_kernels.py (every kernel against the reference).
Fixed seeds, no committed tensors.

A case is (kind, route, M, cin, cout, dt, transposed, identity, accumulate, bias, act, stats, nrep, skip, slots, up, defer, max_wg,
wt_big, use_wpart, exact):
 - kind "pw": jn_pw; "bdx3": jn_pw_bwd_data_x3; "bw": jn_pw_bwd_weight.  (cin, cout) are the ENTRY's for "pw" (transposed: cin is
   the contracted dimension, w is [cin][cout]) and the forward LAYER's for "bdx3" and "bw" (w and gw are [cout][cin]);
 - route: the forced route of jn_pw: 1 = X1, 2 = X3, 3 = XS, 4 = WIDE, 5 = NARROW, 6 = MFMA;
 - M pixels.  The kernels see N * H * W only, so a plain case is N = 2 images of 1 x M / 2 pixels (one image where M is odd); the
   fused-upsample cases (up = 1), the only kernels that read H and W, are 2 images of 5 x 7;
 - dt: 0 = f32 maps, fp32 matrix pipe; 1 = f32 maps, bf16 pipe (the gradients of bf16 mode); 2 = bf16 -> bf16; 3 = bf16 -> f32;
 - skip: 0 = no flag, 1 = a flag below skip_when (the launch runs), 2 = a flag at skip_when (nothing may change);
 - defer: 0 = plain table, 1 = deferred BatchNorm entries as channel runs, 2 = as per-channel arrays;
 - wt_big: the launch runs under JN_PW_WT_SMALL_M=0 (the 128-pixel data-gradient variant on a small map).

Pixel counts: the smallest with an edge of the kernel's own pixel tile BM (pw_mfma 32 WM; pw_narrow 64, 128 with one channel
tile; pw_xs / pw_x3 16 PT; pw_dir 16 per wave, four waves): M = 5, BM + 5 (a tile and a partial one), with max_wg = 1 and 2 a
count that gives every workgroup (every wave of pw_dir) three tiles, the last partial; for nrep = 8 ten workgroups (more than the
replicas); M = 16400 where the forward variant of pw_mfma is chosen by the pixel count (JN_PW_TINY_M = 16384).

Not in the list, and why: pw_dir_kernel<8, ..> (launch_pw_dir's ctw = 8) is never launched: launch_pw and tools/pwxsbench.hip pass
ctw = 0 and pw_dir_auto_ctw returns 4 or 2.  pw_x3_kernel's flat-order (FRAG = false) forward forms exist only under
JN_X3_ALL_SHAPES (tools/pwxsbench.hip): every shape of pw_xs_shape is a shape of pw_x3_fragment_order, so a network's planes are
always read in fragment order; w_split3_kernel (flat) still runs in every X1 / X3 case, as the first of the context's two splitter
launches, and its planes are what w_split3_frag_kernel overwrites.  pw_mfma_kernel<2, .., false, 4, ..> is dead code the old
dispatch instantiated and the selection function cannot return.  The RED / RED2 forms of the fused backward are not reachable
through jn_pw_bwd_fused (tests/test_gpu_pw_bwd_fused128.py covers the others)."""
import collections
import contextlib
import functools
import os

import torch

from tests.conv3_cases import (BF16_ABS, BF16_L2, BF16_MAX, CANARY, CANARY_BF16, DW_EXACT_L2, DW_MAX, DW_ORDER, NREP, OUT_L2,      # noqa: F401
                               OUT_MAX, SKIP_WHEN, SPLIT_VS_F32, STAT_ATOL, STAT_RTOL, X3_W, X3_X, distances, padded, split3,
                               stats_over_bar, transform)
from tests.kernel_helpers import _bf16

Case = collections.namedtuple("Case", "kind route M cin cout dt transposed identity accumulate bias act stats nrep skip slots up defer "
                                      "max_wg wt_big use_wpart exact")

X1, X3, XS, WIDE, NARROW, MFMA = 1, 2, 3, 4, 5, 6
IN_PAD, OUT_PAD = 8, 4      # read-side leading dimensions C + 8, written-side C + 4
ROW_PAD = 3                 # rows past M in every map, canary
WPART_MAX = 16384           # JN_WPART_MAX
NREP_DEFER = 8              # JN_NREP_DEFER: replicas of a deferred layer's batch sums
TINY_M, WT_SMALL_M = 16384, 65536      # JN_PW_TINY_M, JN_PW_WT_SMALL_M
UP_HW = (5, 7)
STAT_ORDER = 1e-5           # two runs of fp64 statistics fed from fp32 partial sums: within this of the largest element
DEFER_DN, DEFER_DMAX = 2, 65536
# ---- the bars: those of conv3_cases.py (imported above), and one of this unit ------------------------------------------------
# fp32 maps on the bf16 pipe (dt 1 and 3: both operands rounded to bf16, fp32 sums, fp32 output): the borrowed max-norm bar 5e-3
# max|ref| + 1e-4 does not hold with 2x to spare for plain bf16 arithmetic on outputs of order 1, and small outputs would flatten the
# sigmoid epilogue of dt 3 to a constant.  The CPU emulation of that arithmetic, measured against fp64 on the cases of this file
# (test_pw_cases_cpu.py prints it; worst: 48 -> 24 channels transposed, M = 5):
BF16_PIPE_MEASURED = 4.5e-3      # max |delta| / max |ref|
BF16_PIPE_MAX = 9e-3             # 2 x the above: the margin the earlier pins give bf16 storage.  (The relative-L2 bar stays BF16_L2.)


def _case(kind, route, M, cin, cout, **o):
    d = dict(dt=0, transposed=0, identity=0, accumulate=0, bias=0, act=0, stats=0, nrep=NREP, skip=0, slots=1, up=0, defer=0, max_wg=0,
             wt_big=0, use_wpart=0, exact=0)
    d.update(o)
    return Case(kind, route, M, cin, cout, **d)


def images(c):
    """(N, H, W) of the case's launch."""
    if c.up:
        return 2, UP_HW[0], UP_HW[1]
    return (2, 1, c.M // 2) if c.M % 2 == 0 else (1, 1, c.M)


ENTRY_TYPES = {0: (0, 0, 0), 1: (0, 0, 1), 2: (1, 1, 1), 3: (1, 0, 1)}      # dt -> (dtype_in, dtype_out, bf16_mfma) of jn_pw


def route_args(c, route):
    """The arguments of jn_pw_route for the case's launch (all but variant_out)."""
    n, h, w = images(c)
    di, do, bf = ENTRY_TYPES[c.dt]
    return [n, h, w, c.cin, c.cout, c.cin + IN_PAD, c.cout + OUT_PAD, di, do, bf, c.transposed, c.accumulate, c.bias, c.act, c.slots, c.up, route]


@contextlib.contextmanager
def launch_env(c):
    """The environment of the case's launch: wt_big sets the hook that jn_pw_route and the launcher read per call."""
    old = os.environ.get("JN_PW_WT_SMALL_M")
    if c.wt_big:
        os.environ["JN_PW_WT_SMALL_M"] = "0"
    try:
        yield
    finally:
        if c.wt_big:
            if old is None:
                del os.environ["JN_PW_WT_SMALL_M"]
            else:
                os.environ["JN_PW_WT_SMALL_M"] = old


def defer_struct(c, sums_ptr, params_ptr, rep_stride, use_runs):
    """jn_pw's descriptor of the case's deferred input view (jolineedle_amd._lib.JnPwDefer) over the given device buffers."""
    from jolineedle_amd._lib import JnPwDefer, JnPwRun
    runs = defer_runs(c.cin)
    d = JnPwDefer(sums_ptr, rep_stride, params_ptr, DEFER_DN, DEFER_DMAX, len(runs), use_runs)
    for i, r in enumerate(runs):
        d.run[i] = JnPwRun(*r)
    return d


# ---- pw_mfma_kernel: the selection restated (pw_mfma_variant, kernels_conv.hip); test_pw_cases_cpu.py holds it to jn_pw_route ------
def mfma_variant(c):
    """(CT, KC, WM) of the case's launch on route MFMA."""
    nt = (c.cout + 15) // 16
    ct = nt if nt <= 3 else 4 if (nt == 4 or (nt % 8 != 0 and nt % 4 == 0)) else 8
    mtot = c.M * c.slots
    if c.transposed:
        wm = 2 if ct % 2 == 0 and mtot <= (0 if c.wt_big else WT_SMALL_M) else 4
    else:
        wm = 1 if ct % 4 == 0 and mtot <= TINY_M and c.cin <= 128 else 2 if ct % 2 == 0 else 4
    bf = c.dt != 0
    kc = 64 if bf else 32 if ct > 4 else 64
    if not bf and ct <= 4:
        if wm >= 2 and c.cin <= 16:
            kc = 16
        elif c.cin <= 32:
            kc = 32
    return ct, kc, wm


_TYPES = {0: ("float", "float", "false"), 1: ("float", "float", "true"), 2: ("bf16_t", "bf16_t", "true"), 3: ("bf16_t", "float", "true")}


def mfma_name(c):
    ct, kc, wm = mfma_variant(c)
    it, ot, bf = _TYPES[c.dt]
    return f"pw_mfma_kernel<{ct}, {kc}, {'true' if c.transposed else 'false'}, {wm}, {it}, {ot}, {bf}>"


# (cin, cout): the issue's eight, then one per remaining (CT, KC) of the fp32 pipe.  K = 24 is a partial 32-wide chunk, 48 a partial
# 64-wide one, 72 = two chunks of 32 and a quarter, 160 two and a half of 64; cout = 24, 40, 80, 136 end in a partial channel tile;
# 40 and 48 are CT = 3; 80 (five tiles) goes to CT = 8, 192 (twelve) to CT = 4
MFMA_PAIRS = ((16, 16), (24, 40), (48, 48), (32, 24), (64, 64), (96, 80), (72, 136), (160, 192),
              (32, 16), (40, 16), (16, 24), (48, 24), (16, 40), (32, 64), (16, 64), (160, 80))
MFMA_BIG_M = ((16, 64), (32, 64), (64, 64), (96, 80))      # CT % 4 == 0 with cin <= 128: the 64-pixel forward variant needs M > 16384
BF_WT_PAIRS = ((16, 16), (48, 48), (48, 24), (160, 192), (96, 80))      # K = 16 (padded to 32), 48 (chunk_q4 pads to 64) and 160
BF_FWD_PAIRS = ((16, 16), (48, 24), (48, 48), (48, 64), (160, 192), (96, 80), (160, 80))

KERNELS = collections.OrderedDict()      # kernel name -> its cases


def _add(name, c):
    KERNELS.setdefault(name, []).append(c)


def _edges(bm):
    return 5, bm + 5


def _mfma_cases():
    def add(cin, cout, **o):
        probe = _case("pw", MFMA, 5, cin, cout, **o)
        bm = 32 * mfma_variant(probe)[2]
        for M in _edges(bm):
            c = probe._replace(M=M)
            _add(mfma_name(c), c)
        return probe._replace(M=bm + 5), bm
    for cin, cout in MFMA_PAIRS:
        add(cin, cout, stats=1)
        for big in ((0, 1) if mfma_variant(_case("pw", MFMA, 5, cin, cout, transposed=1))[0] % 2 == 0 else (0,)):
            add(cin, cout, transposed=1, wt_big=big)
    for cin, cout in MFMA_BIG_M:
        c = _case("pw", MFMA, TINY_M + 16, cin, cout, stats=1, nrep=8)
        _add(mfma_name(c), c)
    for cin, cout in BF_WT_PAIRS:
        for big in ((0, 1) if mfma_variant(_case("pw", MFMA, 5, cin, cout, dt=1, transposed=1))[0] % 2 == 0 else (0,)):
            add(cin, cout, dt=1, transposed=1, wt_big=big)
    for cin, cout in BF_FWD_PAIRS:
        add(cin, cout, dt=2)
        add(cin, cout, dt=3, bias=1, act=1)
    for act in (0, 2, 3):
        add(48, 24, dt=3, bias=1, act=act)
    # the options, each once per direction on a two-tile shape (and on the partial channel tile of cout = 40 for the statistics)
    for cin, cout, o in ((32, 24, {}), (24, 40, {}), (64, 64, {}), (32, 24, dict(transposed=1)), (64, 64, dict(transposed=1, wt_big=1))):
        two, bm = add(cin, cout, **o)
        opts = [dict(accumulate=1), dict(stats=1, nrep=NREP), dict(stats=1, accumulate=1), dict(stats=1, skip=1), dict(stats=1, skip=2), dict(slots=3),
                dict(slots=3, accumulate=1, stats=1), dict(bias=1, act=2), dict(bias=1, act=1, accumulate=1)]
        if not o:
            opts += [dict(defer=1), dict(defer=2)]
        for opt in opts:
            c = two._replace(**opt)
            _add(mfma_name(c), c)
        c = two._replace(M=9 * bm + 5, stats=1, nrep=8)
        _add(mfma_name(c), c)


def _persistent(name, route, cin, cout, bm, options, tiles_per_wg=3, wg_tiles=1, **fixed):
    """The edges of a persistent kernel: M = 5, a tile and a partial one, and with max_wg = 1 and 2 three tiles per workgroup (wg_tiles
    tiles side by side in one: pw_dir's four waves), the last partial; then one case per option on the two-tile shape."""
    for M in _edges(bm * wg_tiles):
        _add(name, _case("pw", route, M, cin, cout, **fixed))
    for wg in (1, 2):
        _add(name, _case("pw", route, (tiles_per_wg * wg * wg_tiles - 1) * bm + 5, cin, cout, max_wg=wg, **dict(fixed, **({} if "stats" in fixed or fixed.get("dt") else dict(stats=1)))))
    for o in options:
        M = 9 * bm * wg_tiles + 5 if o.get("nrep") == 8 else bm * wg_tiles + 5
        _add(name, _case("pw", route, M, cin, cout, **dict(fixed, **o)))


_STAT_OPTS = (dict(stats=1), dict(stats=1, nrep=8), dict(stats=1, skip=1), dict(stats=1, skip=2))
_DEFER_OPTS = (dict(defer=1), dict(defer=2), dict(defer=1, stats=1, nrep=8))
PWN_TABLE = ((1, 16), (2, 16), (2, 32), (4, 32), (4, 64), (8, 64))      # JN_PWN_TABLE: (channel tiles, K)
XS_SHAPES = {(64, 64): (4, 2, 2), (64, 128): (4, 2, 2), (128, 64): (8, 2, 4), (128, 128): (8, 2, 4), (128, 256): (2, 2, 2), (256, 128): (4, 2, 2),
             (256, 256): (2, 4, 2), (512, 256): (2, 2, 2)}      # pw_xs_shape: (K, N) -> (D of pw_xs, PT of pw_x3, D of pw_x3) at the default tiling
X1_TILES = {(64, 64): (2, 2), (64, 128): (2, 2), (128, 64): (2, 4), (128, 128): (2, 4), (128, 256): (2, 4), (256, 128): (4, 2), (256, 256): (4, 2),
            (512, 256): (4, 2)}      # launch_pw_x1: (PT, D)


def _build():
    _mfma_cases()
    # pw_narrow_kernel: the six shapes of the table, and the partial last channel tile of CT = 2 and CT = 8
    for ct, k in PWN_TABLE:
        couts = (16 * ct,) + ((24,) if (ct, k) == (2, 16) else (120,) if (ct, k) == (8, 64) else ())
        for cout in couts:
            _persistent(f"pw_narrow_kernel<{ct}, {k}>", NARROW, k, cout, 64 if ct % 2 == 0 else 128, _STAT_OPTS + _DEFER_OPTS if cout == 16 * ct else ())
    # pw_xs_kernel / pw_x3_kernel / its single-plane bf16 form: every shape at the launcher's default tiling
    for (K, Nc), (d_xs, pt3, d3) in XS_SHAPES.items():
        ctw = Nc // 64
        pt = 4 if K == 512 or (K == 64 and ctw == 2) else 2
        light = (K, Nc) not in ((128, 128), (64, 128), (512, 256))      # every option on three shapes (64 -> 128: the statistics pass through Xs)
        _persistent(f"pw_xs_kernel<{K}, {ctw}, {pt}, {d_xs}>", XS, K, Nc, 16 * pt, _STAT_OPTS[:1] if light else _STAT_OPTS + _DEFER_OPTS)
        _persistent(f"pw_x3_kernel<{K}, {ctw}, {pt3}, {d3}, 3, float>", X3, K, Nc, 16 * pt3, _STAT_OPTS[:1] if light else _STAT_OPTS + _DEFER_OPTS)
        p1, d1 = X1_TILES[(K, Nc)]
        _persistent(f"pw_x3_kernel<{K}, {ctw}, {p1}, {d1}, 1, bf16_t>", X1, K, Nc, 16 * p1, (dict(skip=1), dict(skip=2)) if light else
                    (dict(skip=1), dict(skip=2), dict(stats=1), dict(stats=1, nrep=8)), dt=2)
    for name, route, K, Nc in (("pw_xs_kernel<256, 2, 2, 4, true>", XS, 256, 128), ("pw_x3_kernel<128, 1, 2, 4, 3, float, true>", X3, 128, 64),
                               ("pw_x3_kernel<256, 2, 2, 2, 3, float, true>", X3, 256, 128)):
        for o in ({}, dict(stats=1), dict(max_wg=1, stats=1), dict(stats=1, skip=2), dict(defer=1)):
            _add(name, _case("pw", route, 2 * UP_HW[0] * UP_HW[1], K, Nc, up=1, **o))
    # pw_dir_kernel<CTW, WT, PF, ST, TF>: 64-channel slices (32 from K = 320 up); cout = 96: the second slice half empty, 68: four
    # live channels in it
    fwd_opts = _STAT_OPTS + _DEFER_OPTS + (dict(accumulate=1, stats=1), dict(slots=3, stats=1), dict(slots=3, accumulate=1))
    for (K, Nc), opts in (((64, 64), fwd_opts), ((128, 96), _STAT_OPTS[:2]), ((192, 64), ()), ((256, 68), _STAT_OPTS[:2])):
        _persistent("pw_dir_kernel<4, false, 2, true, true>", WIDE, K, Nc, 16, opts, wg_tiles=4)
    for (K, Nc), opts in (((512, 256), _STAT_OPTS[:2] + _DEFER_OPTS[:2]), ((320, 128), (dict(slots=3, stats=1),))):
        _persistent("pw_dir_kernel<2, false, 2, true, true>", WIDE, K, Nc, 16, opts, wg_tiles=4)
    grad_opts = (dict(accumulate=1), dict(slots=3), dict(slots=3, accumulate=1), dict(skip=1), dict(skip=2))
    for ctw, pairs in ((4, ((64, 64), (128, 96), (256, 68))), (2, ((512, 256), (320, 128)))):
        for i, (K, Nc) in enumerate(pairs):
            _persistent(f"pw_dir_kernel<{ctw}, true, 4, false, true>", WIDE, K, Nc, 16, grad_opts if i == 0 else (), wg_tiles=4, transposed=1, stats=0)
            _persistent(f"pw_dir_kernel<{ctw}, true, 4, false, false>", WIDE, K, Nc, 16, grad_opts if i == 0 else (), wg_tiles=4, transposed=1, identity=1,
                        stats=0)
            _persistent(f"pw_dir_kernel<{ctw}, true, 2, true, true>", WIDE, K, Nc, 16, _STAT_OPTS[1:] + (dict(stats=1, slots=3, accumulate=1),) if i == 0 else (),
                        wg_tiles=4, transposed=1, stats=1)
    # launch_pw_x3_bwd_data (w_split3_t_kernel + pw_x3_kernel<.., SLOTS>): the four shapes, one and three slots; 512 input channels: two
    # column halves
    for (co, ci), name in (((256, 128), "pw_x3_kernel<256, 2, 2, 2, 3, float, false, true>"), ((128, 256), "pw_x3_kernel<128, 4, 2, 4, 3, float, false, true>"),
                           ((256, 256), "pw_x3_kernel<256, 4, 2, 2, 3, float, false, true>"), ((256, 512), "pw_x3_kernel<256, 4, 2, 2, 3, float, false, true>")):
        for slots in (1, 3):
            for M, wg in ((5, 0), (37, 0), (69, 1), (32 * 5 + 5, 2)):      # (three slots: a workgroup's walk crosses the slot boundary)
                _add("w_split3_t_kernel, " + name, _case("bdx3", 0, M, ci, co, slots=slots, max_wg=wg))
    # pw_bwd_weight_kernel<CTN, CTK>: 16, 24, 40, 64 channels are 1, 2, 3, 4 tiles of 16, the second of 24 and the third of 40 partial;
    # (80, 72): two 64-channel blocks each way, the second partial.  M = 5, 65 (a second row chunk of one row), 200 (four chunks)
    chans = (16, 24, 40, 64)
    for cn, cout in enumerate(chans, 1):
        for ck, cin in enumerate(chans, 1):
            for M in (5, 65, 200):
                for slots in (1, 3):
                    for wp in (0, 1):
                        _add(f"pw_bwd_weight_kernel<{cn}, {ck}>", _case("bw", 0, M, cin, cout, slots=slots, use_wpart=wp))
    for M in (5, 65, 200):
        for slots in (1, 3):
            for wp in (0, 1):
                _add("pw_bwd_weight_kernel<4, 4>", _case("bw", 0, M, 72, 80, slots=slots, use_wpart=wp))
    # pw_bwd_weight_wide_kernel<SP>: one 128 x 128 block; (192, 136): two blocks each way, 64 and 8 live channels in the second; M = 300:
    # two row chunks of 256
    for exact in (0, 1):
        for cout, cin in ((128, 128), (192, 136)):
            for slots in (1, 3):
                _add(f"pw_bwd_weight_wide_kernel<{'false' if exact else 'true'}>", _case("bw", 0, 300, cin, cout, slots=slots, exact=exact))


_build()
ALL_CASES = [c for cases in KERNELS.values() for c in cases]


def is_split(c):
    """Products on the bf16 pipe from split fp32 operands: compared with the fp32 route on the same inputs as well."""
    return c.kind == "bdx3" or (c.kind == "pw" and c.route == X3)


def is_bf16(c):
    return c.kind == "pw" and c.dt != 0


def f32_twin(c):
    """The case on the fp32 pipe, for the split routes: XS for X3, the transposed WIDE launch for the split data gradient."""
    if c.kind == "bdx3":      # the gradient conv: contracted over the layer's cout, w [cout][cin] read transposed
        return _case("pw", WIDE, c.M, c.cout, c.cin, transposed=1, identity=1, slots=c.slots)
    return c._replace(route=XS, up=0)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _table(g, S, C, identity=False):
    """[S, 3, C]: scales in [0.5, 1.5]; shifts 0.5 randn; about a quarter of the channels is read raw (channel 1 always)."""
    t = torch.empty(S, 3, C)
    t[:, 0] = 0.5 + torch.rand(S, C, generator=g)
    t[:, 1] = 0.5 * torch.randn(S, C, generator=g)
    t[:, 2] = (torch.rand(S, C, generator=g) < 0.75).float()
    t[:, 2, 1] = 0.0
    if identity:
        t[:, 0], t[:, 1], t[:, 2] = 1.0, 0.0, 0.0
    return t


def defer_runs(cin):
    """The input view as a concat of four producers, a quarter of the channels each: (c0, c1, stat0, g0, b0, hw).  Two deferred layers
    with different maps, a plain one (stat0 < 0), and one above the deferral limit (DEFER_DN * hw > DEFER_DMAX: reads the table)."""
    q = cin // 4
    return ((0, q, 3, 5, 5 + cin, 49.0), (q, 2 * q, 3 + q + 2, 5 + q + 1, 5 + cin + q + 3, 196.0), (2 * q, 3 * q, -1, 0, 0, 196.0),
            (3 * q, cin, 3 + 2 * q + 4, 5 + 2 * q + 2, 5 + cin + 2 * q + 6, 40000.0))


def _defer_inputs(g, cin):
    """Batch sums [8][rep_stride] of a synthetic producer (fp64 sums of count = dN * hw values per stat channel, spread unevenly over
    the replicas), the parameter buffer, and a table whose deferred entries hold what must not be read."""
    n_stat = cin + 16
    rep_stride = 2 * n_stat + 6
    sums = torch.zeros(NREP_DEFER, rep_stride, dtype=torch.float64)
    for c0, c1, stat0, g0, b0, hw in defer_runs(cin):
        if stat0 < 0:
            continue
        count = int(DEFER_DN * min(hw, 400.0))      # (the run above the limit is never derived: its sums only have to be there)
        n = c1 - c0
        vals = (0.5 * torch.randn(n, generator=g, dtype=torch.float64))[:, None] + \
            (0.5 + torch.rand(n, generator=g, dtype=torch.float64))[:, None] * torch.randn(n, count, generator=g, dtype=torch.float64)
        s1, s2 = vals.sum(1), (vals * vals).sum(1)
        if hw == 49.0:      # one channel whose variance comes out below zero (E[x^2] - mean^2 of a near-constant channel): clamped
            s1[1] = 0.1 * count
            s2[1] = (0.01 - 5e-4) * count
        frac = torch.rand(NREP_DEFER, n, generator=g, dtype=torch.float64) ** 3
        frac = frac / frac.sum(0)
        sums[:, 2 * stat0:2 * (stat0 + n):2] = frac * s1
        sums[:, 2 * stat0 + 1:2 * (stat0 + n):2] = frac.flip(0) * s2
    params = torch.randn(5 + 2 * cin + 16, generator=g)
    params[:] = torch.where(params.abs() < 0.3, torch.full_like(params, 0.7), params)      # (a weight near 0 would hide its channel)
    params[defer_runs(cin)[0][3] + 1] = 0.03      # the clamped channel: 1 / sqrt(eps) = 31.6 times this is its scale
    return sums, params, rep_stride


def derived_table(c, d, dtype=torch.float64, mutant=None):
    """[3, cin]: the case's plain table with the deferred entries replaced by what the sums give: mean, variance (clamped at 0),
    eps = 1e-3, scale = gamma / sqrt(var + eps), shift = beta - mean * scale, flag 1."""
    tab = d["tab"][0].to(dtype).clone()
    sums = d["sums"].to(dtype)
    tot = sums[:7].sum(0) if mutant == "seven_replicas" else sums.sum(0)
    for c0, c1, stat0, g0, b0, hw in defer_runs(c.cin):
        over = DEFER_DN * hw > DEFER_DMAX
        if stat0 < 0 or (over and mutant != "over_limit_derived"):
            continue
        n, count = c1 - c0, DEFER_DN * hw
        mean = tot[2 * stat0:2 * (stat0 + n):2] / count
        var = tot[2 * stat0 + 1:2 * (stat0 + n):2] / count - mean * mean
        if mutant != "var_unclamped":
            var = var.clamp(min=0.0)
        sc = d["params"][g0:g0 + n].to(dtype) / torch.sqrt(var + 1e-3)
        tab[0, c0:c1], tab[1, c0:c1], tab[2, c0:c1] = sc, d["params"][b0:b0 + n].to(dtype) - mean * sc, 1.0
    return tab


@functools.lru_cache(maxsize=None)
def _inputs(kind, M, cin, cout, dt, transposed, identity, slots, defer):
    seed = (((("pw", "bdx3", "bw").index(kind) * 20000 + M) * 600 + cin) * 600 + cout) * 64 + dt * 16 + transposed * 8 + identity * 4 + slots
    g = torch.Generator().manual_seed(seed * 2 + (1 if defer else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    S = slots
    if kind == "bdx3":
        return dict(x=r(S, M, cout), w=r(cout, cin) / cout ** 0.5)
    if kind == "bw":
        return dict(gz=r(S, M, cout), x=r(S, M, cin), tab=_table(g, S, cin), prev=0.1 * r(cout, cin))
    # bf16 OUTPUT maps: rounding the output alone costs up to 3.9e-3 of max|ref|, which leaves the max-norm bar 5e-3 max|ref| + 1e-4 no
    # 2x margin on outputs of order 1 (conv3_cases.py, dw_cases.py): those cases have small weights and outputs of a few thousandths,
    # where the bar's absolute part is worth more than another 1e-2 of max|ref|.  The relative-L2 bar is scale-free.
    small = 1.0 / 512 if dt == 2 else 1.0
    d = dict(x=r(S, M, cin), tab=_table(g, S, cin, identity=bool(identity)), w=(r(cin, cout) if transposed else r(cout, cin)) / cin ** 0.5 * small,
             bias=0.3 * r(cout) * small, prev=r(S, M, cout) * small)
    if defer:
        d["sums"], d["params"], d["rep_stride"] = _defer_inputs(g, cin)
        for c0, c1, stat0, g0, b0, hw in defer_runs(cin):
            if stat0 >= 0 and DEFER_DN * hw <= DEFER_DMAX:
                d["tab"][0, 0, c0:c1], d["tab"][0, 1, c0:c1], d["tab"][0, 2, c0:c1] = 100.0, -50.0, 0.0
    return d


def inputs(c):
    """The case's dense fp32 tensors (slots first, channels last); shared by all routes and options of a shape.  Do not modify."""
    return _inputs(c.kind, c.M, c.cin, c.cout, c.dt if c.kind == "pw" else 0, c.transposed, c.identity, c.slots, 1 if c.defer else 0)


# ---- the reference: a plain restatement, fp64 by default ---------------------------------------------------------------
def activation(v, act):
    return v if act == 0 else v * torch.sigmoid(v) if act == 1 else torch.relu(v) if act == 2 else torch.sigmoid(v)


def activated(c, d, dtype, mutant=None):
    """T(x) of every slot, [S, M, cin]."""
    x = d["x"].to(dtype)
    outs = []
    for s in range(x.shape[0]):
        if c.defer:
            t = derived_table(c, d, dtype, mutant)
        else:
            t = d["tab"][0 if mutant == "slot_table" else s].to(dtype)
        if mutant == "flag_ignored":
            t = torch.stack([t[0], t[1], torch.ones_like(t[2])])
        if mutant == "table_ignored":
            t = torch.stack([t[0], t[1], torch.zeros_like(t[2])])
        outs.append(transform(x[s], t))
    return torch.stack(outs)


def products(c, a, w, mutant=None):
    """The matmul alone, linear in both operands (the split emulations call it per plane): "pw" a [S, M, cin] -> [S, M, cout]; "bdx3"
    g_z [S, M, cout] -> [S, M, cin]; "bw" (a [S, M, cin], g_z [S, M, cout]) -> [cout, cin]."""
    if c.kind == "bw":
        gz = w
        if mutant == "missing_slot":
            a, gz = a[:-1], gz[:-1]
        if mutant == "missing_row":      # the last row of the last row chunk
            a = a.clone()
            a[:, -1] = 0
        return torch.einsum("smn,smk->nk", gz, a)
    if c.kind == "bdx3":
        out = a @ w
        if mutant == "second_half_missing":
            out = out.clone()
            out[..., 256:] = 0
        return out
    if mutant == "drop_last_k_quad":
        a = a.clone()
        a[..., -4:] = 0
    wt = w if c.transposed else w.t()      # [cin, cout]
    if mutant == "untransposed":
        wt = wt.t()
    return a @ wt


def finish(c, d, z, dtype, mutant=None):
    """Bias, activation, accumulate, statistics: (out [S, M, cout], stats [2, cout] or None)."""
    if c.kind == "bw":
        return z + d["prev"].to(dtype), None
    if c.kind == "bdx3":
        return z, None
    if c.bias and mutant != "bias_after_act":
        z = z + d["bias"].to(dtype)
    out = activation(z, c.act)
    if c.bias and mutant == "bias_after_act":
        out = out + d["bias"].to(dtype)
    before = out
    if c.accumulate and mutant != "no_accumulate":
        out = out + d["prev"].to(dtype)
    if mutant == "drop_last_pixel":
        out = out.clone()
        out[:, -1] = 0
    if mutant == "tile_shift":
        out = torch.roll(out, 16, -1)
    st = before if mutant == "stats_before_accumulate" else out
    stats = torch.stack([st.sum((0, 1)), (st * st).sum((0, 1))]) if c.stats else None
    return out, stats


def compute(c, dtype=torch.float64, mutant=None):
    """The case's result in `dtype` arithmetic: (out, stats); out [S, M, cout] ("bdx3": the data gradient [S, M, cin]; "bw":
    gw [cout, cin], added to `prev`); stats = (sum, sum of squares) of out per channel over all slots and pixels, [2, cout]."""
    d = inputs(c)
    if c.kind == "bw":
        z = products(c, activated(c, d, dtype, mutant), d["gz"].to(dtype), mutant)
    elif c.kind == "bdx3":
        z = products(c, d["x"].to(dtype), d["w"].to(dtype), mutant)
    else:
        z = products(c, activated(c, d, dtype, mutant), d["w"].to(dtype), mutant)
    return finish(c, d, z, dtype, mutant)


def _key(c):
    """The case without what does not change its results."""
    return c._replace(route=0, skip=0, nrep=NREP, max_wg=0, wt_big=0, use_wpart=0, exact=0, defer=1 if c.defer else 0)


@functools.lru_cache(maxsize=None)
def _reference(key):
    return compute(key)


def reference(c):
    """fp64, computed once per distinct computation; shared by the routes and options.  Do not modify.  bf16 maps: from the inputs
    rounded to bf16, the expected output NOT rounded."""
    if c.kind == "pw" and c.dt >= 2:
        return compute_rounded_inputs(_key(c))
    return _reference(_key(c))


@functools.lru_cache(maxsize=None)
def compute_rounded_inputs(key):
    d = inputs(key)
    z = products(key, activated(key, dict(d, x=_bf16(d["x"])), torch.float64), d["w"].double())
    return finish(key, d, z, torch.float64)


# ---- emulations of the kernels' number formats (CPU) ---------------------------------------------------------------------
def compute_split(c, drop_hi_lo=False):
    """The split routes in fp32 arithmetic.  Outputs and data gradients: three bf16 planes per operand, the six products of jn_split.h
    summed in fp32, small ones first.  The wide weight gradient: two planes, h l + l h + h h.  drop_hi_lo: the mutant that forgets the
    product of one operand's high plane with the other's next plane (about 2^-9 of the sum)."""
    d = inputs(c)
    f32 = torch.float32
    if c.kind == "bw":
        a, g = activated(c, d, f32), d["gz"]
        ah, gh = _bf16(a), _bf16(g)
        al, gl = _bf16(a - ah), _bf16(g - gh)
        z = None
        for ap, gp in ((al, gh), (ah, gl), (ah, gh)):
            if drop_hi_lo and ap is al:
                continue
            p = products(c, ap, gp)
            z = p if z is None else z + p
        return finish(c, d, z, f32)
    a = d["x"] if c.kind == "bdx3" else activated(c, d, f32)
    xp, wp = split3(a), split3(d["w"])
    z = None
    for e in range(6):
        if drop_hi_lo and X3_W[e] == 0 and X3_X[e] == 1:
            continue
        p = products(c, xp[X3_X[e]], wp[X3_W[e]])
        z = p if z is None else z + p
    return finish(c, d, z, f32)


def compute_bf16(c):
    """The bf16 pipe: the transformed operand and the weight rounded to bf16, fp32 sums; bf16 input maps rounded before the
    transform, bf16 output maps after the epilogue.  The statistics are those of the fp32 values."""
    d = inputs(c)
    if c.dt >= 2:
        d = dict(d, x=_bf16(d["x"]))
    a = _bf16(activated(c, d, torch.float32))
    out, stats = finish(c, d, products(c, a, _bf16(d["w"])), torch.float32)
    return (_bf16(out) if c.dt == 2 else out), stats


def emulate(c):
    """The case in the arithmetic of its kernel."""
    if is_bf16(c):
        return compute_bf16(c)
    if is_split(c) or (c.kind == "bw" and c.cin >= 128 and c.cout >= 128 and not c.exact):
        return compute_split(c)
    return compute(c, torch.float32)


# ---- distances -----------------------------------------------------------------------------------------------------------
def pixels(c):
    return c.M * c.slots


def over_bars(c, got, ref, margin=1.0):
    """[] when (out, stats) `got` is within the case's bars divided by `margin`, else the offending (name, distance, bar) triples."""
    bad = []
    l2, mx = distances(got[0], ref[0])
    scale = ref[0].abs().max().item()
    if c.kind == "bw":
        bl2, bmx, babs = (DW_EXACT_L2 if c.exact else float("inf")), DW_MAX, 0.0
    elif is_bf16(c):
        bl2, bmx, babs = BF16_L2, (BF16_MAX if c.dt == 2 else BF16_PIPE_MAX), BF16_ABS
    else:
        bl2, bmx, babs = OUT_L2, OUT_MAX, 0.0
    if not l2 * margin <= bl2:
        bad.append(("relative L2", l2, bl2))
    if not mx * margin <= bmx + babs / scale:
        bad.append(("max-norm / max|ref|", mx, bmx + babs / scale))
    if ref[1] is not None:
        st = stats_over_bar(got[1], ref[1], pixels(c))
        if not st * margin <= 1.0:
            bad.append(("statistics / their bar", st, 1.0))
    return bad
