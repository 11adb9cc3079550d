"""The fused pointwise backward at 128 input channels (csrc/kernels_bwd_pw.hip: ``pw_bwd_fused128_kernel``, 32-pixel tiles, two
workgroups per CU, W^T streamed in fragment order) through the context-free entry ``jn_pw_bwd_fused``: against an fp64
restatement of the formulas in the kernel's header comment, and against the 64-pixel kernel (route 1) it replaces; and, against the
same fp64 restatement, every other shape the entry admits (pw_bwd_fused_kernel, cout and cin each 16, 32, 64 or 128).

Bars:
 - data gradient, route 0 against route 1: 64 output channels multiply on the fp32 matrix pipe in the same k order as the
   64-pixel kernel: the same bits.  128 output channels take the six-product bf16 form of the wide route: relative L2 < 2e-5,
   the bar of test_wide_data_gradient_on_the_bf16_pipe_matches_the_fp32_pipe;
 - data gradient against fp64: relative L2 < 2e-5 (the bar of test_wide_data_gradient_on_the_bf16_pipe_matches_the_fp32_pipe
   for a split-bf16 product form; fp32 products over 128 terms sit well inside it);
 - weight gradient against fp64: max |delta| / max |dW| < 1e-4, the leaf bar of
   test_split_weight_gradients_stay_close_to_fp32_mfma, for BOTH routes on the same inputs;
 - two runs of route 0: the data gradient bit for bit; the weight gradient bit for bit with one workgroup (every dW
   element then has one writer) and otherwise to the order of its fp32 atomics, max |delta| / max |dW| < 1e-5 (at most
   S * ceil(M / 32) <= 12 partial sums per element here, each reordering worth a few 2^-24 of the largest)."""
import itertools

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import ptr
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CIN = 128


def _inputs(cout, M, S, seed, cin=CIN):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g)
    C = cout + cin
    tab = torch.empty(S, 3, C)
    tab[:, 0] = u(0.5, 1.5, S, C)
    tab[:, 1] = 0.5 * r(S, C)
    tab[:, 2] = (torch.rand(S, C, generator=g) < 0.75).float()          # some input channels are read raw (fl = 0)
    save = torch.stack([0.3 * r(S, cout), u(0.5, 2.0, S, cout)], -1)     # (mean, invstd)
    consts = torch.stack([0.1 * r(S, cout), 0.1 * r(S, cout), u(0.5, 1.5, S, cout)], -1)      # (c1, c2, k)
    return dict(g=r(S, M, cout), z=r(S, M, cout), x=r(S, M, cin), tab=tab, save=save, consts=consts,
                w=r(cout, cin) / cin ** 0.5, gadd=r(S, M, cin), gx0=r(S, M, cin), gw0=0.1 * r(cout, cin))


def _reference(t, cout, accumulate, gadd):
    """fp64: g_z = k (g silu'(y) - c1 - zhat c2); gx (=|+=) g_z . w (+ gadd); gw += g_z^T . a_in over all slots."""
    d = {k: v.double() for k, v in t.items()}
    sc, sh = d["tab"][:, 0, :cout].unsqueeze(1), d["tab"][:, 1, :cout].unsqueeze(1)
    isc, ish, ifl = (d["tab"][:, i, cout:].unsqueeze(1) for i in range(3))
    mean, istd = d["save"][..., 0].unsqueeze(1), d["save"][..., 1].unsqueeze(1)
    c1, c2, k = (d["consts"][..., i].unsqueeze(1) for i in range(3))
    y = d["z"] * sc + sh
    s = torch.sigmoid(y)
    gz = k * (d["g"] * s * (1 + y * (1 - s)) - c1 - (d["z"] - mean) * istd * c2)
    yi = d["x"] * isc + ish
    a_in = torch.where(ifl != 0, yi * torch.sigmoid(yi), d["x"])
    gx = gz @ d["w"]
    if gadd:
        gx = gx + d["gadd"]
    if accumulate:
        gx = gx + d["gx0"]
    gw = d["gw0"] + torch.einsum("smn,smk->nk", gz, a_in)
    return gx, gw


def _run(dev, cout, M, S, accumulate, gadd, route, max_wg, cin=CIN):
    lib = _lib.load_library()
    gx, gw = dev["gx0"].clone(), dev["gw0"].clone()
    rc = lib.jn_pw_bwd_fused(ptr(dev["g"]), ptr(dev["z"]), ptr(dev["x"]), ptr(dev["tab"]), ptr(dev["save"]), ptr(dev["consts"]),
                             ptr(dev["w"]), ptr(dev["gadd"]) if gadd else None, int(accumulate), ptr(gx), ptr(gw), S, M, cout, cin,
                             route, max_wg, None)
    _lib.check(rc, "jn_pw_bwd_fused")
    torch.cuda.synchronize()
    return gx.cpu(), gw.cpu()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("cout", [128, 64])
def test_fused128_matches_fp64_and_the_64_pixel_kernel(cout, M, S):
    t = _inputs(cout, M, S, seed=1000 * cout + 10 * M + S)
    dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
    for accumulate, gadd in itertools.product((False, True), (False, True)):
        want_gx, want_gw = _reference(t, cout, accumulate, gadd)
        dw_scale = want_gw.abs().max().item()
        old_gx, old_gw = _run(dev, cout, M, S, accumulate, gadd, 1, 0)
        old_dw = (old_gw.double() - want_gw).abs().max().item() / dw_scale
        print(f"cout {cout} M {M} S {S} acc {int(accumulate)} gadd {int(gadd)}: route 1 dW {old_dw:.2e}")
        assert old_dw < 1e-4, ("route 1", old_dw)
        for max_wg in (0, 1, 2):
            gx, gw = _run(dev, cout, M, S, accumulate, gadd, 0, max_wg)
            gx_rel = ((gx.double() - want_gx).norm() / want_gx.norm()).item()
            dw = (gw.double() - want_gw).abs().max().item() / dw_scale
            vs_old = ((gx - old_gx).double().norm() / old_gx.double().norm()).item()
            print(f"  max_wg {max_wg}: gx rel L2 {gx_rel:.2e}  dW {dw:.2e}  against route 1: rel L2 {vs_old:.2e}")
            if cout == 64:
                assert torch.equal(gx, old_gx), ("gx differs from the 64-pixel kernel", max_wg, (gx - old_gx).abs().max().item())
            else:
                assert vs_old < 2e-5, (max_wg, vs_old)
            assert gx_rel < 2e-5, (max_wg, gx_rel)
            assert dw < 1e-4, (max_wg, dw)
            gx2, gw2 = _run(dev, cout, M, S, accumulate, gadd, 0, max_wg)
            assert torch.equal(gx2, gx), max_wg
            if max_wg == 1:
                assert torch.equal(gw2, gw)
            else:
                again = (gw2 - gw).abs().max().item() / dw_scale
                assert again < 1e-5, (max_wg, again)


@pytest.mark.parametrize("cin", [16, 32, 64, 128])
@pytest.mark.parametrize("cout", [16, 32, 64, 128])
def test_fused_backward_matches_fp64_at_every_shape_the_entry_admits(cout, cin):
    """All sixteen shapes of pw_bwd_fused_supported on the launcher's own choice of kernel (pw_bwd_fused_kernel<cout / 16, cin / 16,
    false>, 64-pixel tiles; pw_bwd_fused128_kernel at 128 input and 64 or 128 output channels), at M = 1, a tile less one pixel, a
    tile, a tile and a pixel, two tiles and two pixels; one and three slots; max_wg 0, 1, 2.  The bars of the test above.  Two runs
    give the same dW bits where every element has one writer (max_wg = 1 and, on the 64-pixel kernel, whose grid has a row per
    slot, one slot), else dW to the order of its fp32 atomics.  (The RED / RED2 forms are not reachable through this entry.)"""
    per_slot_grid = not (cin == 128 and cout in (64, 128))
    worst_gx = worst_dw = 0.0
    for M, S in itertools.product((1, 63, 64, 65, 130), (1, 3)):
        t = _inputs(cout, M, S, seed=100000 * cout + 1000 * cin + 10 * M + S, cin=cin)
        dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
        for accumulate, gadd in ((False, False), (True, True)):
            want_gx, want_gw = _reference(t, cout, accumulate, gadd)
            dw_scale = want_gw.abs().max().item()
            for max_wg in (0, 1, 2):
                gx, gw = _run(dev, cout, M, S, accumulate, gadd, 0, max_wg, cin=cin)
                gx_rel = ((gx.double() - want_gx).norm() / want_gx.norm()).item()
                dw = (gw.double() - want_gw).abs().max().item() / dw_scale
                worst_gx, worst_dw = max(worst_gx, gx_rel), max(worst_dw, dw)
                assert gx_rel < 2e-5, (M, S, accumulate, max_wg, gx_rel)
                assert dw < 1e-4, (M, S, accumulate, max_wg, dw)
                gx2, gw2 = _run(dev, cout, M, S, accumulate, gadd, 0, max_wg, cin=cin)
                assert torch.equal(gx2, gx), (M, S, accumulate, max_wg)
                if max_wg == 1 and (S == 1 or not per_slot_grid):
                    assert torch.equal(gw2, gw), (M, S, accumulate)
                else:
                    again = (gw2 - gw).abs().max().item() / dw_scale
                    assert again < 1e-5, (M, S, accumulate, max_wg, again)
    print(f"{cin} -> {cout}: worst gx rel L2 {worst_gx:.2e}, worst dW {worst_dw:.2e} of max|dW|")


def test_entry_refuses_bad_arguments():
    lib = _lib.load_library()
    t = {k: v.to(DEV).contiguous() for k, v in _inputs(128, 4, 1, seed=5).items()}
    args = lambda **o: [ptr(t["g"]), ptr(t["z"]), ptr(t["x"]), ptr(t["tab"]), ptr(t["save"]), ptr(t["consts"]), ptr(t["w"]), None, 0,
                        ptr(t["gx0"]), ptr(t["gw0"]), o.get("S", 1), o.get("M", 4), o.get("cout", 128), o.get("cin", 128),
                        o.get("route", 0), o.get("max_wg", 0), None]
    for bad in (dict(S=0), dict(M=0), dict(cout=48), dict(cin=256), dict(route=2), dict(max_wg=-1)):
        assert lib.jn_pw_bwd_fused(*args(**bad)) == -1, bad
    a = args()
    a[0] = None
    assert lib.jn_pw_bwd_fused(*a) == -1


def test_encoder_backward_with_small_128_channel_maps_matches_autograd():
    """64-pixel patches, N = 3: the 128-channel maps of the encoder have 48 and 12 pixels per step: a partial first tile and a
    workgroup per tile.  Bars of test_nano_backbone_backward_vs_autograd."""
    product, oracle = make_pair(3, patch_size=64, block_size=6, with_detector=False, image_processor=None, gpt_backbone="yolox-nano")
    g = torch.Generator().manual_seed(29)
    x = torch.rand((3, 3, 64, 64), generator=g)
    net = oracle.gpt_backbone.train()
    outs = net(x)
    R = [torch.randn(o.shape, generator=g) for o in outs]
    loss = sum((o * r).sum() for o, r in zip(outs, R))
    net.zero_grad()
    loss.backward()
    product.engine_zero_grad()
    product.backbone_features(x, train=True)
    product.backbone_backward(x, R)
    got = product.engine_grads("gpt_backbone.")
    torch.cuda.synchronize()
    for name, p in net.named_parameters():
        ref = p.grad
        scale = ref.abs().max().item() + 1e-6
        err = (got["gpt_backbone." + name] - ref).abs().max().item() / scale
        assert err < 2e-3, (name, err, scale)
