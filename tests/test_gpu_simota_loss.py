"""`yolox_loss_kernel` through the context-free `jn_yolox_loss` against the fp64 oracle (`oracle/yolox_ref.py::
losses_from_raw`) on the committed cases of tests/simota_cases.py: dynamic k up to 8, contested anchors, boxes left without
an anchor, 209 candidates over ten 256-anchor chunks, empty patches, boxes without a candidate, the zero-row-first quirk,
the exact max / min tie.  The assignment is compared exactly (the cases keep every decision away from a tie, see
simota_cases.margins), the numbers against fixed bars: 8 x the fp32 CPU oracle's own distance from fp64."""
import ctypes as C

import pytest
import torch

from jolineedle_amd import _lib, yolox
from jolineedle_amd._lib import ptr
from tests import simota_cases as sc
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(case):
    raw, tg = sc.build(case)
    d_raw, metrics, scale = yolox.yolox_loss(raw.to(DEV), tg.to(DEV), case.P, sc.STRIDES, case.use_l1, sc.LOSS_SCALE)
    return d_raw.cpu(), metrics.cpu(), scale.cpu()


def _id(case):
    return f"{case.P}-{case.N}x{case.nb}-{case.layout}-s{case.seed}-{'l1' if case.use_l1 else 'nol1'}"


@pytest.mark.parametrize("case", sc.CASES + [sc.TIE_CASE], ids=_id)
def test_loss_kernel_vs_fp64_oracle(case):
    ref = sc.reference(case)
    d_raw, metrics, scale = _run(case)
    assert d_raw.shape == (case.N, sc.n_anchors(case.P), 6) and bool(torch.isfinite(d_raw).all())
    # ---- exact: the foreground set per patch, the counts, zeros on the background ----
    fg = d_raw[..., 4] < 0                                         # sigmoid(o) - 1 < 0 on foreground, sigmoid(o) > 0 elsewhere
    for n in range(case.N):
        assert torch.equal(fg[n], ref["fg"][n]), (n, "kernel only", (fg[n] & ~ref["fg"][n]).nonzero().flatten().tolist(),
                                                  "oracle only", (~fg[n] & ref["fg"][n]).nonzero().flatten().tolist())
    # num_fg from the scale, then num_gt from metrics[5] = num_fg / max(num_gt, 1): one fp32 division of two small integers
    assert round(sc.LOSS_SCALE / float(scale)) == max(ref["num_fg"], 1), (float(scale), ref["num_fg"])
    assert round(float(metrics[5]) * max(ref["num_gt"], 1)) == ref["num_fg"], (float(metrics[5]), ref["num_fg"], ref["num_gt"])
    assert float(metrics[5]) == float(torch.tensor(ref["num_fg"], dtype=torch.float32) / max(ref["num_gt"], 1))
    assert bool((d_raw[~fg][:, [0, 1, 2, 3, 5]] == 0).all())
    # ---- numbers against fp64, fixed bars ----
    got = dict(metrics=[float(v) for v in metrics[:5].double()], scale=float(scale.double()),
               grad=d_raw.double() * scale.double())
    dist = sc.distances(got, ref)
    print(f"{_id(case)}: num_fg {ref['num_fg']} num_gt {ref['num_gt']}  metrics {['%.2e' % v for v in dist['metrics']]}  "
          f"scale {dist['scale']:.2e}  grad max {['%.2e' % v for v in dist['grad_max']]}  fg L2 {dist['grad_fg_l2']:.2e}")
    sc.check_bars(dist, _id(case))
    if case.layout == "tie":                                       # the even split reached the gradient: half of either edge's share
        a = int(ref["fg"][0].nonzero())
        assert ref["num_fg"] == 1 and float(d_raw[0, a, 0]) != 0.0


def test_twelve_rows_with_at_most_eight_boxes_equal_eight_rows():
    """nb > 8 is accepted as long as no patch holds more than eight boxes: the padding rows change nothing, bit for bit."""
    case = next(c for c in sc.CASES if c.nb == 8 and c.N >= 2 and c.P == 160 and c.use_l1)
    raw, tg = sc.build(case)
    wide = torch.zeros((case.N, 12, 5))
    wide[:, :8] = tg
    raw_d = raw.to(DEV)
    a = yolox.yolox_loss(raw_d, tg.to(DEV), case.P, sc.STRIDES, True, sc.LOSS_SCALE)
    b = yolox.yolox_loss(raw_d, wide.to(DEV), case.P, sc.STRIDES, True, sc.LOSS_SCALE)
    assert int((sc.to_cxcywh(wide).sum(2) > 0).sum(1).max()) == 8
    for x, y, name in zip(a, b, ("d_raw", "metrics", "scale")):
        assert torch.equal(x, y), name


def test_more_than_eight_boxes_in_a_patch_are_refused():
    """Eleven boxes in one patch: the reference uses all eleven, the kernel would keep eight.  Every Python entry says so."""
    raw, tg = sc.build(sc.BOX_CAP_CASE)
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        yolox.yolox_loss(raw.to(DEV), tg.to(DEV), sc.BOX_CAP_CASE.P, sc.STRIDES, True, 1.0)
    product, _ = make_pair(9, patch_size=64, block_size=4, image_processor="yolox-nano", max_batch=2)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    tg64 = tg.clone()
    tg64[..., 1:] *= 64.0 / sc.BOX_CAP_CASE.P
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        product.yolox.loss_and_backward(x, tg64)
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        product.yolox(x, tg64)
    ok = tg64.clone()
    ok[:, 8:] = 0.0                                                # eight boxes in twelve rows pass
    losses = product.yolox.loss_and_backward(x, ok)
    assert bool(torch.isfinite(losses["total_loss"]))


def test_entry_point_contract():
    lib = _lib.load_library()
    P, A = 64, sc.n_anchors(64)
    raw = torch.zeros((1, A, 6), device=DEV)
    tg = torch.zeros((1, 1, 5), device=DEV)
    d_raw, metrics, scale = torch.empty_like(raw), torch.zeros(8, device=DEV), torch.zeros(1, device=DEV)

    def call(raw_=raw, tg_=tg, N=1, nb=1, P_=P, out=d_raw):
        return lib.jn_yolox_loss(ptr(raw_), ptr(tg_), N, nb, P_, 8, 16, 32, 1, C.c_float(1.0), ptr(out), ptr(metrics), ptr(scale),
                                 _lib.current_stream(torch.device(DEV)))
    assert call(nb=0) == -1 and b"row" in lib.jn_last_error()
    assert call(P_=100) == -1 and b"100" in lib.jn_last_error()
    assert call(raw_=None) == -1 and call(tg_=None) == -1 and call(out=None) == -1
    assert call(N=0) == -1
    assert call() == 0                                             # N = 1, nb = 1: an empty patch, objectness only
    torch.cuda.synchronize()
    assert float(scale) == 1.0 and float(metrics[5]) == 0.0
    want = A * torch.log(torch.tensor(2.0, dtype=torch.float64)).item()          # softplus(0) per anchor, denominator 1
    assert abs(float(metrics[2]) - want) <= 1.25e-6 * want and float(metrics[0]) == float(metrics[2])
    assert bool((d_raw[..., 4] == 0.5).all()) and bool((d_raw[..., [0, 1, 2, 3, 5]] == 0).all())
    with pytest.raises(_lib.JnError):
        yolox.yolox_loss(raw, tg[:, :0], P)
