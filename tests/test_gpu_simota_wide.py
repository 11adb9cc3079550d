"""`yolox_loss_wide_kernel` — the SimOTA loss over EVERY box of a patch, the opt-in box policy "all" — against the fp64
oracle (`oracle/yolox_ref.py::losses_from_raw`): on the wide cases of tests/simota_wide_cases.py (9 to 64 boxes in a patch,
up to 761 candidates, contested anchors won by boxes the default kernel would cut) and on every committed case of
tests/simota_cases.py, with the assertions and the fixed bars of tests/test_gpu_simota_loss.py.  Then what surrounds the
kernel: determinism, the policy switch on the engine's three loss paths, the engine against the CPU oracle with eleven
boxes in a patch, and the capacity checks."""
import copy
import ctypes as C

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, yolox
from jolineedle_amd._lib import ptr
from tests import simota_cases as sc
from tests import simota_wide_cases as wc
from tests.helpers import make_pair, model_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _id(case):
    return f"{case.P}-{case.N}x{case.nb}-{case.layout}-s{case.seed}-{'l1' if case.use_l1 else 'nol1'}"


def _check_against_oracle(case, ref, raw, tg):
    d_raw, metrics, scale = (t.cpu() for t in yolox.yolox_loss(raw.to(DEV), tg.to(DEV), case.P, sc.STRIDES, case.use_l1,
                                                               sc.LOSS_SCALE, boxes="all"))
    assert d_raw.shape == (case.N, sc.n_anchors(case.P), 6) and bool(torch.isfinite(d_raw).all())
    # ---- exact: the foreground set per patch, the counts, zeros on the background ----
    fg = d_raw[..., 4] < 0                                         # sigmoid(o) - 1 < 0 on foreground, sigmoid(o) > 0 elsewhere
    for n in range(case.N):
        assert torch.equal(fg[n], ref["fg"][n]), (n, "kernel only", (fg[n] & ~ref["fg"][n]).nonzero().flatten().tolist(),
                                                  "oracle only", (~fg[n] & ref["fg"][n]).nonzero().flatten().tolist())
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
    return d_raw


@pytest.mark.parametrize("case", wc.ALL, ids=_id)
def test_wide_kernel_vs_fp64_oracle_on_the_wide_cases(case):
    _check_against_oracle(case, wc.reference(case), *wc.build(case))


@pytest.mark.parametrize("case", sc.CASES + [sc.TIE_CASE], ids=_id)
def test_wide_kernel_vs_fp64_oracle_on_the_committed_cases(case):
    """The wide path is exact where the narrow one is."""
    ref = sc.reference(case)
    d_raw = _check_against_oracle(case, ref, *sc.build(case))
    if case.layout == "tie":                                       # the even split reached the gradient
        a = int(ref["fg"][0].nonzero())
        assert ref["num_fg"] == 1 and float(d_raw[0, a, 0]) != 0.0


def test_two_launches_give_the_same_bits():
    case = wc.DETERMINISM_CASE
    raw, tg = wc.build(case)
    assert wc.margins(case)["patches"][0]["ng"] == 40
    raw_d, tg_d = raw.to(DEV), tg.to(DEV)
    a = yolox.yolox_loss(raw_d, tg_d, case.P, sc.STRIDES, True, sc.LOSS_SCALE, boxes="all")
    b = yolox.yolox_loss(raw_d, tg_d, case.P, sc.STRIDES, True, sc.LOSS_SCALE, boxes="all")
    for x, y, name in zip(a, b, ("d_raw", "metrics", "scale")):
        assert torch.equal(x, y), name


def test_the_policy_switch_on_the_three_engine_paths():
    raw, tg = sc.build(sc.BOX_CAP_CASE)
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):                    # the default did not move
        yolox.yolox_loss(raw.to(DEV), tg.to(DEV), sc.BOX_CAP_CASE.P, sc.STRIDES, True, 1.0)
    product, _ = make_pair(9, patch_size=64, block_size=4, image_processor="yolox-nano", max_batch=2)
    x = torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    tg64 = tg.clone()
    tg64[..., 1:] *= 64.0 / sc.BOX_CAP_CASE.P
    num_gt = int((sc.to_cxcywh(tg64).sum(2) > 0).sum())
    assert num_gt >= 12 and product.det_loss_boxes == "cap8"
    # at most eight rows: the default kernel under either policy, bit for bit.  (The validation loss reads the backbone's
    # running statistics, which no validation call moves, and the head's batch statistics, which are the patches' own.)
    ok8 = tg64[:, :8].contiguous()
    _, _, narrow = product.yolox.validation_loss(x, ok8, predict=False)
    product.set_det_loss_boxes("all")
    assert product.det_loss_boxes == "all"
    try:
        _, _, same = product.yolox.validation_loss(x, ok8, predict=False)
        for k in yolox.LOSS_NAMES:
            assert torch.equal(same[k], narrow[k]), k
        _, _, l_fwd = product.yolox(x, tg64)
        l_step = product.yolox.loss_and_backward(x, tg64)
        _, _, l_val = product.yolox.validation_loss(x, tg64)
        for losses in (l_fwd, l_step, l_val):
            assert all(bool(torch.isfinite(losses[k])) for k in yolox.LOSS_NAMES), losses
            nfg = float(losses["num_fg"]) * num_gt
            assert abs(nfg - round(nfg)) < 1e-3 and round(nfg) >= 1, nfg
        with pytest.raises(ValueError, match="every"):
            product.set_det_loss_boxes("every")
        assert product.det_loss_boxes == "all"
    finally:
        product.set_det_loss_boxes("cap8")
    assert product.det_loss_boxes == "cap8"
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        product.yolox.loss_and_backward(x, tg64)
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        product.yolox(x, tg64)
    with pytest.raises(ValueError, match=r"patch 0 holds 11 .* at most 8"):
        product.yolox.validation_loss(x, tg64)


# Targets of the engine test: eleven boxes in patch 0, three in patch 1, drawn from this seed.  Chosen on the CPU among
# 1..50 by tracing the fp64 oracle head's own raw outputs with simota_cases._trace_patch: margins (a) 2.5e-1 px,
# (b) 3.9e-2, (c) 3.0e-2, (d) 1.1e-1, (e) 1.6e-1 px — admissible (thresholds 1e-3, 1e-2, 1e-3, 1e-3, 1e-4), and the
# widest (c) and (d) of the admissible seeds; 10 foreground anchors.
ENGINE_SEED = 29


def _engine_targets(P=64):
    g = torch.Generator().manual_seed(ENGINE_SEED)
    tg = torch.zeros((2, 12, 5))
    for n, k in ((0, 11), (1, 3)):
        c = torch.rand((k, 2), generator=g) * (P - 16) + 8
        wh = torch.rand((k, 2), generator=g) * 24 + 6
        tg[n, :k, 1:3] = c - wh / 2
        tg[n, :k, 3:5] = c + wh / 2
    return tg


def test_engine_vs_oracle_with_eleven_boxes_in_a_patch():
    """jn_detector_step under "all" against torch autograd on the CPU oracle: the six losses and the predictor-conv
    gradients, by the rules of test_detector_training_step_vs_oracle."""
    from tests.test_gpu_parity import _blocky_images, _detector_pair
    P, N = 64, 2
    product, oracle = _detector_pair(P, 0.5, image_processor="yolox-nano", max_batch=N)
    x, tg = _blocky_images(N, P, 8), _engine_targets(P)
    assert int((sc.to_cxcywh(tg)[0].sum(1) > 0).sum()) == 11
    det64 = copy.deepcopy(oracle.yolox).double().train()        # conditioning reference: the same graph in fp64
    with torch.no_grad():                                       # the seed's margins, on the fp64 head's own outputs
        raw64, _ = det64.head.raw_logits(det64.backbone(x.double()))
    grid, stride, _ = sc.geometry(P)
    lab = sc.to_cxcywh(tg.double())
    traces = [sc._trace_patch(lab[n, :int((lab[n].sum(1) > 0).sum()), 1:], raw64[n], grid, stride) for n in range(N)]
    assert sc.admissible({k: min(t[k] for t in traces) for k in "abcde"}) and traces[0]["ng"] == 11
    _, _, ref64 = det64(x.double(), tg.double())
    ref64["total_loss"].backward()
    g64 = {n: p.grad for n, p in det64.named_parameters() if p.grad is not None}
    det = oracle.yolox.train()
    det.zero_grad()
    _, _, ref = det(x, tg)
    ref["total_loss"].backward()
    product.set_det_loss_boxes("all")
    product.engine_zero_grad()
    got = product.yolox.loss_and_backward(x, tg)
    for k in ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg"):
        r, v = float(torch.as_tensor(ref[k]).detach()), float(got[k])
        assert abs(v - r) < 2e-3 * max(1.0, abs(r)), (k, v, r)
    assert round(float(got["num_fg"]) * 14) == sum(t["nfg"] for t in traces)
    grads = product.engine_grads("yolox.")
    checked = 0
    for name, p in det.named_parameters():
        if p.grad is None or "_preds" not in name:
            continue
        gp, rg = grads["yolox." + name], p.grad
        scale = rg.abs().max().item()
        if scale < 1e-10:
            assert gp.abs().max().item() < 1e-7, name
            continue
        cond = (rg.double() - g64[name]).abs().max().item() / scale
        err = (gp.double() - g64[name]).abs().max().item() / scale
        assert err < max(5e-3, 8.0 * cond), (name, err, cond, scale)
        checked += 1
    assert checked >= 9                                            # weights of the nine predictor convs at least


def test_capacity_is_checked_on_the_host():
    lib = _lib.load_library()
    stream = _lib.current_stream(torch.device(DEV))
    metrics, scale = torch.zeros(8, device=DEV), torch.zeros(1, device=DEV)

    def call(raw, tg, P):
        out = torch.empty_like(raw)
        rc = lib.jn_yolox_loss_wide(ptr(raw), ptr(tg), raw.shape[0], tg.shape[1], P, 8, 16, 32, 1, C.c_float(1.0), ptr(out),
                                    ptr(metrics), ptr(scale), stream)
        return rc, out
    most = yolox.MAX_BOXES_WIDE
    raw64 = torch.zeros((1, sc.n_anchors(64), 6), device=DEV)
    rc, _ = call(raw64, torch.zeros((1, most + 1, 5), device=DEV), 64)
    assert rc == -1 and str(most).encode() in lib.jn_last_error() and b"JN_DETLOSS_MAX_BOXES" in lib.jn_last_error()
    assert sc.n_anchors(672) == 9261
    rc, _ = call(torch.zeros((1, 9261, 6), device=DEV), torch.zeros((1, 1, 5), device=DEV), 672)
    assert rc == -1 and b"A=9261" in lib.jn_last_error()
    with pytest.raises(_lib.JnError):                              # a wider `targets` raises from the C check
        yolox.yolox_loss(raw64, torch.zeros((1, most + 1, 5), device=DEV), 64, boxes="all")
    bare = ja.GPT(model_config(patch_size=64, block_size=2, with_detector=False, image_processor=None), max_batch=1)
    assert lib.jn_set_det_loss_boxes(bare.engine().handle, 1) == -5 and b"detector" in lib.jn_last_error()
    with pytest.raises(_lib.JnError):
        bare.set_det_loss_boxes("all")
    assert bare.det_loss_boxes == "cap8"
    # the widest `targets` the kernel takes: two real rows in MAX_BOXES_WIDE equal the two rows alone, bit for bit
    case = next(c for c in sc.CASES if c.P == 64 and c.nb == 2 and c.N == 1)
    raw, tg = sc.build(case)
    padded = torch.zeros((1, most, 5))
    padded[:, :2] = tg
    a = yolox.yolox_loss(raw.to(DEV), tg.to(DEV), 64, sc.STRIDES, True, sc.LOSS_SCALE, boxes="all")
    b = yolox.yolox_loss(raw.to(DEV), padded.to(DEV), 64, sc.STRIDES, True, sc.LOSS_SCALE, boxes="all")
    assert sc.reference(case)["num_gt"] == 2
    for u, v, name in zip(a, b, ("d_raw", "metrics", "scale")):
        assert torch.equal(u, v), name
