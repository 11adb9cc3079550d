"""Teacher-forced validation on the device: the loss / accuracy kernel (jn_supervised_metrics) against fp64 torch, the
eval-mode supervised pass (jn_supervised_eval) and the detector's validation loss (jn_detector_eval_loss: eval-mode
PAFPN, train-mode head) against the CPU oracle, and ``SupervisedTrainer.eval_supervised_on_images`` /
``test_on_images`` end to end.

Bars.  Kernel: 2e-6 * max(1, |ref|) on the per-token loss and the mean against fp64 (fp32 torch on these logits sits at
1.6e-7); everything integer exact.  Supervised pass: the suite's TOL_LOGIT on the logits, 2e-4 on the loss (the bar of
test_supervised_step_vs_oracle); accuracy exact, on inputs whose smallest top-2 logit gap in the oracle is >= 1e-3 (ten
logit bars), asserted.  Detector: 2e-3 * max(1, |ref|) on the six loss entries (the bar of
test_detector_training_step_vs_oracle), fp64_bars.STAT_ATOL / STAT_RTOL on the head's running statistics, TOL_MAP on the
maps."""
import copy

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, detection
from jolineedle_amd._lib import check, ptr
from tests.fp64_bars import STAT_ATOL, STAT_RTOL
from tests.helpers import make_pair, synth_batch, synth_tokens
from tests.test_gpu_parity import TOL_LOGIT, TOL_MAP, _detector_pair, _loose_box_match
from tests.test_supervised_eval_cpu import literal_labels, prefix_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOP_W = 2.5
LOSS_NAMES = ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg")
LOSS_BAR = 2e-3
MODES = ("best-action", "on-self-trajectory")


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------
def _metrics_call(logits, cur, nxt, masks, on_self, want=True):
    B, T, nA = logits.shape
    d = lambda t, dt: t.to(DEV, dt).contiguous()
    lg, c, n, m = d(logits, torch.float32), d(cur, torch.int64), d(nxt, torch.int64), d(masks, torch.uint8)
    tl = torch.full((B, T), -7.0, device=DEV) if want else None
    pr = torch.full((B, T), 77, device=DEV, dtype=torch.uint8) if want else None
    out = torch.full((4,), -7.0, device=DEV)
    check(_lib.load_library().jn_supervised_metrics(ptr(lg), ptr(c), ptr(n), ptr(m), B, T, nA, STOP_W, int(on_self), ptr(tl),
                                                    ptr(pr), ptr(out), _lib.current_stream(torch.device(DEV))),
          "jn_supervised_metrics")
    return out.cpu(), None if tl is None else tl.cpu(), None if pr is None else pr.cpu()


def _metrics_ref64(logits, labels, masks):
    B, T, nA = logits.shape
    w = torch.ones(nA, dtype=torch.float64)
    if nA > 8:
        w[8] = STOP_W
    ce = torch.nn.functional.cross_entropy(logits.double().reshape(B * T, nA), labels.flatten(), weight=w, reduction="none")
    valid = (masks == 1).flatten()
    pred = logits.reshape(B * T, nA).argmax(dim=1)                    # CPU argmax: the first maximum
    hits = (pred[valid] == labels.flatten()[valid]).sum()
    return ce.view(B, T), valid.view(B, T), pred.view(B, T), hits


@pytest.mark.parametrize("B,T,nA", [(1, 1, 9), (3, 5, 9), (7, 11, 8), (64, 62, 9)])
@pytest.mark.parametrize("loss_mode", MODES)
def test_metrics_kernel_against_fp64(B, T, nA, loss_mode):
    g = torch.Generator().manual_seed(1000 * B + T)
    logits = torch.randn((B, T, nA), generator=g) * 3
    logits[0, 0, 5] = logits[0, 0, 2] = logits[0, 0].max() + 1.0          # a tie: the first maximum wins
    cur, nxt = torch.randint(0, nA, (B, T), generator=g), torch.randint(0, nA, (B, T), generator=g)
    # a full row, a row of length 1 and an all-padding row, then random prefixes (B = 1: the one row is both full and 1 long)
    lengths = ([T, 1, 0] + torch.randint(0, T + 1, (max(B - 3, 0),), generator=g).tolist())[:B]
    masks = prefix_masks(lengths, T, torch.uint8)
    on_self = loss_mode == "on-self-trajectory"
    labels = literal_labels(cur, nxt, masks, loss_mode)
    ce, valid, pred, hits = _metrics_ref64(logits, labels, masks)
    m, tl, pr = _metrics_call(logits, cur, nxt, masks, on_self)
    n_valid = int(valid.sum())
    assert n_valid == sum(lengths) and float(m[3]) == n_valid
    ref_tl = torch.where(valid, ce, torch.zeros_like(ce))
    err = (tl.double() - ref_tl).abs() / ref_tl.abs().clamp(min=1.0)
    mean = float(ce[valid].mean())
    print(f"token loss err {float(err.max()):.2e}, mean err {abs(float(m[0]) - mean) / max(1.0, abs(mean)):.2e}")
    assert float(err.max()) <= 2e-6
    assert abs(float(m[0]) - mean) <= 2e-6 * max(1.0, abs(mean))
    assert torch.equal(tl[~valid], torch.zeros_like(tl[~valid])) and torch.equal(pr[~valid], torch.zeros_like(pr[~valid]))
    assert torch.equal(pr[valid].long(), pred[valid]) and int(pr[0, 0]) == 2
    assert float(m[1]) == float(torch.tensor(float(hits)) / torch.tensor(float(n_valid)))        # one fp32 division, as torch's mean
    assert float(m[2]) == float(masks.sum(dim=1).float().mean())
    # the labels, through the loss they select: where the two modes pick different actions the per-token losses differ
    other = literal_labels(cur, nxt, masks, MODES[1 - MODES.index(loss_mode)])
    differs = valid & (other != labels)
    if differs.any():
        ce_other = _metrics_ref64(logits, other, masks)[0]
        far = differs & ((ce_other - ce).abs() > 1e-3)
        assert far.any() and ((tl.double() - ce).abs()[far] < (tl.double() - ce_other).abs()[far]).all()
    # ordered sums: a second call gives the same bits; the optional outputs are optional
    m2, tl2, pr2 = _metrics_call(logits, cur, nxt, masks, on_self)
    assert torch.equal(m.view(torch.int32), m2.view(torch.int32)) and torch.equal(tl, tl2) and torch.equal(pr, pr2)
    m3, _, _ = _metrics_call(logits, cur, nxt, masks, on_self, want=False)
    assert torch.equal(m.view(torch.int32), m3.view(torch.int32))
    # the empty batch: torch's mean of nothing is NaN, the accuracy's NaN becomes 0 (src/supervised.py:188-195)
    e, etl, epr = _metrics_call(logits, cur, nxt, torch.zeros_like(masks), on_self)
    assert torch.isnan(e[0]) and float(e[1]) == 0.0 and float(e[2]) == 0.0 and float(e[3]) == 0.0
    assert not etl.any() and not epr.any()


# ---- 2. the eval-mode supervised pass ------------------------------------------------------------------------------------
def _oracle_metrics(oracle, patches, cur, nxt, classes, positions, masks, loss_mode, nA=9):
    with torch.no_grad():
        logits, _ = oracle(patches, cur, classes, positions)
    B, T = cur.shape
    labels = literal_labels(cur, nxt, masks, loss_mode)
    w = torch.ones(nA)
    w[8] = STOP_W
    ce = torch.nn.functional.cross_entropy(logits.reshape(B * T, nA), labels.flatten(), weight=w, reduction="none").view(B, T)
    valid = masks == 1
    pred = logits.argmax(dim=2)
    top2 = logits.topk(2, dim=2).values
    return {"logits": logits, "labels": labels, "token_loss": torch.where(valid, ce, torch.zeros_like(ce)), "pred": pred,
            "loss": ce[valid].mean(), "accuracy": (pred[valid] == labels[valid]).float().mean(),
            "episode_length": masks.sum(dim=1).float().mean(), "gap": float((top2[..., 0] - top2[..., 1])[valid].min())}


def _sup_cfg(loss_mode="best-action", **kw):
    return ja.CfgNode(stop_enabled=True, stop_weight=STOP_W, loss_mode=loss_mode, **kw)


def _state(product):
    product.sync_weights()
    product.pull_parameters()
    return {k: v.detach().cpu().clone() for k, v in product.state_dict().items()}


@pytest.mark.parametrize("B,T,tok_seed", [(3, 5, 100), (1, 8, 101)])
def test_supervised_eval_against_the_eval_mode_oracle(B, T, tok_seed):
    """15 patches at max_batch 4 (chunks of 4 + 4 + 4 + 3 that straddle the sequences), and one sequence of block_size."""
    product, oracle = make_pair(3, patch_size=64, block_size=8, with_detector=False, image_processor=None, max_batch=4)
    patches, cur, positions = synth_tokens(B, T, 64, 9, 4, tok_seed)
    classes = torch.tensor([3, 99, 0][:B])
    nxt = torch.randint(0, 9, (B, T), generator=torch.Generator().manual_seed(7))
    nxt[0, 1] = 8                                                      # a STOP label: the class weight
    masks = prefix_masks([T, 2, 4][:B], T)
    before = _state(product)
    for loss_mode in MODES:
        ref = _oracle_metrics(oracle, patches, cur, nxt, classes, positions, masks, loss_mode)
        assert ref["gap"] >= 1e-3, ref["gap"]                          # the condition under which the arg-max is decided
        got = ja.SupervisedTrainer(_sup_cfg(loss_mode), product).eval_step(patches, cur, nxt, positions, masks, classes=classes)
        torch.cuda.synchronize()
        m = got["metrics"].cpu()
        print(f"logits err {float((got['logits'].cpu() - ref['logits']).abs().max()):.2e}, loss {float(m[0])} vs {float(ref['loss'])}")
        assert (got["logits"].cpu() - ref["logits"]).abs().max() < TOL_LOGIT
        assert abs(float(m[0]) - float(ref["loss"])) < 2e-4
        assert (got["token_loss"].cpu() - ref["token_loss"]).abs().max() < 2e-4 * STOP_W
        assert float(m[1]) == float(ref["accuracy"]) and float(m[2]) == float(ref["episode_length"])
        valid = masks == 1
        assert torch.equal(got["predicted"].cpu().long()[valid], ref["pred"][valid]) and not got["predicted"].cpu()[~valid].any()
        assert float(m[3]) == float(valid.sum())
    # nothing of the model moved: every parameter and every BatchNorm statistic reads back bit for bit
    after = _state(product)
    assert before.keys() == after.keys() and sum(k.endswith("running_var") for k in before) > 50
    for k in before:
        assert torch.equal(before[k], after[k]), k
    # the same numbers as the path the package offered before: GPT.forward in eval mode, T passes of B patches
    lg_old, _ = product(patches, cur, classes, positions)
    assert (lg_old - got["logits"]).abs().max() < TOL_LOGIT


def test_supervised_eval_and_gpt_forward_decode_alike():
    """B = 3, T = 3 at max_batch 4, eval mode, no dropout: jn_supervised_eval (encoder chunks of 4 + 4 + 1 patches) and
    jn_gpt_forward (three passes of 3) embed and decode through the same two functions of the library, so their logits on
    the same inputs are equal bit for bit."""
    product, _ = make_pair(3, patch_size=64, block_size=8, with_detector=False, image_processor=None, max_batch=4)
    product.eval()
    patches, cur, positions = synth_tokens(3, 3, 64, 9, 4, 100)
    classes, masks = torch.tensor([3, 99, 0]), prefix_masks([3, 2, 1], 3)
    nxt = torch.randint(0, 9, (3, 3), generator=torch.Generator().manual_seed(7))
    got = ja.SupervisedTrainer(_sup_cfg(), product).eval_step(patches, cur, nxt, positions, masks, classes=classes)
    with torch.no_grad():
        logits, _ = product(patches, cur, classes, positions)
    torch.cuda.synchronize()
    print(f"largest difference of the two paths' logits: {float((logits - got['logits']).abs().max()):.3e}")
    assert logits.shape == got["logits"].shape == (3, 3, 9)
    assert torch.equal(logits, got["logits"])


def test_supervised_eval_limits_and_a_pending_backward():
    product, _ = make_pair(3, patch_size=64, block_size=8, with_detector=False, image_processor=None, max_batch=4)
    tr = ja.SupervisedTrainer(_sup_cfg(), product)
    patches, cur, positions = synth_tokens(5, 2, 64, 9, 4, 5)
    ones = torch.ones((5, 2))
    with pytest.raises(_lib.JnError, match="max_batch"):               # B above max_batch
        tr.eval_step(patches, cur, cur, positions, ones)
    patches, cur, positions = synth_tokens(1, 9, 64, 9, 4, 5)
    with pytest.raises(_lib.JnError, match="block size"):              # T above block_size
        tr.eval_step(patches, cur, cur, positions, torch.ones((1, 9)))
    # a train-mode forward whose backward is still pending: the validation pass takes the encoder's workspace, the
    # backward must then refuse (JN_ESTATE) instead of differentiating overwritten activations
    patches, cur, positions = synth_tokens(1, 4, 64, 9, 4, 6)
    product.train()
    logits, _ = product(patches, cur, torch.zeros(1, dtype=torch.long), positions)
    assert logits.grad_fn is not None
    tr.eval_step(patches, cur, cur, positions, torch.ones((1, 4)))
    with pytest.raises(Exception, match="code -5|overwritten"):
        logits.sum().backward()
    product.eval()


def test_supervised_eval_in_the_bf16_inference_mode():
    """bf16 is the inference mode: the validation pass runs in it, held to the mode's own bar (1e-3 on the logits against
    the fp32 oracle, test_bf16_mode_logits_and_rollout_golden)."""
    product, oracle = make_pair(3, patch_size=64, block_size=8, with_detector=False, image_processor=None, max_batch=4,
                                act_dtype="bf16")
    patches, cur, positions = synth_tokens(3, 5, 64, 9, 4, 100)
    classes, masks = torch.tensor([3, 99, 0]), prefix_masks([5, 2, 4], 5)
    nxt = torch.randint(0, 9, (3, 5), generator=torch.Generator().manual_seed(7))
    ref = _oracle_metrics(oracle, patches, cur, nxt, classes, positions, masks, "best-action")
    got = ja.SupervisedTrainer(_sup_cfg(), product).eval_step(patches, cur, nxt, positions, masks, classes=classes)
    assert (got["logits"].cpu() - ref["logits"]).abs().max() < 1e-3
    # the loss is 1-Lipschitz in the logits' max-norm up to the class weight: |d loss| <= 2 * w * |d logits|
    assert abs(float(got["metrics"][0]) - float(ref["loss"])) < 2 * STOP_W * 1e-3


# ---- 3. the detector's validation loss --------------------------------------------------------------------------------------
def _det_targets(N, P, nb=3):
    """The three boxes of test_detector_training_step_vs_oracle, scaled to the patch."""
    tg = torch.zeros((N, nb, 5))
    tg[0, 0] = torch.tensor([0, 10, 14, 60, 70.])
    tg[1, 0] = torch.tensor([0, 30, 30, 90, 64.])
    tg[1, 1] = torch.tensor([0, 4, 50, 30, 90.])
    tg[..., 1:] *= P / 128
    return tg


def _validation_ref(det, x, tg, chunk=None):
    """NeedleYOLOXRef in the reference's validation context (eval mode, no_grad), chunk by chunk; moves det's head statistics."""
    N = x.shape[0]
    chunk = chunk or N
    det.eval()
    outs, fpn, tot = [], [[], [], []], {k: 0.0 for k in LOSS_NAMES}
    with torch.no_grad():
        for i in range(0, N, chunk):
            o, f, lo = det(x[i:i + chunk], tg[i:i + chunk])
            assert not det.training
            outs += o
            for lvl in range(3):
                fpn[lvl].append(f[lvl])
            n = min(chunk, N - i)
            for k in LOSS_NAMES:
                tot[k] = tot[k] + float(lo[k]) * (n / N)
    return outs, [torch.cat(f) for f in fpn], tot


def _eval_head_raw(det, fpn):
    with torch.no_grad():
        return det.eval().head(fpn)                     # [n, A, 6] decoded: cx, cy, w, h, obj, cls


def _pair_iou(b):
    lt, rb = torch.maximum(b[:, None, :2], b[None, :, :2]), torch.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter, area = wh[..., 0] * wh[..., 1], (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area[:, None] + area[None] - inter)


def _robust_threshold(raws, stol=4e-3, nms_thr=0.45):
    """A confidence threshold at which the oracle's predictions are DECIDED, picked on the CPU from the eval-head outputs
    `raws` (a list of [n, A, 6]) of every call the test will compare: the widest gap of all their scores that (a) holds the
    band of _loose_box_match three times over (> 3 * stol, the margin test_reference_loop_with_detector_loss_... asks),
    (b) leaves boxes on at least two patches of every call and (c) passes no pair of boxes of one patch whose NMS verdict
    hangs on rounding: overlapping (IoU > nms_thr - 0.05) with scores closer than 1e-4, or an IoU within 2e-3 of nms_thr."""
    scores = [r[..., 4] * r[..., 5] for r in raws]
    v = torch.unique(torch.cat([s.flatten() for s in scores])).flip(0)
    second = min(float(s.max(dim=1).values.sort(descending=True).values[1]) for s in scores)
    for gap, i in sorted(((float(v[i] - v[i + 1]), i) for i in range(len(v) - 1)), reverse=True):
        thr = float((v[i] + v[i + 1]) / 2)
        if gap <= 3 * stol:
            break
        if thr + stol >= second:
            continue
        fragile = 0
        for r, s in zip(raws, scores):
            for n in range(r.shape[0]):
                keep = s[n] >= thr
                c, sc = r[n][keep], s[n][keep]
                b = torch.stack((c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2), 1)
                iou, ds = _pair_iou(b), (sc[:, None] - sc[None]).abs()
                upper = torch.triu(torch.ones_like(iou, dtype=torch.bool), 1)
                fragile += int((upper & (((iou > nms_thr - 0.05) & (ds < 1e-4)) | ((iou - nms_thr).abs() < 2e-3))).sum())
        if fragile == 0:
            return thr
    raise AssertionError("no decided threshold for these inputs")


def _bn_stats(sd, prefix):
    return {k: v for k, v in sd.items() if k.startswith(prefix) and (k.endswith("running_mean") or k.endswith("running_var"))}


def _check_losses(got, ref, tag=""):
    for k in LOSS_NAMES:
        r, v = float(ref[k]), float(got[k])
        print(f"{tag}{k}: {v} vs {r}")
        assert abs(v - r) < LOSS_BAR * max(1.0, abs(r)), (k, v, r)


@pytest.mark.parametrize("ip,P,N,n_head_stats", [("yolox-nano", 128, 2, 54), ("yolox-nano", 64, 4, 54), ("yolox-s", 96, 3, 30)])
def test_detector_validation_against_the_eval_mode_oracle(ip, P, N, n_head_stats):
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(31))
    tg = _det_targets(N, P)
    # on the CPU: the oracle's validation call on a copy, the eval-head scores it ends with, a threshold in their widest gap
    _, oracle0 = _detector_pair(P, 0.5, image_processor=ip, max_batch=N)
    dry = copy.deepcopy(oracle0.yolox)
    _, dry_fpn, _ = _validation_ref(dry, x, tg)
    thr = _robust_threshold([_eval_head_raw(dry, dry_fpn)])
    product, oracle = _detector_pair(P, thr, image_processor=ip, max_batch=N)
    det = oracle.yolox
    # the route the package took before: train-mode backbone.  It must lie more than ten bars from the validation route
    old = copy.deepcopy(det).train()
    with torch.no_grad():
        _, _, lo_old = old(x, tg)
    sd0 = {k: v.clone() for k, v in det.state_dict().items()}
    ref_out, ref_fpn, ref = _validation_ref(det, x, tg)
    assert abs(float(lo_old["total_loss"]) - ref["total_loss"]) > 10 * LOSS_BAR * max(1.0, abs(ref["total_loss"]))
    assert sum(o is not None for o in ref_out) >= 2
    sd1 = det.state_dict()
    assert all(torch.equal(sd0[k], sd1[k]) for k in _bn_stats(sd0, "backbone."))
    assert sum(not torch.equal(sd0[k], sd1[k]) for k in _bn_stats(sd0, "head.")) == n_head_stats == len(_bn_stats(sd0, "head."))

    before = _state(product)
    assert not product.training
    with torch.no_grad():
        outputs, fpn_outs, losses = product.yolox(x, tg)
    torch.cuda.synchronize()
    assert losses["total_loss"].grad_fn is None
    _check_losses(losses, ref)
    for lvl in range(3):
        assert fpn_outs[lvl].shape == ref_fpn[lvl].shape and (fpn_outs[lvl].cpu() - ref_fpn[lvl]).abs().max() < TOL_MAP, lvl
    for b in range(N):
        _loose_box_match(outputs[b], ref_out[b], thr, P)
        if outputs[b] is not None:
            assert outputs[b][:, :4].min() >= 0 and outputs[b][:, :4].max() <= P - 1
    assert sum(o is not None for o in outputs) >= 2
    # a following inference call sees the head statistics as the call left them (the BatchNorm table was rebuilt)
    eng = product.engine()
    with torch.no_grad():
        raw = det.eval().head(det.backbone(x))
    got_raw = torch.empty(raw.shape, device=DEV)
    boxes = torch.zeros((N, eng.cfg.max_det_per_patch, 7), device=DEV)
    counts = torch.zeros(N, device=DEV, dtype=torch.int32)
    check(eng.lib.jn_detect(eng.handle, ptr(x.to(DEV)), N, ptr(boxes), ptr(counts), ptr(got_raw),
                            _lib.current_stream(torch.device(DEV))), "jn_detect")
    torch.cuda.synchronize()
    assert (got_raw.cpu()[..., :4] - raw[..., :4]).abs().max() < 1e-3 * max(1.0, P / 64)      # the bars of
    assert (got_raw.cpu()[..., 4:] - raw[..., 4:]).abs().max() < 1e-5                         # test_detector_backbone_and_raw_head
    with torch.no_grad():
        ref_inf, _, _ = det(x)
    out_inf, _, _ = product.yolox(x)
    for b in range(N):
        _loose_box_match(out_inf[b], ref_inf[b], thr, P)
    # statistics: the backbone's untouched (bit for bit), every head statistic moved, and to where the oracle's moved
    after = _state(product)
    moved = 0
    for k in before:
        if k.startswith("yolox.head.") and k in _bn_stats(before, "yolox.head."):
            r = sd1[k[len("yolox."):]]
            assert (after[k] - r).abs().max() <= STAT_ATOL + STAT_RTOL * r.abs().max(), k
            assert ((after[k] - r).abs() <= STAT_ATOL + STAT_RTOL * r.abs()).all(), k
            moved += int(not torch.equal(before[k], after[k]))
        else:
            assert torch.equal(before[k], after[k]), k
    assert moved == n_head_stats


def test_detector_validation_in_chunks_of_max_batch():
    """N = 5 at max_batch 2: three engine calls weighted 2/5, 2/5, 1/5; the oracle chunk by chunk (the chunking deviation
    that training documents: statistics and the 1 / num_fg factor are per chunk)."""
    P, N = 64, 5
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(32))
    tg = _det_targets(N, P)
    tg[4, 2] = torch.tensor([0, 20., 8., 40., 40.])           # a box in the last chunk of one
    _, oracle0 = _detector_pair(P, 0.5, image_processor="yolox-nano", max_batch=2)
    dry = copy.deepcopy(oracle0.yolox)
    _, dry_fpn, _ = _validation_ref(dry, x, tg, chunk=2)
    thr = _robust_threshold([_eval_head_raw(dry, dry_fpn)])
    product, oracle = _detector_pair(P, thr, image_processor="yolox-nano", max_batch=2)
    ref_out, ref_fpn, ref = _validation_ref(oracle.yolox, x, tg, chunk=2)
    with torch.no_grad():
        outputs, fpn_outs, losses = product.yolox(x, tg)
    _check_losses(losses, ref, "chunked ")
    for lvl in range(3):
        assert (fpn_outs[lvl].cpu() - ref_fpn[lvl]).abs().max() < TOL_MAP, lvl
    # (every chunk's predictions come from the head statistics as THAT chunk left them; the oracle's list is built the same way)
    assert len(outputs) == N
    for b in range(N):
        _loose_box_match(outputs[b], ref_out[b], thr, P)
    # predict=False skips the eval head and the maps, the losses are the same call
    product2, oracle2 = _detector_pair(P, thr, image_processor="yolox-nano", max_batch=2)
    with torch.no_grad():
        out2, fpn2, losses2 = product2.yolox(x, tg, predict=False)
    assert out2 == [None] * N and fpn2 is None
    _check_losses(losses2, ref, "predict=False ")


def test_resident_training_pass_survives_the_validation_call():
    """jnroll.h: a resident detector training pass keeps its own workspace slot, the validation call works in the eval
    workspace: the pass's backward gives the gradient it gives without the call in between.  Two backwards of the same
    pass differ by the order of fp32 atomic sums only (1e-4 of the largest entry is a hundred times that); a backward
    through overwritten activations would be off by the gradient's own size."""
    P, N = 64, 4
    product, _ = _detector_pair(P, 0.5, image_processor="yolox-nano", max_batch=N)
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(31))
    tg = _det_targets(N, P)
    grads = []
    for validate in (False, True):
        product.train()
        _, _, l = product.yolox(x, tg, predict=False)
        assert l["total_loss"].grad_fn is not None
        if validate:
            product.eval()
            with torch.no_grad():
                _, _, lv = product.yolox(x, tg)
            assert abs(float(lv["total_loss"]) - float(l["total_loss"])) > 10 * LOSS_BAR * float(l["total_loss"])
        l["total_loss"].backward()
        torch.cuda.synchronize()
        named = {n: p for n, p in product.named_parameters() if n.startswith("yolox.") and p.grad is not None}
        grads.append({n: p.grad.detach().cpu().clone() for n, p in named.items()})
        for p in named.values():
            p.grad.zero_()
    product.eval()
    assert len(grads[0]) > 100 and grads[0].keys() == grads[1].keys()
    checked = 0
    for n, a in grads[0].items():
        scale = float(a.abs().max())
        if scale > 1e-10:
            assert float((grads[1][n] - a).abs().max()) <= 1e-4 * scale, n
            checked += 1
    assert checked > 100


@pytest.mark.parametrize("grad", [False, True])
def test_train_mode_call_keeps_the_train_mode_backbone(grad):
    """product.train(): with and without grad the loss branch runs PAFPN and head with batch statistics, as before; the
    backbone's running statistics move too.  So does eval mode with grad ENABLED."""
    P, N = 64, 4
    product, oracle = _detector_pair(P, 0.5, image_processor="yolox-nano", max_batch=N)
    x = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(31))
    tg = _det_targets(N, P)
    det = oracle.yolox.train()
    with torch.no_grad():
        _, _, ref = det(x, tg)
    ref = {k: float(ref[k]) for k in LOSS_NAMES}
    before = _state(product)
    product.train()
    with torch.set_grad_enabled(grad):
        _, _, losses = product.yolox(x, tg, predict=False)
    assert (losses["total_loss"].grad_fn is not None) == grad
    _check_losses(losses, ref, f"train grad={grad} ")
    after = _state(product)
    stats = _bn_stats(before, "yolox.backbone.")
    assert len(stats) > 100 and all(not torch.equal(before[k], after[k]) for k in stats)
    product.eval()
    if grad:                         # eval mode, grad enabled: still the train-mode backbone (a second step of its statistics)
        _, _, l2 = product.yolox(x, tg, predict=False)
        assert l2["total_loss"].grad_fn is not None
        _check_losses(l2, ref, "eval grad ")
        again = _state(product)
        assert all(not torch.equal(again[k], after[k]) for k in stats)


def test_compute_yolo_metrics_on_the_device_equals_the_host():
    product, _ = make_pair(3, patch_size=64, block_size=4, image_processor="yolox-nano", max_batch=4)
    tr = ja.SupervisedTrainer(_sup_cfg(), product)
    box = lambda x1, y1, x2, y2, s: torch.tensor([[x1, y1, x2, y2, s, 1.0, 0.0]], device=DEV)
    tg = torch.zeros((1, 3, 2, 6), device=DEV)
    none = [[box(1, 1, 9, 9, 0.9), None, None]]
    assert float(tr.compute_yolo_metrics(none, tg)["map"]) == 0.0
    tg[0, 0, 0] = torch.tensor([0, 2., 2., 20., 20., 1.])
    tg[0, 2, 1] = torch.tensor([0, 30., 30., 50., 60., 1.])
    cases = {"perfect": [[box(2, 2, 20, 20, 0.9), None, box(30, 30, 50, 60, 0.8)]],
             "swapped": [[box(30, 30, 50, 60, 0.8), None, box(2, 2, 20, 20, 0.9)]],
             "missed": [[box(2, 2, 20, 20, 0.9), None, None]],
             "false positive first": [[torch.cat((box(40, 40, 60, 60, 0.95), box(2, 2, 20, 20, 0.9))), None, box(30, 30, 50, 60, 0.8)]]}
    want = {"perfect": 1.0, "swapped": 0.0, "missed": 51 / 101}
    for name, outs in cases.items():
        dev_v = tr.compute_yolo_metrics(outs, tg)["map"]
        host_v = tr.compute_yolo_metrics([[None if o is None else o.cpu() for o in outs[0]]], tg.cpu(), device_metrics=False)["map"]
        assert dev_v.is_cuda and dev_v.dtype == torch.float32
        assert float(dev_v) == pytest.approx(float(host_v), abs=1e-6), name
        if name in want:
            assert float(dev_v) == pytest.approx(want[name], abs=1e-6), name
        else:
            assert 0.0 < float(dev_v) < 1.0
    packed = detection.pack_boxes(cases["perfect"][0], 7, torch.device(DEV))
    assert float(tr.compute_yolo_metrics(packed, tg)["map"]) == pytest.approx(1.0, abs=1e-6)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------
E2E = dict(P=64, T=5, n_images=4, batch_size=2, max_batch=4, seed=21, model_seed=7)


def _e2e_pair(thr):
    product, oracle = make_pair(E2E["model_seed"], patch_size=E2E["P"], block_size=E2E["T"], image_processor="yolox-nano",
                                gpt_backbone="yolox-nano", detector_conf_threshold=thr, max_batch=E2E["max_batch"],
                                max_det_per_patch=512)
    with torch.no_grad():                       # spread the scores, as _detector_pair does
        for k in range(3):
            oracle.yolox.head.cls_preds[k].weight.mul_(40.0)
            oracle.yolox.head.obj_preds[k].weight.mul_(40.0)
            oracle.yolox.head.reg_preds[k].weight.mul_(8.0)
    product.load_state_dict(oracle.state_dict())
    return product, oracle


def _e2e_cfg(loss_mode):
    return _sup_cfg(loss_mode, max_seq_len=E2E["T"], patch_size=E2E["P"], seed=0, detection_enabled=True)


def _oracle_batch(oracle, tr, loss_mode):
    """One batch of eval_supervised on the oracle: the statements of src/supervised.py:442-476 on the given trajectories;
    the detector in chunks of max_batch like the product.  Moves the oracle's head statistics."""
    c = lambda k: tr[k].cpu()
    sup = _oracle_metrics(oracle.eval(), c("patches"), c("current_actions"), c("next_actions"), c("class_id"), c("positions"),
                          c("masks"), loss_mode)
    outs, _, yolo = _validation_ref(oracle.yolox, c("patches_yolox"), c("bboxes_yolox")[..., :5], chunk=E2E["max_batch"])
    oracle.eval()
    return sup, outs, yolo


def test_eval_supervised_on_images_end_to_end():
    P, T, n_img, bs = E2E["P"], E2E["T"], E2E["n_images"], E2E["batch_size"]
    images, bboxes, _ = synth_batch(n_img, 3, 3, P, seed=8)
    class_ids = torch.tensor([0, 3, 99, 1])
    # dry run on the CPU (the walks are host work and seeded): the eval-head scores of every detector call both runs will
    # make, in order, and a confidence threshold in their widest common gap
    product0, oracle0 = _e2e_pair(0.5)
    dry_tr = ja.SupervisedTrainer(_e2e_cfg("best-action"), product0)
    trajectories = [dry_tr.generate_trajectories({"image": images[i:i + bs], "bboxes": bboxes[i:i + bs], "class_id": class_ids[i:i + bs]},
                                                 seed=E2E["seed"] + i, use_views=False, seed_ties=True) for i in range(0, n_img, bs)]
    dry, raws = copy.deepcopy(oracle0), []
    for loss_mode in MODES:
        for tr in trajectories:
            px, bx = tr["patches_yolox"].cpu(), tr["bboxes_yolox"].cpu()[..., :5]
            for i in range(0, px.shape[0], E2E["max_batch"]):
                _, f, _ = _validation_ref(dry.yolox, px[i:i + E2E["max_batch"]], bx[i:i + E2E["max_batch"]])
                raws.append(_eval_head_raw(dry.yolox, f))
    assert max(t["patches_yolox"].shape[0] for t in trajectories) > E2E["max_batch"]          # the detector call is chunked
    thr = _robust_threshold(raws)
    product, oracle = _e2e_pair(thr)
    names = {"loss", "action_loss", "action_accuracy", "episode_length", "yolo_total_loss", "yolo_iou_loss", "yolo_conf_loss",
             "yolo_cls_loss", "yolo_l1_loss", "yolo_num_fg", "yolo_loss", "map"}
    for loss_mode in MODES:
        trainer = ja.SupervisedTrainer(_e2e_cfg(loss_mode), product)
        product.train()
        got = trainer.eval_supervised_on_images(images, bboxes, bs, class_ids=class_ids, seed=E2E["seed"])
        assert product.training                                          # the mode is restored
        product.eval()
        assert set(got) == names and all(len(v) == n_img // bs for v in got.values())
        assert len(trainer.last_eval_supervised) == n_img // bs
        for i, kept in enumerate(trainer.last_eval_supervised):
            tr = kept["trajectories"]
            for k in ("current_actions", "positions", "masks", "patches_yolox"):      # the seeded walks of the dry run
                assert torch.equal(tr[k].cpu(), trajectories[i][k].cpu()), k
            sup, outs, yolo = _oracle_batch(oracle, tr, loss_mode)
            assert sup["gap"] >= 1e-3, sup["gap"]
            row = {k: v[i] for k, v in got.items()}
            print(loss_mode, i, row)
            assert abs(row["action_loss"] - float(sup["loss"])) < 2e-4
            assert row["action_accuracy"] == float(sup["accuracy"]) and row["episode_length"] == float(sup["episode_length"])
            assert torch.equal(kept["labels"], sup["labels"])
            valid = tr["masks"].cpu() == 1
            assert torch.equal(kept["predicted"][valid], sup["pred"][valid])
            assert (kept["token_loss"] - sup["token_loss"]).abs().max() < 2e-4 * STOP_W
            for k in LOSS_NAMES:
                assert abs(row["yolo_" + k] - yolo[k]) < LOSS_BAR * max(1.0, abs(yolo[k])), (k, row["yolo_" + k], yolo[k])
            assert row["yolo_loss"] == row["yolo_total_loss"]
            assert row["loss"] == float(torch.tensor(row["action_loss"]) + torch.tensor(row["yolo_loss"]))
            # mAP-50 with every patch a unit: a step function of the score order and the hit flags, equal up to fp32
            # rounding once the kept boxes agree (the threshold sits in a gap of the scores)
            bx = tr["bboxes_yolox"].cpu()
            tgts = [p[p[:, -1] == 1][:, :5] for p in bx]
            assert row["map"] == pytest.approx(detection.map_50(outs, tgts), abs=1e-6)
    # equal seeds, equal walks: the trajectories and the decision-side numbers repeat bit for bit (the detector's do not:
    # every validation call moves the head statistics, as the reference's does)
    trainer = ja.SupervisedTrainer(_e2e_cfg("on-self-trajectory"), product)
    a = trainer.eval_supervised_on_images(images, bboxes, bs, class_ids=class_ids, seed=E2E["seed"])
    kept_a = trainer.last_eval_supervised
    b = trainer.eval_supervised_on_images(images, bboxes, bs, class_ids=class_ids, seed=E2E["seed"])
    for k in ("action_loss", "action_accuracy", "episode_length"):
        assert a[k] == b[k] == got[k], k
    for x, y in zip(kept_a, trainer.last_eval_supervised):
        assert torch.equal(x["token_loss"], y["token_loss"]) and torch.equal(x["labels"], y["labels"])
    assert not product.training


def test_test_on_images_assembles_the_metrics_of_test():
    P, T, n_img, bs = E2E["P"], E2E["T"], E2E["n_images"], E2E["batch_size"]
    images, bboxes, _ = synth_batch(n_img, 3, 3, P, seed=8)
    product, _ = _e2e_pair(0.2)
    trainer = ja.SupervisedTrainer(_e2e_cfg("best-action"), product)
    assert trainer.best_metric_history == [] and trainer.last_test_metrics is None
    m = trainer.test_on_images(list(images), bboxes, bs, seed=E2E["seed"])
    for k in ("loss", "action_loss", "action_accuracy", "episode_length", "yolo_total_loss", "yolo_loss", "map"):
        assert len(m["supervised_" + k]) == n_img // bs, k
    assert len(m["map"]) == n_img and len(m["prop_patches_found"]) == 2 * n_img          # eval_envs: per image, per walk
    assert trainer.last_test_metrics is m
    assert trainer.best_metric_history == [pytest.approx(sum(m["map"]) / n_img)]
    trainer.test_on_images(list(images), bboxes, bs, seed=E2E["seed"])
    assert len(trainer.best_metric_history) == 2
