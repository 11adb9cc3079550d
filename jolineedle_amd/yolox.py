"""``NeedleYOLOX`` — detector wrapper of the reference (src/models/yolox.py:15-120): inference branch
(``jn_detect``) and the training loss branch (``jn_detector_forward`` / ``jn_detector_backward`` behind an autograd
node, or ``jn_detector_step`` in one call), computed by libjnroll.so."""
from typing import List, Optional

import torch

from . import _lib
from ._lib import check, ptr

LOSS_NAMES = ("total_loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg")
MAX_BOXES_PER_PATCH = 8          # DL_MAXG of csrc/kernels_detloss.hip: boxes of one patch the loss kernel holds in LDS
MAX_BOXES_WIDE = 1024            # JN_DETLOSS_MAX_BOXES of include/jnroll.h: rows of `targets` the wide loss kernel accepts
DET_LOSS_BOXES = ("cap8", "all")  # box policies of the loss: jn_yolox_loss (MAX_BOXES_PER_PATCH) / jn_yolox_loss_wide (every box)


def check_box_cap(targets: torch.Tensor) -> None:
    """Refuses targets [N, nb, 5] (class, x1, y1, x2, y2) with more boxes in one patch than the loss kernel holds: the kernel
    would cut the patch to its first ``MAX_BOXES_PER_PATCH`` rows without a word, where the reference uses every row.  A
    box is a row whose (class, cx, cy, w, h) sum is positive, as the kernel counts them.  With nb <= 8 nothing is launched
    or read back; above, one reduction and one readback."""
    if targets.shape[1] <= MAX_BOXES_PER_PATCH:
        return
    t = targets
    rows = t[..., 0] + 0.5 * (t[..., 1] + t[..., 3]) + 0.5 * (t[..., 2] + t[..., 4]) + (t[..., 3] - t[..., 1]) + (t[..., 4] - t[..., 2])
    worst, patch = (rows > 0).sum(dim=1).max(dim=0)
    worst, patch = int(worst), int(patch)
    if worst > MAX_BOXES_PER_PATCH:
        raise ValueError(f"patch {patch} holds {worst} ground-truth boxes; the detector loss takes at most "
                         f"{MAX_BOXES_PER_PATCH} per patch")


def yolox_loss(raw: torch.Tensor, targets: torch.Tensor, patch_size: int, strides=(8, 16, 32), use_l1: bool = True,
               loss_scale: float = 1.0, boxes: str = "cap8"):
    """The detector's SimOTA loss on given predictor outputs (``jn_yolox_loss``, no engine): raw [N, A, 6] and targets
    [N, nb, 5] = (class, x1, y1, x2, y2) on the device.  Returns (d_raw [N, A, 6] = d loss / d raw before the
    1 / max(num_fg, 1) factor, metrics f32[8] in the order of ``LOSS_NAMES``, scale f32[1] = loss_scale / max(num_fg, 1)).
    ``boxes="all"`` (``jn_yolox_loss_wide``, A <= 8400, nb <= ``MAX_BOXES_WIDE``) uses every box of a patch, as the
    reference does; the default ``"cap8"`` raises ``ValueError`` on a patch with more than ``MAX_BOXES_PER_PATCH``."""
    if boxes not in DET_LOSS_BOXES:
        raise ValueError(f"boxes={boxes!r}: one of {DET_LOSS_BOXES}")
    entry = "jn_yolox_loss_wide" if boxes == "all" else "jn_yolox_loss"
    assert raw.is_cuda and raw.dim() == 3 and raw.shape[2] == 6 and targets.dim() == 3 and targets.shape[2] == 5
    assert targets.shape[0] == raw.shape[0]
    dev = raw.device
    raw = raw.to(torch.float32).contiguous()
    t = targets.to(dev, torch.float32).contiguous()
    N, A, nb = raw.shape[0], raw.shape[1], t.shape[1]
    if all(int(s) > 0 and patch_size % int(s) == 0 for s in strides):
        assert A == sum((patch_size // int(s)) ** 2 for s in strides), (A, patch_size, strides)
    if boxes != "all":
        check_box_cap(t)
    d_raw = torch.empty_like(raw)
    metrics = torch.zeros(8, device=dev)
    scale = torch.zeros(1, device=dev)
    check(getattr(_lib.load_library(), entry)(ptr(raw), ptr(t), N, nb, int(patch_size), *(int(s) for s in strides),
                                              int(bool(use_l1)), float(loss_scale), ptr(d_raw), ptr(metrics), ptr(scale),
                                              _lib.current_stream(dev)), entry)
    return d_raw, metrics, scale


DET_CANDIDATES = ("first2048", "all")      # candidate policies of the stage: jn_postprocess / jn_postprocess_all


def postprocess(raw: torch.Tensor, conf: float, nms_thr: float, patch_size: int, max_out: int, candidates: str = "first2048"):
    """The detector's threshold / sort / NMS / clamp stage on given decoded predictions (``jn_postprocess``, no engine):
    raw [N, A, 6] = (cx, cy, w, h, obj, cls) on the device, finite, w and h >= 0.  Returns (boxes [N, max_out, 7] zero
    beyond the count, counts int32 [N], stats int32 [N, 2] = anchors with obj * cls >= conf before the 2048-candidate cap,
    NMS survivors before ``max_out``): ``stats[:, 0] > 2048`` or ``stats[:, 1] > max_out`` says a cap cut the patch.
    ``candidates="all"`` (``jn_postprocess_all``, A <= 8400) has no candidate cap: every passing anchor reaches the NMS."""
    if candidates not in DET_CANDIDATES:
        raise ValueError(f"candidates={candidates!r}: one of {DET_CANDIDATES}")
    entry = "jn_postprocess_all" if candidates == "all" else "jn_postprocess"
    assert raw.is_cuda and raw.dim() == 3 and raw.shape[2] == 6
    dev = raw.device
    raw = raw.to(torch.float32).contiguous()
    N, A = raw.shape[0], raw.shape[1]
    boxes = torch.zeros((N, max(int(max_out), 0), 7), device=dev)
    counts = torch.zeros((N,), device=dev, dtype=torch.int32)
    stats = torch.zeros((N, 2), device=dev, dtype=torch.int32)
    check(getattr(_lib.load_library(), entry)(ptr(raw), N, A, float(conf), float(nms_thr), float(patch_size - 1), int(max_out),
                                              ptr(boxes), ptr(counts), ptr(stats), _lib.current_stream(dev)), entry)
    return boxes, counts, stats


class _DetectorGraph(torch.autograd.Function):
    """Graph node behind ``losses["total_loss"]`` of ``NeedleYOLOX.forward(patches, targets)`` in grad mode (SURVEY.md §8b;
    src/models/yolox.py:58-73 returns a differentiable loss, src/reinforce.py:336-341 adds it to the policy loss before ONE
    ``backward()``).  backward = ``jn_detector_backward`` per resident pass with the upstream scalar torch hands over, then the
    engine's packed gradients are added to ``param.grad`` (reference layout)."""

    @staticmethod
    def forward(ctx, anchor, model, gen, total_loss, passes, keep):
        # `keep`: the patch / target chunks the engine's backward reads through raw pointers (stem weight gradient)
        ctx.model, ctx.gen, ctx.passes, ctx.keep = model, gen, passes, keep
        return total_loss.view_as(total_loss)

    @staticmethod
    def backward(ctx, dloss):
        model = ctx.model
        if ctx.gen != model._detector_gen:
            raise RuntimeError("backward through a detector forward whose activations were overwritten by a later training pass")
        eng, dev = model.engine(), model.device
        dloss = dloss.to(dev, torch.float32).contiguous()
        for index, weight in ctx.passes:
            check(eng.lib.jn_detector_backward(eng.handle, index, ptr(dloss), float(weight), _lib.current_stream(dev)),
                  "jn_detector_backward")
        model.publish_engine_grads()
        return None, None, None, None, None, None


class NeedleYOLOX:
    """View on the ``yolox.*`` part of a GPT's engine.

    ``forward(patches, targets=None) -> (outputs, fpn_outs, losses)`` as src/models/yolox.py:24-91.

    Without ``targets``: the inference branch (eval-mode BatchNorm), ``losses == {}``.

    With ``targets`` ([N, nb, 5 | 6] = class, x1, y1, x2, y2[, 1]; zero rows = padding): the engine runs PAFPN + head in
    train mode (batch-statistics BatchNorm, running statistics updated), the SimOTA assignment and the IoU / objectness /
    class / L1 losses, and — as the reference does after its loss branch (:74-91) — the eval-mode head on the same FPN
    maps, postprocess and clamp: ``outputs`` are those predictions, ``fpn_outs`` the three (train-mode) maps.  In grad
    mode ``losses["total_loss"]`` carries a graph whose backward is the engine's: the reference's statements
    ``loss += yolo_loss["total_loss"]; (loss / ga).backward()`` (src/reinforce.py:339-341, src/supervised.py:888-897) run
    as written, in either order with the policy loss's own backward.  The other entries of ``losses`` are values
    (the reference's loops only log them).  ``predict=False`` skips the eval head / maps (the loops discard them).

    At most ``MAX_BOXES_PER_PATCH`` = 8 boxes per patch: ``targets`` may be wider (padding rows), but a patch with more
    real rows raises ``ValueError`` (the loss kernel would drop the rest, the reference uses them all).
    Under the owning model's box policy "all" (``GPT.set_det_loss_boxes``, config field ``det_loss_boxes``) every box of
    a patch is used instead, as in the reference, and nothing raises up to ``MAX_BOXES_WIDE`` rows.

    A detection batch larger than ``max_batch`` is fed in chunks of ``max_batch``, each weighted by its share of the
    patches (deviation: BatchNorm statistics and the 1 / num_fg normalisation are per chunk); every chunk keeps its own
    workspace until the backward.

    Validation — the owning model in eval mode AND grad disabled, the context of the reference's ``eval_supervised``
    (src/supervised.py:407, 465 under ``model.eval()``): the PAFPN then runs in the module's mode, eval (running
    statistics, none written), and only the head goes to train mode for the loss, so the head's running statistics do
    move (src/models/yolox.py:54-62; ``jn_detector_eval_loss``); ``fpn_outs`` are the eval-mode maps.  Every other
    combination takes the path above: in particular eval mode WITH grad enabled still runs the train-mode backbone.
    """

    def __init__(self, gpt, conf_threshold: float):
        self._gpt = gpt
        self.conf_threshold = conf_threshold

    def __call__(self, patches, targets=None, predict: bool = True):
        return self.forward(patches, targets, predict)

    def _check_boxes(self, t: torch.Tensor) -> None:
        if self._gpt.det_loss_boxes != "all":                      # under "all" the engine uses every box: nothing to refuse
            check_box_cap(t)

    def _boxes_to_list(self, boxes, counts) -> List[Optional[torch.Tensor]]:
        cnt = counts.tolist()
        return [boxes[i, :c].clone() if c > 0 else None for i, c in enumerate(cnt)]

    def forward(self, patches: torch.Tensor, targets: Optional[torch.Tensor] = None, predict: bool = True):
        g = self._gpt
        g.sync_weights()
        eng = g.engine()
        N = patches.shape[0]
        K = eng.cfg.max_det_per_patch
        x = patches.to(g.device, torch.float32).contiguous()
        if targets is None:
            boxes = torch.zeros((N, K, 7), device=g.device)
            counts = torch.zeros((N,), device=g.device, dtype=torch.int32)
            for i in range(0, N, g.max_batch):
                n = min(g.max_batch, N - i)
                check(eng.lib.jn_detect(eng.handle, ptr(x[i:i + n]), n, ptr(boxes[i:i + n]), ptr(counts[i:i + n]),
                                        None, _lib.current_stream(g.device)), "jn_detect")
            fpn_outs = g.backbone_features(x, _lib.JN_NET_DETECTOR)
            return self._boxes_to_list(boxes, counts), fpn_outs, {}
        # ---- loss branch + eval head (src/models/yolox.py:58-91) ----
        assert targets.shape[0] == N and targets.shape[-1] >= 5
        t = targets[..., :5].to(g.device, torch.float32).contiguous()
        self._check_boxes(t)
        graph = torch.is_grad_enabled()
        if not g.training and not graph:
            return self._validation_forward(x, t, predict)
        if graph:
            g.bind_flat()
        g._detector_gen = getattr(g, "_detector_gen", 0) + 1
        cfg = eng.cfg
        P = g.patch_size
        boxes = counts = None
        fpn = [None, None, None]
        if predict:
            boxes = torch.zeros((N, K, 7), device=g.device)
            counts = torch.zeros((N,), device=g.device, dtype=torch.int32)
            chans = [int(256 * cfg.det_width), int(512 * cfg.det_width), int(1024 * cfg.det_width)]
            fpn = [torch.empty((N, c, P // s, P // s), device=g.device) for c, s in zip(chans, (8, 16, 32))]
        tot = {k: torch.zeros((), device=g.device) for k in LOSS_NAMES}
        starts = list(range(0, N, g.max_batch))
        passes, keep = [], []
        for index, i in enumerate(starts):
            n = min(g.max_batch, N - i)
            metrics = torch.zeros(8, device=g.device)
            xc, tc = x[i:i + n], t[i:i + n]
            check(eng.lib.jn_detector_forward(eng.handle, ptr(xc), n, ptr(tc), t.shape[1], index, len(starts), ptr(metrics),
                                              ptr(boxes[i:i + n]) if predict else None, ptr(counts[i:i + n]) if predict else None,
                                              *(ptr(f[i:i + n]) if predict else None for f in fpn),
                                              _lib.current_stream(g.device)), "jn_detector_forward")
            for j, k in enumerate(LOSS_NAMES):
                tot[k] = tot[k] + metrics[j] * (n / N)
            passes.append((index, n / N))
            keep.append((xc, tc))
        if graph:
            anchor = next(p for n_, p in g.named_parameters() if n_.startswith("yolox") and p.requires_grad)
            tot["total_loss"] = _DetectorGraph.apply(anchor, g, g._detector_gen, tot["total_loss"], passes, (x, t, keep))
        outputs = self._boxes_to_list(boxes, counts) if predict else [None] * N
        return outputs, (tuple(fpn) if predict else None), tot

    def _fpn_buffers(self, N: int):
        cfg, P, dev = self._gpt.engine().cfg, self._gpt.patch_size, self._gpt.device
        chans = [int(256 * cfg.det_width), int(512 * cfg.det_width), int(1024 * cfg.det_width)]
        return [torch.empty((N, c, P // s, P // s), device=dev) for c, s in zip(chans, (8, 16, 32))]

    def _validation_forward(self, x: torch.Tensor, t: torch.Tensor, predict: bool, packed: bool = False):
        """The loss branch as validation reaches it (src/supervised.py:465: ``model.eval()`` and ``no_grad``), through
        ``jn_detector_eval_loss``: eval-mode PAFPN, train-mode head.  No graph, no resident pass.  packed: the
        predictions stay on the device as (boxes [N, K, 7], counts int32 [N]) and nothing is read back."""
        g = self._gpt
        eng, dev = g.engine(), g.device
        N, K = x.shape[0], eng.cfg.max_det_per_patch
        boxes = counts = None
        fpn = [None, None, None]
        if predict:
            boxes = torch.zeros((N, K, 7), device=dev)
            counts = torch.zeros((N,), device=dev, dtype=torch.int32)
            fpn = self._fpn_buffers(N)
        tot = {k: torch.zeros((), device=dev) for k in LOSS_NAMES}
        for i in range(0, N, g.max_batch):
            n = min(g.max_batch, N - i)
            metrics = torch.zeros(8, device=dev)
            check(eng.lib.jn_detector_eval_loss(eng.handle, ptr(x[i:i + n]), n, ptr(t[i:i + n]), t.shape[1], ptr(metrics),
                                                ptr(boxes[i:i + n]) if predict else None, ptr(counts[i:i + n]) if predict else None,
                                                *(ptr(f[i:i + n]) if predict else None for f in fpn),
                                                _lib.current_stream(dev)), "jn_detector_eval_loss")
            for j, k in enumerate(LOSS_NAMES):
                tot[k] = tot[k] + metrics[j] * (n / N)
        if packed and predict:
            outputs = (boxes, counts)
        else:
            outputs = self._boxes_to_list(boxes, counts) if predict else [None] * N
        return outputs, (tuple(fpn) if predict else None), tot

    def validation_loss(self, patches: torch.Tensor, targets: torch.Tensor, predict: bool = True, packed: bool = False):
        """``forward(patches, targets)`` on the validation route whatever the modes are (``eval_supervised_on_images``
        puts the model in eval mode itself): (outputs, fpn_outs, losses), see the class docstring."""
        g = self._gpt
        g.sync_weights()
        assert targets.shape[0] == patches.shape[0] and targets.shape[-1] >= 5
        x = patches.to(g.device, torch.float32).contiguous()
        t = targets[..., :5].to(g.device, torch.float32).contiguous()
        self._check_boxes(t)
        return self._validation_forward(x, t, predict, packed)

    def loss_and_backward(self, patches: torch.Tensor, targets: torch.Tensor, loss_scale: float = 1.0) -> dict:
        """Loss branch of src/models/yolox.py:58-73 AND ``(loss_scale * total_loss).backward()`` in one engine call
        (``jn_detector_step``): the fast path of ``train_iteration``.  Returns the reference's loss dict (device scalars, no
        graph); the yolox.* gradients are accumulated in the engine's gradient arena."""
        g = self._gpt
        g.sync_weights()
        eng = g.engine()
        N = patches.shape[0]
        assert targets.shape[0] == N and targets.shape[-1] >= 5
        x = patches.to(g.device, torch.float32).contiguous()
        t = targets[..., :5].to(g.device, torch.float32).contiguous()
        self._check_boxes(t)
        tot = {k: torch.zeros((), device=g.device) for k in LOSS_NAMES}
        for i in range(0, N, g.max_batch):
            n = min(g.max_batch, N - i)
            metrics = torch.zeros(8, device=g.device)
            check(eng.lib.jn_detector_step(eng.handle, ptr(x[i:i + n]), n, ptr(t[i:i + n]), t.shape[1],
                                           float(loss_scale) * n / N, ptr(metrics), _lib.current_stream(g.device)),
                  "jn_detector_step")
            for j, k in enumerate(LOSS_NAMES):
                tot[k] = tot[k] + metrics[j] * (n / N)
        if getattr(g, "_flat_grads", None) is not None and getattr(g, "_publish_detector_grads", True):
            g.publish_engine_grads()                   # bound model (autograd bridge): yolox.*.grad follow at once
        return tot

    @staticmethod
    def clamp_outputs(outputs, image_size: int):
        """src/models/yolox.py:93-113."""
        for b in outputs:
            if b is not None:
                b[:, :4].clamp_(min=0, max=image_size - 1)
        return outputs
