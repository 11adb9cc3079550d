"""``SupervisedTrainer`` — the teacher-forced training step of the reference
(src/supervised.py:138-177 loss, :863-902 step) over ``jn_supervised_step``, fed by teacher trajectories
(``generate_trajectories``, src/supervised.py:95-136, over trajectory.NeedleSimpleEnv) whose patches are gathered on
the device, and followed by the detector step on the trajectories' detector patches (src/supervised.py:881-902).
``eval_on_images`` is the free-running half of ``test()`` (src/supervised.py:279-405) on the engine's rollout and
``eval_envs_on_images`` the multistart evaluation that selects the best checkpoint (``eval_envs``, :638-752);
``eval_supervised_on_images`` is the teacher-forced validation (``eval_supervised``, :407-483) over ``jn_supervised_eval``
and the detector's validation loss, and ``test_on_images`` the metric assembly of ``test()`` (:754-810); augmentation is
opt-in (``init_detection``)."""
import ctypes as C
import random
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr
from .rollouts import RolloutRunner
from .trainer import Trainer


def reference_actions(current_actions: torch.Tensor, next_actions: torch.Tensor, masks: torch.Tensor,
                      loss_mode: str = "best-action") -> torch.Tensor:
    """The labels of a teacher-forced batch (src/supervised.py:449-458, 870-877): ``next_actions``, or with
    ``loss_mode == "on-self-trajectory"`` the action the trajectory itself takes next — ``current_actions`` shifted left by
    one, with column n_b - 1 of row b (n_b = the row's mask sum) taken from ``next_actions``; a row without tokens
    addresses column -1, the last one, as the reference's index does."""
    if loss_mode != "on-self-trajectory":
        return next_actions
    ref = torch.zeros_like(current_actions)
    ref[:, :-1] = current_actions[:, 1:]
    last = masks.sum(dim=1).long() - 1
    rows = torch.arange(current_actions.shape[0], device=current_actions.device)
    ref[rows, last] = next_actions[rows, last]
    return ref


class SupervisedTrainer(Trainer):
    def __init__(self, config, model, logger=None, train_dataset=None, test_dataset=None, rank: int = 0):
        Trainer.__init__(self, config, model, logger, train_dataset, test_dataset, rank)
        self.stop_weight = float(getattr(config, "stop_weight", 1.0)) if getattr(config, "stop_enabled", False) else 1.0
        self.best_metric_name = "map"
        self.best_metric_history = []
        self.last_test_metrics = None
        self._flat_grads = None
        self._device_walks = 0          # calls of the device route of generate_trajectories: its default seeds move on
        self._runner = None             # ``_eval_runner``'s, built on first use

    def generate_trajectories(self, batch: Dict, position: Optional[Tuple[int, int]] = None, seed: Optional[int] = None,
                              use_views: bool = True, seed_ties: bool = False, device: Optional[bool] = None) -> Dict:
        """One teacher walk per image of `batch` (``image`` [B, C, H, W] on the device or a list of [C, H, W] of one
        size, ``bboxes`` [B, nb, 4] xyxy with zero-row padding or a list, ``class_id``) -> the collated dict of
        src/supervised.py:95-136: patches [B, T, C, P, P], current_actions / next_actions / labels [B, T],
        positions [B, T, 2], masks [B, T], local_bboxes [B, T, nb, 6], patches_yolox [M, C, P, P], bboxes_yolox
        [M, nb, 6], class_id [B].  The walks are integer work on the host; both patch tensors come from the
        device-resident images in two gather launches.  `seed` makes the walks reproducible (the reference seeds
        nothing here).  use_views=False leaves the rotations / translations of the config off (``test()`` disables
        both, src/supervised.py:773-774).  seed_ties: with a `seed`, the teacher's choice among equally near targets
        (Python's global ``random`` in the reference and by default here) is drawn from ``random.Random(seed + i)`` too, so
        that equal seeds give equal walks whatever else drew from the global stream.

        device (None: ``config.device_trajectories``, default False): the walks of the whole batch come from ONE
        ``trajectory.teacher_walks_device`` call (``jn_teacher_walks``) on the boxes uploaded once, and its positions, masks
        and detector cells feed the two gathers without a host check.  The rule is ``trajectory.teacher_walks``: the
        env's walk on two Philox streams of (`seed`, image index) instead of numpy's and Python's, so
        the walks differ from the host route's; seed=None uses ``config.seed * 1000003 +`` the number of such calls this
        trainer has made; `seed_ties` has no meaning here (ties always come from the seed).  The box outputs keep the
        batch's nb columns, the real rows first."""
        from .trajectory import NeedleSimpleEnv, assemble_samples
        cfg = self.config
        if device is None:
            device = bool(getattr(cfg, "device_trajectories", False))
        images = batch["image"]
        if not isinstance(images, torch.Tensor):
            images = torch.stack(list(images))
        if getattr(cfg, "uint8_images", False) and images.dtype == torch.uint8:
            images = images.to(self.device).contiguous()          # the bytes, gathered as byte / 255
        else:
            images = images.to(self.device, torch.float32).contiguous()
        P = int(cfg.patch_size)
        # --augment-rotate / --augment-translate (src/dataset.py:274-278): the teacher walks the transformed boxes on the
        # views' canvas and both patch tensors are cut through the views; the augmented images are never written
        views, boxes = None, batch["bboxes"]
        if use_views and (getattr(cfg, "rotations", False) or getattr(cfg, "translations", False)):
            from .views import stack_bboxes, trainer_views
            views = trainer_views(self, images, boxes, P)
            boxes = views.transform_bboxes(stack_bboxes(boxes, images.shape[0]))
        self.last_views = views
        height, width = views.canvas if views is not None else images.shape[2:]
        if device:
            return self._device_trajectories(batch, images, views, boxes, int(height) // P, int(width) // P, position, seed)
        idx = []
        for i in range(images.shape[0]):
            bb = boxes[i]
            if isinstance(bb, torch.Tensor):
                bb = bb[(bb != 0).any(dim=-1)] if bb.numel() else bb.reshape(0, 4)      # drop the collate's zero rows
            ties = random.Random(seed + i) if seed_ties and seed is not None else None
            env = NeedleSimpleEnv(None, P, bb, seed=None if seed is None else seed + i, height=height, width=width, py_random=ties)
            idx.append(env.generate_sample_indices(int(cfg.max_seq_len), int(getattr(cfg, "min_keypoints", 0)),
                                                   int(getattr(cfg, "max_keypoints", 0)),
                                                   bool(getattr(cfg, "binomial_keypoints", False)), position))
        out = assemble_samples(images, list(range(images.shape[0])), idx, P, views=views)
        cid = batch.get("class_id")
        out["class_id"] = (torch.as_tensor(cid) if cid is not None else torch.zeros(images.shape[0], dtype=torch.long)).to(self.device, torch.long)
        return out

    def _device_trajectories(self, batch: Dict, images, views, boxes, gh: int, gw: int, position, seed) -> Dict:
        """The device route of ``generate_trajectories``: `boxes` are the batch's (a tensor or a list) or, with views, the
        transformed ones on the canvas of gh x gw cells."""
        from .trajectory import gather_indexed, teacher_walks_device
        from .views import stack_bboxes
        cfg, dev = self.config, self.device
        B, P, T = int(images.shape[0]), int(cfg.patch_size), int(cfg.max_seq_len)
        self._device_walks += 1
        if seed is None:
            seed = int(getattr(cfg, "seed", 0)) * 1000003 + self._device_walks
        starts = None
        if position is not None:
            starts = torch.tensor([[int(position[0]), int(position[1])]] * B, dtype=torch.int64).reshape(B, 2)
        empty = isinstance(boxes, torch.Tensor) and boxes.numel() == 0
        bb = (torch.zeros((B, 0, 4), dtype=torch.int64) if empty else stack_bboxes(boxes, B)).to(dev)     # the one upload
        w = teacher_walks_device(bb, gh, gw, P, T, int(getattr(cfg, "min_keypoints", 0)), int(getattr(cfg, "max_keypoints", 0)),
                                 bool(getattr(cfg, "binomial_keypoints", False)), seed, start_positions=starts)
        # masked steps read image -1: zero patches, like the host route's (valid by construction: no host check)
        image = torch.arange(B, device=dev, dtype=torch.int64)[:, None].expand(B, T)
        ii = torch.where(w["masks"] > 0, image, torch.full_like(image, -1)).reshape(-1)
        patches = gather_indexed(images, ii, w["positions"].reshape(-1, 2), P, views=views, _check_positions=False)
        cells = w["cells_yolox"]
        out = {"patches": patches.view(B, T, *patches.shape[1:]),
               "patches_yolox": gather_indexed(images, cells[:, 0].contiguous(), cells[:, 1:].contiguous(), P, views=views,
                                               _check_positions=False),
               "bboxes_yolox": w["bboxes_yolox"]}
        for k in ("current_actions", "next_actions", "positions", "masks", "labels", "local_bboxes"):
            out[k] = w[k]
        cid = batch.get("class_id")
        out["class_id"] = (torch.as_tensor(cid) if cid is not None else torch.zeros(B, dtype=torch.long)).to(dev, torch.long)
        return out

    def train_iteration(self, batch: Dict, optimizer_step: bool = True, process_group=None, seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Loop body of src/supervised.py:844-902 without augmentation: trajectories -> teacher-forced step (CE loss,
        backward) -> detector loss + backward on the trajectories' detector patches -> AdamW on both groups."""
        cfg = self.config
        tr = self.generate_trajectories(batch, seed=seed)
        cur, nxt, masks = tr["current_actions"], tr["next_actions"], tr["masks"]
        ref_actions = reference_actions(cur, nxt, masks, getattr(cfg, "loss_mode", "best-action"))   # src/supervised.py:870-877
        detection = self.yolox_model() is not None and bool(getattr(cfg, "detection_enabled", True))
        aug = self.detection_augment
        if aug is not None:
            B_, T_ = cur.shape
            tr["patches"] = aug(tr["patches"].flatten(0, 1)).view(B_, T_, *tr["patches"].shape[2:])
            tr["patches_yolox"] = aug(tr["patches_yolox"])
        res = self.train_step(tr["patches"], cur, ref_actions, tr["positions"], masks, optimizer_step=False, classes=tr["class_id"])
        ga = int(getattr(cfg, "gradient_accumulation", 1))
        if detection:
            yolo = self.model.yolox.loss_and_backward(tr["patches_yolox"], tr["bboxes_yolox"], loss_scale=1.0)
            for k, v in yolo.items():
                res["yolo_" + k] = v
            res["loss"] = res["loss"] + yolo["total_loss"].cpu()
        if optimizer_step and self.iter_num % ga == 0:
            self._engine_optimizer_step(0.0, detection, process_group)     # (0.0: no clipping, as in ``train_step``)
        res["trajectories"] = tr
        return res

    # ---- the reference's supervised loop on the autograd bridge (src/supervised.py:138-198, 812-911) -------------------
    def compute_metrics(self, action_logits, actions, masks, yolo_loss: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """src/supervised.py:138-198: CrossEntropy(weight[STOP] = stop_weight, reduction none) over the non-padding tokens,
        accuracy, the detector's loss terms under ``yolo_*`` and their total added to ``loss``, ``episode_length``."""
        nA = action_logits.shape[-1]
        weight = torch.ones(nA, device=action_logits.device)
        if getattr(self.config, "stop_enabled", False):
            weight[-1] = self.stop_weight
        flat, target = action_logits.reshape(-1, nA), actions.flatten()
        valid = (masks == 1).flatten()
        per_token = torch.nn.functional.cross_entropy(flat, target, weight=weight, reduction="none")
        metrics = {"action_loss": per_token[valid].mean(),
                   "action_accuracy": (target[valid] == flat.argmax(dim=1)[valid]).float().mean()}
        metrics["loss"] = metrics["action_loss"]
        if yolo_loss is not None:
            for k, v in yolo_loss.items():
                metrics["yolo_" + k] = v if isinstance(v, torch.Tensor) else torch.tensor(v)
            metrics["yolo_loss"] = metrics["yolo_total_loss"]
            metrics["loss"] = metrics["loss"] + metrics["yolo_loss"].to(metrics["loss"].device)
        if torch.isnan(metrics["action_accuracy"]):
            metrics["action_accuracy"] = torch.zeros((), device=action_logits.device)
        metrics["episode_length"] = masks.sum(dim=1).float().mean()
        return metrics

    def training_step(self, batch: Dict, optim_gpt, optim_yolox=None, seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The body of the reference's loop (src/supervised.py:834-902): trajectories -> [augmentation] ->
        ``model(patches, current_actions, classes, positions)`` -> reference actions -> detector loss -> compute_metrics
        -> ``loss.backward()`` -> every ga-th iteration ``optim.step()`` / ``zero_grad()`` (no clipping).  ``model`` is this
        package's GPT in train mode: the logits carry a graph whose backward is the engine's, and so does the detector's
        ``total_loss`` (``yolox.py::_DetectorGraph``): ONE ``loss.backward()`` runs both; the optimisers average the gradients over the ranks with ONE all-reduce of the flat buffer each
        (the job DDP's bucketed all-reduce does in the reference, src/supervised.py:815)."""
        cfg, model = self.config, self.model
        self.iter_num += 1
        model.train()
        batch = self.generate_trajectories(batch, seed=seed)
        patches, current_actions, next_actions = batch["patches"], batch["current_actions"], batch["next_actions"]
        positions, masks, classes = batch["positions"], batch["masks"], batch["class_id"]
        aug = self.detection_augment
        if aug is not None:
            with torch.no_grad():
                B_, T_ = current_actions.shape
                patches = aug(patches.flatten(0, 1)).view(B_, T_, *patches.shape[2:])
        action_logits, _ = model(patches, current_actions, classes=classes, positions=positions)
        ref_actions = reference_actions(current_actions, next_actions, masks, getattr(cfg, "loss_mode", "best-action"))
        yolo_loss = None
        if self.yolox_model() is not None and bool(getattr(cfg, "detection_enabled", True)):
            patches_yolox = batch["patches_yolox"]
            if aug is not None:
                with torch.no_grad():
                    patches_yolox = aug(patches_yolox)
            _, _, yolo_loss = self.yolox_model()(patches_yolox, batch["bboxes_yolox"], predict=False)   # :881-888; total_loss has a graph
        metrics = self.compute_metrics(action_logits, ref_actions, masks, yolo_loss)
        metrics["loss"].backward()
        if self.iter_num % int(getattr(cfg, "gradient_accumulation", 1)) == 0:
            optim_gpt.step()
            if optim_yolox is not None:
                optim_yolox.step()
            optim_gpt.zero_grad()
            if optim_yolox is not None:
                optim_yolox.zero_grad()
        return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in metrics.items()}

    def run(self, rank: int, world_size: int, port: int, batches=None, max_iters: int = None, backend: str = None,
            seed: Optional[int] = None):
        """``SupervisedTrainer.run`` (src/supervised.py:812-911) without the dataset / Visdom / test plumbing (out of scope,
        SURVEY.md §8): `batches` is any iterable of collated batches ({"image", "bboxes"[, "class_id"]}), re-iterated when
        exhausted.  One process per GPU; gradients are averaged by the optimisers' all-reduce (DDP semantics), BatchNorm
        statistics stay per rank.  Returns the metrics of the last iteration."""
        def step(i, batch, optim_gpt, optim_yolox):
            return self.training_step(batch, optim_gpt, optim_yolox, seed=None if seed is None else seed + i)
        return self._run_loop(step, rank, world_size, port, backend, batches, max_iters,
                              augment=bool(getattr(self.config, "augment_detection", False)), sync_gradients=world_size > 1)

    # ---- evaluation: the free-running half of test() (src/supervised.py:279-405, 407-470) ------------------------------
    def _eval_runner(self) -> RolloutRunner:
        """A ``RolloutRunner`` over this trainer's model, walking ``test_max_seq_len`` steps.  Kept between calls so that
        its rollout counter (start positions, sampling seeds) moves on like a loop's."""
        if self._runner is None:
            cfg = self.config
            self._runner = RolloutRunner(self.model, int(getattr(cfg, "test_max_seq_len", None) or cfg.max_seq_len),
                                         bool(getattr(cfg, "stop_enabled", False)), int(getattr(cfg, "seed", 0)), self.rank,
                                         action_mask=getattr(cfg, "action_mask", None))
        return self._runner

    @torch.no_grad()
    def eval_on_images(self, images, bboxes, batch_size: int, sample_actions: bool = False, do_detection: bool = None,
                       merge_bboxes: bool = None, device_metrics: bool = False, streams: str = "loop",
                       class_ids=None, action_mask: str = None) -> Dict[str, list]:
        """The free-running half of the reference's ``test()``: ``test_model_on_env`` (src/supervised.py:279-405) lets the
        policy walk one image, calling the full-sequence forward again at every step, and compares every chosen action
        with the teacher's ``best_action``.  Here the walks are the engine's rollouts with the token of step t at 1-D
        position t (``token_positions="sequence"``: the KV-cached step computes the last row of that full forward),
        `batch_size` images at a time with the chunking, start positions and detection metrics of
        ``ReinforceTrainer.eval_on_images``, for ``config.test_max_seq_len`` steps; the teacher's opinion of every
        visited state is computed inside the rollout (``jn_set_rollout_teacher``) on the simple env's target cells
        (``trajectory.simple_env_targets``, built on the host per image, uploaded once per chunk).

        Returns per-image lists: `prop_patches_found` (target cells visited / target cells, 0 without targets),
        `episode_length` (the image's own executed steps), with detection `map` and the `yolo_*` entries,
        `teacher_agreement` (share of the own steps with a non-empty teacher set whose action is a member of it; 0 when
        there is none) and `stopped_inside_bbox` (the final cell is a target cell).  No REINFORCE losses;
        ``last_return_values`` of no trainer is touched.  ``self.last_eval_rollouts`` keeps, per image, the small
        part of its walk on the host (actions, positions, logits, teacher_sets, teacher_targets).  With sample_actions
        every walk samples from the stream of its own rollout of the per-image loop (``ragged.walk_agent_keys``), so
        the result does not depend on `batch_size`; streams="batch" keeps the draws keyed by the place in the chunk.
        `class_ids`: one class per image (a tensor or a sequence): the class token of image i's walk is row class_ids[i]
        of ``embed_class``, as ``test_model_on_env`` feeds ``classes=sample["class_id"]`` at every step
        (src/supervised.py:284, 317-331); None = class 0 for every walk.
        `action_mask`: "grid" / "unvisited" / None (``config.action_mask``), see ``RolloutRunner.rollout``.
        Deviations from the reference: DESIGN.md §6."""
        from .ragged import eval_image_chunks
        if do_detection is None:
            do_detection = bool(getattr(self.config, "detection_enabled", True)) and self.yolox_model() is not None
        if merge_bboxes is None:
            merge_bboxes = bool(getattr(self.config, "merge_bboxes", False))
        chunks = self._eval_walks(images, bboxes, batch_size, do_detection, sample_actions=sample_actions, streams=streams,
                                  class_ids=class_ids, action_mask=action_mask)
        return self._walk_metrics(eval_image_chunks(self._eval_runner(), self.yolox_model() if do_detection else None, chunks,
                                                    do_detection, merge_bboxes, device_metrics))

    def _eval_walks(self, images, bboxes, batch_size, do_detection, **kw):
        """The free-running walks of both evaluations, as chunk records: ``ragged.rollout_chunks`` of the eval runner in
        sequence-position mode with the teacher armed on the simple env's target cells; the model is in eval mode
        (src/supervised.py:294) until the last record has been taken."""
        from .ragged import rollout_chunks
        from .trajectory import simple_env_targets
        P = int(self.config.patch_size)
        rows = [torch.as_tensor(b).reshape(-1, 4).to(torch.long) for b in bboxes]

        def target_grids(rows, extents, canvas):
            grid = torch.zeros((len(rows), *canvas), dtype=torch.uint8)
            for b, (r, (gh, gw)) in enumerate(zip(rows, extents)):
                grid[b, :gh, :gw] = simple_env_targets(r, gh * P, gw * P, P)
            return grid

        with self._eval_mode():
            yield from rollout_chunks(self._eval_runner(), images, rows, batch_size, do_detection=do_detection,
                                      token_positions="sequence", teacher_targets=target_grids, **kw)

    def _walk_metrics(self, per_walk: list) -> Dict[str, list]:
        """The per-walk entries of ``eval_on_images`` from the per-walk (tail, rollout) pairs; fills ``last_eval_rollouts``."""
        from .trajectory import teacher_agreement
        out: Dict[str, list] = {}
        self.last_eval_rollouts = []
        for tail, ro_b in per_walk:
            walk = {k: ro_b[k][0].cpu() for k in ("actions", "positions", "logits", "teacher_sets", "teacher_targets")}
            self.last_eval_rollouts.append(walk)
            y, x = walk["positions"][-1].tolist()
            m = {"prop_patches_found": tail["prop_patches_found"], "episode_length": walk["actions"].numel(),
                 "teacher_agreement": teacher_agreement(walk["teacher_sets"], walk["actions"]),
                 "stopped_inside_bbox": bool(walk["teacher_targets"][y, x])}
            m.update({k: v for k, v in tail.items() if k == "map" or k.startswith("yolo_")})
            for k, v in m.items():
                out.setdefault(k, []).append(float(v))
        return out

    @torch.no_grad()
    def eval_envs_on_images(self, images, bboxes, batch_size: int, eval_mode: str = "multistart", n_starts: int = 2,
                            sample_actions: bool = False, start_positions=None, device_metrics: bool = True,
                            streams: str = "loop", class_ids=None, action_mask: str = None) -> Dict[str, list]:
        """``eval_envs`` of the reference (src/supervised.py:638-752) without its plots — the evaluation whose `map` at one
        start selects ``checkpoint_best.pt`` (:81, :804): every image is walked from K starts and, for every prefix
        k = 1..K of those walks, the detections of the walks are pooled per visited patch, de-duplicated by an NMS at
        IoU 0.5 and scored per patch against the patch-local pieces of the boxes
        (``metrics_from_multiple_samples``, :569-636, and ``eval_missing_patches``, :485-567).

        The K walks of `batch_size` images run as ONE ragged rollout of batch_size * K agents (agents i * K .. i * K + K - 1
        read image i's one stored copy), exactly as ``eval_on_images`` runs its walks (sequence positions, teacher armed).
        eval_mode: "multistart" (K = n_starts random starts, each where the per-image loop's reset would put it),
        "corners" (K = 4, the corners of the image's own grid) or "rollouts" (K = n_starts walks from walk 0's start;
        meaningful with sample_actions); start_positions [n_images, K, 2] overrides the mode's starts (and its K).  With
        sample_actions, walk (i, k) samples from the stream of rollout i * K + k of the per-image loop
        (``ragged.walk_agent_keys``): the K walks of an image are that loop's K rollouts, whatever `batch_size` is;
        streams="batch" keeps the draws keyed by the agent's place in the chunk.  The
        tokens of a walk are t = 0 .. its own steps, the last patch reached included (:354-363).
        `class_ids`: one class per image; all K walks of image i run under class_ids[i], as ``eval_envs`` hands the image's
        ``class_id`` to every ``test_model_on_env`` call (:663-687).  None = class 0 for every walk.
        `action_mask`: "grid" / "unvisited" / None (``config.action_mask``), see ``RolloutRunner.rollout``.

        Returns lists.  One entry per WALK, in image order then walk order (:694-695): `prop_patches_found`,
        `episode_length`, `teacher_agreement`, `stopped_inside_bbox` as ``eval_on_images`` reports them.  One entry per
        IMAGE for every k = 1..K, suffix "" for k = 1 and f"_{eval_mode}_{k}" otherwise (:697-710):
          `map_traj{suffix}`                 mAP-50 over the cells the first k walks visited (targets: ``detection.cell_targets``)
          `prop_patches_found_traj{suffix}`  |visited ∩ target cells| / |target cells| (0 without target cells)
          `map{suffix}`                      the same mAP with every target cell no walk reached counted as well: its
                                             targets, no predictions (false negatives)
        An image whose counted cells hold no target gives 0 (:225-230).  All `map*` values are stored as fp32.
        device_metrics=True: per k one ``jn_pool_walk_detections`` launch, per variant one ``jn_match_detections`` over all
        cells of the chunk and one ``jn_average_precision_segments``; one readback per chunk (values and pool stats as one
        tensor).  The buffers are read up to the chunk's longest walk, so a pool of k walks holds at most
        k * (longest walk + 1) * max_det_per_patch boxes; beyond 4096 (at the defaults, 64 boxes per patch and 21 tokens:
        k >= 4, i.e. the last prefix of "corners" unless every walk stops early) that prefix is pooled by the host
        function, with readbacks of its own.  False: the same values from ``detection.pool_walk_detections`` and
        ``detection.map_50`` on the host.  At most ``config.eval_max_per_cell`` (``--eval-max-per-cell``, 64) survivors
        per cell are scored; ``last_eval_pool_stats`` keeps, per chunk, the [K, n, cells, 2] pool sizes and survivor
        counts that show whether the cap was reached.  ``last_eval_rollouts`` keeps the walks, K per image.
        Deviations from the reference: DESIGN.md §6."""
        from . import detection, ragged
        if eval_mode not in ragged.EVAL_MODES:
            raise ValueError(f"eval_mode must be one of {ragged.EVAL_MODES}, got {eval_mode!r}")
        if self.yolox_model() is None:
            raise ValueError("eval_envs_on_images scores detections: the model has no detector")
        runner = self._eval_runner()
        P = int(self.config.patch_size)
        M = int(getattr(self.config, "eval_max_per_cell", 64))
        given = None
        if start_positions is not None:
            given = torch.as_tensor(start_positions).to(torch.int64).cpu()
            assert given.dim() == 3 and given.shape[0] == len(images) and given.shape[2] == 2, "start_positions is [n_images, K, 2]"
            K = int(given.shape[1])
        else:
            K = 4 if eval_mode == "corners" else int(n_starts)
        assert K >= 1
        names = ["" if k == 1 else f"_{eval_mode}_{k}" for k in range(1, K + 1)]
        per_image: Dict[int, dict] = {}
        self.last_eval_pool_stats = []

        def starts(first, indices, extents):
            if given is not None:
                return given[list(indices)]
            return ragged.walk_start_positions(runner, first, indices, extents, K, eval_mode)

        per_walk = {}
        for ch in self._eval_walks(images, bboxes, batch_size, True, sample_actions=sample_actions, walks=K, walk_starts=starts,
                                   streams=streams, class_ids=class_ids, action_mask=action_mask):
            for a, tail, ro_b in ragged.walk_entries(runner, ch):
                per_walk[a] = (tail, ro_b)
            ro, env, sel = ch["rollout"], ch["env"], ch["indices"]
            n, grid = len(sel), (env.n_vertical_patches, env.n_horizontal_patches)
            dev = self.device
            tokens = torch.tensor([s + 1 for s in ch["steps"]], dtype=torch.int32)
            walk_first = torch.arange(n, dtype=torch.int32) * K
            tg, tcounts = detection.cell_targets([ch["rows"][i] for i in sel], ch["extents"][::K], grid, P,
                                                 device=dev if device_metrics else None)
            target_cells = ch["targets"][::K].reshape(n, -1).bool()
            n_tok = max(ch["steps"]) + 1                   # the kernel's LDS bound is k * n_tok * K_det: the longest walk, not T + 1
            args = tuple(ro[name][:, :n_tok] for name in ("det_boxes", "det_counts", "positions"))        # read in place
            tokens_d, first_d = (tokens.to(dev), walk_first.to(dev)) if device_metrics else (None, None)
            stats, values = [], []
            for k in range(1, K + 1):
                walk_count = torch.full((n,), k, dtype=torch.int32)
                if device_metrics:
                    pool = detection.pool_walk_detections_device(*args, tokens_d, first_d, walk_count.to(dev), k, grid, M)
                    maps = detection.walk_cell_maps_device(pool, tg, tcounts, target_cells)
                    vis = pool["visited"]
                    counts = torch.stack(((vis & target_cells).sum(1), target_cells.sum(1))).to(torch.float64)
                    values.append(torch.cat((maps.to(dev), counts)))                     # [4, n] f64
                else:
                    pool = detection.pool_walk_detections(*args, tokens, walk_first, walk_count, grid, M)
                    maps = torch.tensor(detection.walk_cell_maps(pool, tg, tcounts, target_cells.cpu()), dtype=torch.float64)
                    tc = target_cells.cpu()
                    counts = torch.stack(((pool["visited"] & tc).sum(1), tc.sum(1))).to(torch.float64)
                    values.append(torch.cat((maps, counts)))
                stats.append(pool["stats"])
            values, stats = torch.stack(values), torch.stack(stats)
            # the chunk's one readback: the values and the stats (int32, exact in f64) leave the device as one tensor
            flat = torch.cat((values.flatten(), stats.flatten().to(torch.float64))).cpu()
            self.last_eval_pool_stats.append(flat[values.numel():].to(torch.int32).reshape(stats.shape))
            values = flat[:values.numel()].reshape(values.shape).tolist()
            f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
            for b, i in enumerate(sel):
                m = {}
                for name, (map_traj, map_all, hit, tot) in zip(names, values):
                    m["map_traj" + name] = f32(map_traj[b])
                    m["prop_patches_found_traj" + name] = f32(int(hit[b]) / int(tot[b])) if int(tot[b]) > 0 else 0.0
                    m["map" + name] = f32(map_all[b])
                per_image[i] = m
        out = self._walk_metrics([per_walk[a] for a in range(len(per_walk))])
        for i in range(len(images)):
            for k, v in per_image[i].items():
                out.setdefault(k, []).append(v)
        return out

    # ---- validation: the teacher-forced half of test() (src/supervised.py:407-483, 754-810) -----------------------------
    def _yolo_map_device(self, outputs, targets) -> torch.Tensor:
        """``compute_yolo_metrics`` as a device tensor f64 [1], nothing read back.  `outputs`: the predictions of every
        patch, packed (boxes [M, K, >= 5], counts int32 [M]) or in the reference's list form (one list of None / [n, >= 5]
        per image); `targets` [..., nb, 5 | 6] = (class, x1, y1, x2, y2[, 1]), real rows marked by the last column
        (6 columns) or by a non-zero row (5)."""
        from . import detection
        dev = self.device
        t = targets.to(dev, torch.float32)
        t = t.reshape(-1, *t.shape[-2:])
        real = (t[..., -1] == 1) if t.shape[-1] >= 6 else (t != 0).any(dim=-1)
        # the real rows first, in their order (the reference's `patch_targets[patch_targets[:, -1] == 1]`)
        order = torch.argsort((~real).to(torch.int8), dim=1, stable=True)
        rows = torch.take_along_dim(t[..., :5], order[..., None], dim=1).contiguous()
        tcounts = real.sum(dim=1).to(torch.int32)
        if not isinstance(outputs, tuple):
            flat = [o for image in outputs for o in image] if len(outputs) and isinstance(outputs[0], (list, tuple)) else list(outputs)
            width = next((o.shape[1] for o in flat if o is not None), 7)
            outputs = detection.pack_boxes(flat, width, dev)
        M = outputs[0].shape[0]
        assert rows.shape[0] == M, (rows.shape, M)
        if M == 0:
            return torch.zeros(1, device=dev, dtype=torch.float64)
        if rows.shape[1] == 0:
            rows = torch.zeros((M, 1, 5), device=dev)
        if M * 100 > detection.MAX_EVAL_ENTRIES or outputs[0].shape[1] > detection.MAX_EVAL_BOXES:
            # beyond the kernels' limits: the host function (with readbacks of its own)
            return torch.tensor([detection.map_50_device(outputs, (rows, tcounts))], device=dev, dtype=torch.float64)
        return detection.average_precision_device(detection.match_detections_device(outputs, (rows, tcounts)), pooled=True)

    def compute_yolo_metrics(self, outputs, targets, device_metrics: Optional[bool] = None) -> Dict[str, torch.Tensor]:
        """``compute_yolo_metrics`` (src/supervised.py:203-277): {"map": mAP-50 with every PATCH as one unit}; 0 when the
        batch holds no real box (:225-230).  Scores come from column 4.  Arguments as
        ``_yolo_map_device``; the reference passes ``[bbox_outs]`` and ``bboxes_yolox.unsqueeze(0)``.  device_metrics
        (default: the trainer's device is a GPU): the device matching of ``detection.map_50_device``; False: the same
        value from ``detection.map_50`` on the host (list-form `outputs` only)."""
        if device_metrics is None:
            device_metrics = self.device.type == "cuda"
        if device_metrics:
            return {"map": self._yolo_map_device(outputs, targets).to(torch.float32)}
        from . import detection
        flat = [o for image in outputs for o in image] if len(outputs) and isinstance(outputs[0], (list, tuple)) else list(outputs)
        t = targets.reshape(-1, *targets.shape[-2:]).to(torch.float32)
        assert len(flat) == t.shape[0], (len(flat), t.shape)
        tgts = [p[(p[:, -1] == 1) if p.shape[-1] >= 6 else (p != 0).any(dim=-1)][:, :5] for p in t]
        return {"map": torch.tensor([detection.map_50(flat, tgts)], dtype=torch.float32, device=targets.device)}

    def _device_batch(self, patches, current_actions, next_actions, positions, masks, classes):
        """The tensors of a teacher-forced batch as ``jn_supervised_step`` / ``jn_supervised_eval`` read them: on the
        device, contiguous, patches f32, actions / positions / classes int64, masks uint8; None stays None."""
        f = lambda t, dt: None if t is None else torch.as_tensor(t).to(self.device, dt).contiguous()
        cls = f(classes, torch.int64)
        assert cls is None or cls.shape == (current_actions.shape[0],), "classes must be [B]"
        return (f(patches, torch.float32), f(current_actions, torch.int64), f(next_actions, torch.int64),
                f(positions, torch.int64), f(masks, torch.uint8), cls)

    def eval_step(self, patches, current_actions, next_actions, positions, masks, classes=None, loss_mode: Optional[str] = None,
                  want_logits: bool = True) -> Dict[str, torch.Tensor]:
        """The validation twin of ``train_step`` (``jn_supervised_eval``): eval-mode ``model(patches, current_actions,
        classes, positions)`` — running statistics, no dropout, nothing written to the model — then the loss and accuracy
        of ``compute_metrics`` against the labels of `loss_mode` (default ``config.loss_mode``; see
        ``reference_actions``).  B <= max_batch and T <= block_size; B * T is free (the encoder takes the patches in
        chunks of max_batch).  Everything stays on the device, nothing is read back: ``metrics`` f32 [4] = action_loss,
        action_accuracy, episode_length, valid tokens; ``token_loss`` f32 [B, T] and ``predicted`` u8 [B, T] (0 on
        padding); ``logits`` [B, T, n_actions] unless want_logits is False."""
        model, dev = self.model, self.device
        model.sync_weights()
        eng = model.engine()
        if loss_mode is None:
            loss_mode = getattr(self.config, "loss_mode", "best-action")
        B, T = current_actions.shape
        patches, cur, nxt, pos, msk, cls = self._device_batch(patches, current_actions, next_actions, positions, masks, classes)
        out = {"metrics": torch.zeros(4, device=dev, dtype=torch.float32),
               "token_loss": torch.empty((B, T), device=dev, dtype=torch.float32),
               "predicted": torch.empty((B, T), device=dev, dtype=torch.uint8),
               "logits": torch.empty((B, T, eng.cfg.n_actions), device=dev, dtype=torch.float32) if want_logits else None}
        check(eng.lib.jn_supervised_eval(eng.handle, ptr(patches), ptr(cur), ptr(nxt), ptr(cls), ptr(pos), ptr(msk), B, T,
                                         self.stop_weight, int(loss_mode == "on-self-trajectory"), ptr(out["logits"]),
                                         ptr(out["token_loss"]), ptr(out["predicted"]), ptr(out["metrics"]),
                                         _lib.current_stream(dev)), "jn_supervised_eval")
        return out

    @torch.no_grad()
    def eval_supervised_on_images(self, images, bboxes, batch_size: int, class_ids=None, seed: Optional[int] = None) -> Dict[str, list]:
        """``eval_supervised`` (src/supervised.py:407-483), the validation loss and accuracy on teacher trajectories plus
        the detector's validation loss, `batch_size` images at a time (the images of one batch share one size).  The model
        is put in eval mode and restored.  Per batch: ``generate_trajectories`` without views or augmentation ->
        ``jn_supervised_eval`` with ``config.loss_mode`` -> with a detector configured and enabled, its validation call on
        ``patches_yolox`` / ``bboxes_yolox`` (eval-mode PAFPN, train-mode head: the head's running statistics move, as the
        reference's do) -> ``compute_yolo_metrics``; ONE readback per batch.  Returns name -> one entry per batch:
        ``loss``, ``action_loss``, ``action_accuracy``, ``episode_length`` and, with the detector, ``yolo_total_loss``,
        ``yolo_iou_loss``, ``yolo_conf_loss``, ``yolo_cls_loss``, ``yolo_l1_loss``, ``yolo_num_fg``, ``yolo_loss``, ``map``.
        A batch without a valid token gives action_loss NaN and action_accuracy 0.  ``self.last_eval_supervised`` keeps,
        per batch, ``token_loss`` f32, ``predicted`` and ``labels`` int64 [B, T] on the host and the batch's
        ``trajectories`` (device tensors).  `seed` makes the walks reproducible (batch i uses seed + its first image)."""
        from .yolox import LOSS_NAMES
        cfg, dev = self.config, self.device
        n_images = len(images)
        detection = self.yolox_model() is not None and bool(getattr(cfg, "detection_enabled", True))
        loss_mode = getattr(cfg, "loss_mode", "best-action")
        out: Dict[str, list] = {}
        self.last_eval_supervised = []
        with self._eval_mode():
            for first in range(0, n_images, int(batch_size)):
                sel = range(first, min(n_images, first + int(batch_size)))
                batch = {"image": [images[i] for i in sel] if not isinstance(images, torch.Tensor) else images[first:sel.stop],
                         "bboxes": [bboxes[i] for i in sel] if not isinstance(bboxes, torch.Tensor) else bboxes[first:sel.stop],
                         "class_id": None if class_ids is None else torch.as_tensor(class_ids)[first:sel.stop]}
                tr = self.generate_trajectories(batch, seed=None if seed is None else seed + first, use_views=False, seed_ties=True)
                cur, nxt, msk = tr["current_actions"], tr["next_actions"], tr["masks"]
                B, T = cur.shape
                res = self.eval_step(tr["patches"], cur, nxt, tr["positions"], msk, classes=tr["class_id"], loss_mode=loss_mode,
                                     want_logits=False)
                metrics, token_loss, predicted = res["metrics"], res["token_loss"], res["predicted"]
                labels = reference_actions(cur, nxt, msk, loss_mode)
                parts = [metrics.double(), token_loss.flatten().double(), predicted.flatten().double(), labels.flatten().double()]
                if detection:
                    if tr["patches_yolox"].shape[0] > 0:
                        outputs, _, yolo = self.yolox_model().validation_loss(tr["patches_yolox"], tr["bboxes_yolox"], packed=True)
                        parts.append(torch.stack([yolo[k] for k in LOSS_NAMES]).double())
                        parts.append(self._yolo_map_device(outputs, tr["bboxes_yolox"]))
                    else:                                            # no detector patch in the batch: nothing to score
                        parts.append(torch.zeros(len(LOSS_NAMES) + 1, device=dev, dtype=torch.float64))
                host = torch.cat(parts).cpu()                        # the batch's one readback
                m = host[:4].to(torch.float32)
                n = B * T
                self.last_eval_supervised.append({
                    "token_loss": host[4:4 + n].to(torch.float32).view(B, T), "predicted": host[4 + n:4 + 2 * n].long().view(B, T),
                    "labels": host[4 + 2 * n:4 + 3 * n].long().view(B, T), "trajectories": tr})
                row = {"action_loss": m[0], "action_accuracy": m[1], "episode_length": m[2], "loss": m[0]}
                if detection:
                    y = host[4 + 3 * n:].to(torch.float32)
                    for j, k in enumerate(LOSS_NAMES):
                        row["yolo_" + k] = y[j]
                    row["yolo_loss"] = row["yolo_total_loss"]
                    row["loss"] = m[0] + row["yolo_loss"]             # fp32, as compute_metrics adds them (:177-185)
                    row["map"] = y[len(LOSS_NAMES)]
                for k, v in row.items():
                    out.setdefault(k, []).append(float(v))
        return out

    def test_on_images(self, images, bboxes, batch_size: int, class_ids=None, sample_actions: bool = False,
                       seed: Optional[int] = None, streams: str = "loop") -> Dict[str, list]:
        """The metric assembly of ``test()`` (src/supervised.py:754-810) without logger, plots or checkpoint: the
        multistart evaluation's lists (``eval_envs_on_images``), the validation lists under ``supervised_<name>``
        (:796-799); sets ``last_test_metrics`` and extends ``best_metric_history`` by the mean of ``best_metric_name``.
        `class_ids` (one per image) condition BOTH halves: the walks of the multistart evaluation run under the image's
        class, as the teacher-forced validation always did (before, the walks ran under class 0 whatever was given);
        None = class 0 everywhere, every result as before."""
        metrics = self.eval_envs_on_images(images, bboxes, batch_size, sample_actions=sample_actions, streams=streams,
                                           class_ids=class_ids)
        for name, values in self.eval_supervised_on_images(images, bboxes, batch_size, class_ids=class_ids, seed=seed).items():
            metrics["supervised_" + name] = values
        self.last_test_metrics = metrics
        self.best_metric_history.append(float(torch.tensor(metrics[self.best_metric_name], dtype=torch.float64).mean()))
        return metrics

    def train_step(self, patches, current_actions, next_actions, positions, masks, optimizer_step: bool = True,
                   process_group=None, classes=None) -> Dict[str, torch.Tensor]:
        """model(patches, current_actions, classes, positions) -> CE vs next_actions -> backward -> AdamW
        (``classes`` [B] class ids as in src/supervised.py:852, 866; None = class 0)."""
        model, dev = self.model, self.device
        model.sync_weights()
        eng = model.engine()
        self._grad_arena()                      # bound to the engine before its backward writes it
        B, T = current_actions.shape
        patches, cur, nxt, pos, msk, cls = self._device_batch(patches, current_actions, next_actions, positions, masks, classes)
        logits = torch.empty((B, T, eng.cfg.n_actions), device=dev, dtype=torch.float32)
        metrics = torch.zeros(4, device=dev, dtype=torch.float32)
        stream = _lib.current_stream(dev)
        check(eng.lib.jn_supervised_step(eng.handle, ptr(patches), ptr(cur), ptr(nxt), ptr(cls), ptr(pos), ptr(msk), B, T,
                                         self.stop_weight, ptr(logits), ptr(metrics), stream), "jn_supervised_step")
        self.iter_num += 1
        ga = int(getattr(self.config, "gradient_accumulation", 1))
        if optimizer_step and self.iter_num % ga == 0:
            object.__setattr__(model, "_last_lr", self._learning_rates())
            # the supervised loop does not clip gradients (src/supervised.py:897-902); the detector's group steps in
            # ``train_iteration``, after its own backward
            self._engine_optimizer_step(0.0, False, process_group)
        m = metrics.cpu()
        return {"loss": m[0], "action_loss": m[0], "action_accuracy": m[1], "episode_length": m[2], "logits": logits}
