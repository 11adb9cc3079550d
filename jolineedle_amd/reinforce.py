"""``ReinforceTrainer``: the REINFORCE metrics, training and evaluation of the reference (src/reinforce.py:217-497) on
the rollout of ``rollouts.RolloutRunner`` and the plumbing of ``trainer.Trainer``."""
import ctypes as C
from typing import Dict

import torch

from ._lib import JnTrainOpts, check, ptr
from .env import NeedleGeneralEnv
from .rollouts import RolloutRunner, _RolloutCall, _classes_table, _keys_table  # noqa: F401 (the tables: found here too)
from .trainer import Trainer


class ReinforceTrainer(Trainer, RolloutRunner):
    """Rollout / loss part of the reference trainer (dataset, Visdom, checkpoints are
    out of scope).  ``config`` needs max_seq_len, entropy_weight,
    stop_enabled, reward_norm (main.py:310-388)."""

    def __init__(self, config, model, logger=None, train_dataset=None, test_dataset=None, rank: int = 0):
        Trainer.__init__(self, config, model, logger, train_dataset, test_dataset, rank)
        RolloutRunner.__init__(self, model, config.max_seq_len, config.stop_enabled, getattr(config, "seed", 0), rank,
                               getattr(config, "agent_streams", "batch"), getattr(config, "action_mask", None))
        self.entropy_weight = config.entropy_weight
        self.best_metric_name = "prop_patches_found"
        self.last_return_values = []
        self.last_return_mean = 0
        self.last_return_std = 1
        self.allreduce_timing = None        # a list here receives the event pairs of ``dist.allreduce_gradients``

    @torch.no_grad()
    def _compute_last_returns_mean_std(self):
        allv = torch.cat([v.float().cpu() for v in self.last_return_values]) if self.last_return_values else torch.zeros(0)
        if len(allv) == 0:
            mean, std = 0, 1
        elif len(allv) == 1:
            mean, std = allv[0], 1
        else:
            mean, std = allv.mean(), allv.std()
        self.last_return_mean, self.last_return_std = mean, std
        self.last_return_values = []

    # ---- the reference's training loop on the autograd bridge (src/reinforce.py:267-362) -----------------------------
    def training_step(self, batch, optim_gpt, optim_yolox=None, sync_gradients: bool = True, **rollout_kw):
        """The body of the reference's loop, statement for statement (src/reinforce.py:302-353): env -> rollout ->
        compute_metrics -> [detector loss] -> (loss / ga).backward() -> every ga-th iteration clip_grad_value_ ->
        optim.step() -> optim.zero_grad() -> reward-norm window.  Everything torch sees is real: ``loss`` has a graph (the
        rollout node calls the engine's backward), ``param.grad`` are tensors, the optimisers are ``torch.optim.Optimizer``s."""
        from torch.nn.utils import clip_grad
        config, model = self.config, self.model
        self.iter_num += 1
        model.train()
        images, bboxes = batch["image"].to(self.device), batch["bboxes"]
        u8 = bool(getattr(config, "uint8_images", False))
        # --augment-rotate / --augment-translate (src/dataset.py:274-278): drawn per image, applied inside the patch reads
        views = None
        if getattr(config, "rotations", False) or getattr(config, "translations", False):
            from .views import trainer_views
            src = images if (u8 and images.dtype == torch.uint8) else images.to(torch.float32)
            views = trainer_views(self, src.contiguous(), bboxes, self.patch_size)
        self.last_views = views
        if views is not None:
            env = NeedleGeneralEnv(None, views.transform_bboxes(bboxes), self.patch_size, self.max_ep_len, self.n_glimps_levels,
                                   self.stop_enabled, engine=model.engine(), views=views)
        else:
            env = NeedleGeneralEnv(images, bboxes, self.patch_size, self.max_ep_len, self.n_glimps_levels, self.stop_enabled,
                                   engine=model.engine(), uint8_images=u8)
        self.last_env = env
        if getattr(config, "class_tokens", False) and "classes" not in rollout_kw and batch.get("class_id") is not None:
            rollout_kw["classes"] = batch["class_id"]       # opt-in: the reference's loop feeds zeros (src/reinforce.py:128-129)
        rollout = self.rollout(env, keep_patches=False, **rollout_kw)
        metrics = self.compute_metrics(rollout)
        loss = metrics["loss"]
        ga = int(getattr(config, "gradient_accumulation", 1))
        if getattr(config, "detection_enabled", False) and self.yolox_model() is not None:      # src/reinforce.py:330-339
            patches_yolox, bboxes_yolox = self._detection_batch(env, int(getattr(config, "detection_sample_neg", 1)))
            if self.detection_augment is not None:
                with torch.no_grad():
                    patches_yolox = self.detection_augment(patches_yolox)
            yolox = self.yolox_model()
            _, _, yolo_loss = yolox(patches_yolox, bboxes_yolox, predict=False)      # (the loop discards outputs / fpn_outs)
            for k, v in yolo_loss.items():
                metrics["yolo_" + k] = v.detach()
            total_loss = yolo_loss["total_loss"]         # carries the detector's graph (yolox.py::_DetectorGraph)
            loss = loss + total_loss
        (loss / ga).backward()                           # :341 — ONE backward through the rollout node and the detector node
        if self.iter_num % ga == 0:
            opts = [o for o in (optim_gpt, optim_yolox) if o is not None]
            was = [getattr(o, "sync_gradients", False) for o in opts]
            if sync_gradients:
                # data-parallel ranks: ONE all-reduce of the flat gradient buffer (mean), before the clip as under DDP —
                # the optimisers must not reduce the (already averaged, clipped) gradients a second time
                from .dist import allreduce_gradients
                sc = allreduce_gradients(model._flat_grads, model._arena_numel)
                if sc != 1.0:
                    model._flat_grads.mul_(sc)
                for o in opts:
                    if hasattr(o, "sync_gradients"):
                        o.sync_gradients = False
            clip_grad.clip_grad_value_(model.parameters(), 1)
            optim_gpt.step()
            optim_gpt.zero_grad()
            if getattr(config, "detection_enabled", False) and optim_yolox is not None:
                optim_yolox.step()
                optim_yolox.zero_grad()
            for o, w in zip(opts, was):
                if hasattr(o, "sync_gradients"):
                    o.sync_gradients = w
            if config.reward_norm:
                self._compute_last_returns_mean_std()
        metrics["loss"] = loss.detach()
        return metrics

    def run(self, rank: int, world_size: int, ddp_port: int, batches=None, max_iters: int = None, backend: str = None):
        """``ReinforceTrainer.run`` (src/reinforce.py:267-362) without the dataset / Visdom / test plumbing (out of scope,
        SURVEY.md §8): `batches` is any iterable of collated batches ({"image": [B,3,H,W], "bboxes": [B,nb,4]}, the
        ``padded_collate_fn`` layout; default: ``self.train_dataset``), re-iterated when exhausted.  Returns the metrics of
        the last iteration."""
        cfg = self.config
        augment = bool(getattr(cfg, "detection_enabled", False) and getattr(cfg, "augment_detection", False))
        # sync_gradients False on the optimisers: training_step averages the gradients itself, before the clip

        def step(i, batch, optim_gpt, optim_yolox):
            return self.training_step(batch, optim_gpt, optim_yolox, sync_gradients=world_size > 1)
        return self._run_loop(step, rank, world_size, ddp_port, backend, batches, max_iters, augment, sync_gradients=False)

    def _detection_batch(self, env: NeedleGeneralEnv, sample_neg: int):
        """``env.get_detection_batch``; with ``config.device_detection_batch`` (default off) assembled on the device, the
        negatives drawn from ``detection_batch_seed()``."""
        if getattr(self.config, "device_detection_batch", False):
            return env.get_detection_batch(sample_neg, device=True, seed=self.detection_batch_seed())
        return env.get_detection_batch(sample_neg)

    def detection_batch_seed(self) -> int:
        """Key of the device route's negative draws in the current iteration: the trainer's seed, its rank (the draws are
        keyed by the image's index within the rank's batch, so data-parallel ranks need keys of their own; 17 * rank as in
        ``init_detection``) and the iteration counter."""
        return ((self.seed + 17 * int(self.rank)) * 1000003 + int(self.iter_num)) & 0xFFFFFFFFFFFFFFFF

    # ---- training: one REINFORCE iteration (src/reinforce.py:302-353) ------------------------
    def train_iteration(self, env: NeedleGeneralEnv, sample_actions: bool = True, forced_actions=None,
                        start_positions=None, stop_early: bool = True, optimizer_step: bool = True,
                        process_group=None, agent_keys=None, classes=None, action_mask: str = None) -> Dict[str, torch.Tensor]:
        """rollout (train-mode BatchNorm) -> compute_metrics -> backward -> [all-reduce] -> clip + AdamW,
        all inside the engine.  Returns the metrics of src/reinforce.py:243-252.  `agent_keys`, `classes`, `action_mask`
        (the loss and its gradient are then those of the masked Categorical): see ``rollout``."""
        # (a train-mode rollout is recurrent whatever the config says: see ``rollout`` on "sequence")
        call = _RolloutCall(self, env, sample_actions, forced_actions, start_positions, agent_keys, classes, "recurrent", action_mask)
        eng, buf, stream = call.eng, call.buf, call.stream
        self._grad_arena()                      # bound to the engine before its backward writes it
        self.iter_num += 1
        ga = int(getattr(self.config, "gradient_accumulation", 1))
        opts = JnTrainOpts(struct_size=C.sizeof(JnTrainOpts), reward_norm=int(bool(self.config.reward_norm)),
                           ret_mean=float(self.last_return_mean), ret_std=float(self.last_return_std),
                           entropy_weight=float(self.entropy_weight), loss_scale=1.0 / ga)
        metrics_dev = torch.zeros(8, device=self.device, dtype=torch.float32)
        with call.armed():
            check(eng.lib.jn_reinforce_step(eng.handle, call.mode, ptr(call.forced_actions), ptr(call.start_positions), call.seed,
                                            int(stop_early), C.byref(opts), C.byref(call.out), ptr(metrics_dev), stream),
                  "jn_reinforce_step")
        m = metrics_dev.cpu()
        S = int(m[5])
        if self.config.reward_norm:
            lm = buf["logit_masks"][:, :S].bool()
            self.last_return_values.append(buf["returns"][:, :S][lm].clone())
        # detector training step on the patches that hold boxes (+ negatives), src/reinforce.py:330-339
        detection = bool(getattr(self.config, "detection_enabled", False)) and self.yolox_model() is not None
        yolo_losses = {}
        if detection:
            patches_y, boxes_y = self._detection_batch(env, int(getattr(self.config, "detection_sample_neg", 1)))
            if self.detection_augment is not None:                                 # src/reinforce.py:332-333
                patches_y = self.detection_augment(patches_y)
            yolo_losses = self.yolox_model().loss_and_backward(patches_y, boxes_y, loss_scale=1.0 / ga)
        if optimizer_step and self.iter_num % ga == 0:
            object.__setattr__(self.model, "_last_lr", self._learning_rates())
            self._engine_optimizer_step(1.0, detection, process_group, self.allreduce_timing)
            if self.config.reward_norm:
                self._compute_last_returns_mean_std()
        self._last_train_buffers = buf
        self._last_action_sets = call.action_sets
        res = {"action_loss": m[0], "entropy_loss": m[1], "loss": m[2], "returns": m[3], "episode_length": m[4], "steps": S}
        for k, v in yolo_losses.items():
            res["yolo_" + k] = v
        return res

    def compute_metrics(self, rollout: Dict[str, torch.Tensor], env: NeedleGeneralEnv = None):
        """The reference's metric dictionary (src/reinforce.py:217-265): REINFORCE loss with window-normalised returns,
        entropy bonus, mean return and episode length over the valid steps; with ``env``, the found-ratios and STOP usage
        of image 0.  (``train_iteration`` gets the same numbers from ``reinforce_loss_kernel``; this form is the one that
        carries the autograd graph of ``training_step``.)"""
        valid = rollout["logit_masks"]
        n_valid = valid.sum()
        returns = rollout["returns"]
        if self.config.reward_norm:
            self.last_return_values.append(returns[valid].detach().clone())      # feeds the window statistics
            returns = (returns - self.last_return_mean) / (self.last_return_std + 1e-8)

        def masked_mean(x):
            return (x * valid).sum() / n_valid
        action_loss = -masked_mean(rollout["logprobs"] * returns)
        entropy_loss = -masked_mean(rollout["entropies"])
        metrics = {
            "action_loss": action_loss,
            "entropy_loss": entropy_loss,
            "loss": action_loss + self.entropy_weight * entropy_loss,
            "returns": (rollout["rewards"] * valid).sum(dim=1).mean(),
            "episode_length": valid.sum(dim=1).float().mean(),
        }
        if env:
            found = env.prop_patches_found[0]
            metrics["prop_patches_found"] = found
            metrics["prop_bbox_found"] = env.prop_bboxes_found[0]
            if self.stop_enabled:
                stopped = env.terminated[0]
                metrics["stop_used"] = stopped.to(torch.float32)
                metrics["stop_misused"] = (stopped & (found < 1)).to(torch.float32)
        return metrics

    @torch.no_grad()
    def eval_on_batch(self, env: NeedleGeneralEnv, do_detection: bool = None, merge_bboxes: bool = None,
                      token_positions: str = None, action_mask: str = None) -> Dict[str, torch.Tensor]:
        """``eval_on_sample`` of the reference (src/reinforce.py:424-497) without the plotting: greedy rollout,
        rollout metrics incl. the env's found-ratios, and — with detection — mAP-50 of the boxes found along the
        trajectories (moved to full-image coordinates, optionally merged) plus the detector's mAP on every patch that
        holds a box (`yolo_map`).  The reference evaluates one image at a time; any batch size works here (the
        per-image metrics it reads from index 0 stay index 0).  `token_positions`, `action_mask`: see ``rollout``."""
        from .detection import patch_bboxes2full_image
        from .ragged import detection_eval_metrics
        cfg = self.config
        if do_detection is None:
            do_detection = bool(getattr(cfg, "detection_enabled", False))
        if merge_bboxes is None:
            merge_bboxes = bool(getattr(cfg, "merge_bboxes", False))
        ro = self.rollout(env, sample_actions=False, do_detection=do_detection, token_positions=token_positions,
                          action_mask=action_mask)
        metrics = self.compute_metrics(ro, env)
        if do_detection:
            targets = env.get_detection_targets()
            offsets = ro["positions"][:, :, [1, 0]] * self.patch_size        # (y, x) grid -> (x, y) pixels
            preds = patch_bboxes2full_image(ro["bboxes"], offsets, ro["masks"])
            patches, patch_targets = self._detection_batch(env, 0)
            metrics.update(detection_eval_metrics(self.yolox_model(), preds, targets, patches, patch_targets, merge_bboxes))
        return metrics

    @torch.no_grad()
    def eval_on_images(self, images, bboxes, batch_size: int, do_detection: bool = None,
                       merge_bboxes: bool = None, device_metrics: bool = False, token_positions: str = None,
                       class_ids=None, action_mask: str = None) -> Dict[str, list]:
        """The per-image ``all_metrics`` of the reference's ``test()`` (src/reinforce.py:383-392) without its loop of
        ``B = 1`` envs: `images` ([3, Hi, Wi] tensors of any sizes, uint8 read in place or float 0..1) are evaluated
        `batch_size` at a time (``ragged.plan_chunks``), every agent inside its own image.  Returns, for every key of
        ``eval_on_batch``, one value per image in image order, each equal to ``eval_on_batch`` on that image alone (up
        to the engine's rounding across batch sizes; every image starts where its own random reset would put it,
        ``ragged.loop_start_positions``); ``last_return_values`` grows by one entry per image in image
        order, as that loop leaves it.  bboxes[i]: [n_i, 4] xyxy in image i's own pixels.

        device_metrics=True: the `map` entry of a whole chunk comes from the device — the rollout's boxes go
        ``rollout_boxes_packed`` -> (merge_bboxes) ``merge_boxes_device`` -> ``map_50_device(per_image=True)`` without
        leaving it, the targets are merged there too; one readback per chunk.  Same keys; `map` equals the host
        path's up to fp32 storage; the `yolo_*` entries are computed as without it.  `token_positions`: see ``rollout``.
        `class_ids`: one class per image (a tensor or a sequence) behind the class token of its walk; None = class 0.
        `action_mask`: see ``rollout``."""
        from .ragged import eval_image_chunks, image_classes, rollout_chunks
        class_ids = image_classes(class_ids, len(images))
        if do_detection is None:
            do_detection = bool(getattr(self.config, "detection_enabled", False))
        if merge_bboxes is None:
            merge_bboxes = bool(getattr(self.config, "merge_bboxes", False))
        rows = [torch.as_tensor(b).reshape(-1, 4).to(torch.long) for b in bboxes]
        chunks = rollout_chunks(self, images, rows, batch_size, do_detection=do_detection, token_positions=token_positions,
                                class_ids=class_ids, action_mask=action_mask)
        per_image = eval_image_chunks(self, self.yolox_model(), chunks, do_detection, merge_bboxes, device_metrics)
        out: Dict[str, list] = {}
        for tail, ro_b in per_image:                      # compute_metrics in image order: the reward-norm window's order
            m = self.compute_metrics(ro_b)
            m.update(tail)
            for k, v in m.items():
                out.setdefault(k, []).append(float(v))
        return out
