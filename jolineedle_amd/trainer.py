"""``Trainer``: what ``ReinforceTrainer`` and ``SupervisedTrainer`` share, after the base class of the reference
(src/trainer.py): the process group, the detector handle and its augmentation, the engine's gradient arena and optimiser
step, and the loop of ``run``."""
import contextlib

from . import _lib
from ._lib import check


class Trainer:
    def __init__(self, config, model, logger=None, train_dataset=None, test_dataset=None, rank: int = 0):
        self.config, self.model, self.rank = config, model, rank
        self.logger, self.train_dataset, self.test_dataset = logger, train_dataset, test_dataset
        self.device = model.device
        self.iter_num = 0
        self.detection_augment = None       # off until ``init_detection``
        self._owns_process_group = False

    def yolox_model(self):
        return getattr(self.model, "_yolox_view", None)      # None: no detector configured (with_detector = False)

    def ddp_setup(self, rank: int, world_size: int, port: int, backend: str = None):
        """``Trainer.ddp_setup`` (src/trainer.py:61-71): one process per GPU, backend "nccl" (= RCCL over xGMI on ROCm).
        Rendezvous on 127.0.0.1 (the reference's "localhost" may not resolve in a container); ``backend="gloo"`` is for
        CPU-side rehearsals."""
        import os
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        if not dist.is_initialized():
            dist.init_process_group(backend=backend or "nccl", rank=rank, world_size=world_size)
            self._owns_process_group = True           # _run_loop only tears down a group it created itself

    def init_detection(self, **kw):
        """``Trainer.init_detection`` (src/trainer.py:176-186): installs the on-device augmentation of the detector
        patches (and, in supervised training, of the trajectory patches: src/supervised.py:855-861, 884-885).  Off until
        called (the parity tests compare un-augmented steps); keyword arguments go to ``augment.DetectionAugment``
        (e.g. ``planckian_coeffs``)."""
        from .augment import DetectionAugment
        kw.setdefault("seed", int(getattr(self.config, "seed", 0)) + 17 * int(self.rank))
        self.detection_augment = DetectionAugment(**kw)
        return self.detection_augment

    def _grad_arena(self):
        """The engine's flat fp32 gradient arena: owned by the MODEL (one per engine, shared by all trainers)."""
        g = self.model.grad_arena()
        self._optim_numel = self.model._optim_gpt_numel
        return g

    def _learning_rates(self):
        """(learning_rate, yolo_lr) of the config; as ``model._last_lr`` they are ``save_checkpoint``'s default."""
        lr = float(getattr(self.config, "learning_rate", 1e-4))
        return lr, float(getattr(self.config, "yolo_lr", lr))

    def _engine_optimizer_step(self, clip: float, detection: bool, process_group=None, timing: list = None):
        """The optimiser step inside the engine, the ONE exchange step of an iteration: flat gradient all-reduce (RCCL
        over xGMI) -> AdamW on the policy's group, gradients clipped to `clip` (0 = not at all) -> with `detection` the
        detector's group (optim_yolox.step(), src/reinforce.py:348-350) -> zero the arena -> refresh the flat parameters."""
        from .dist import allreduce_gradients
        eng, grads, stream = self.model.engine(), self._grad_arena(), _lib.current_stream(self.device)
        scale = allreduce_gradients(grads, grads.numel() if detection else self._optim_numel, process_group, timing=timing)
        lr, ylr = self._learning_rates()
        check(eng.lib.jn_optimizer_step(eng.handle, lr, 0.01, clip, scale, stream), "jn_optimizer_step")
        if detection:
            check(eng.lib.jn_optimizer_step_group(eng.handle, 1, ylr, 0.01, clip, scale, stream), "jn_optimizer_step_group")
        grads.zero_()
        self.model.refresh_flat_params()

    def _run_loop(self, step, rank: int, world_size: int, port: int, backend, batches, max_iters, augment: bool,
                  sync_gradients: bool):
        """Behind both ``run``s: [``init_detection`` when `augment`] -> rank and, with several ranks or a `backend`, the
        process group -> the model's optimisers, their ``sync_gradients`` flag set to `sync_gradients` -> for ``max_iters``
        iterations ``step(i, batch, optim_gpt, optim_yolox)`` over `batches` (default ``train_dataset``), re-iterated
        when exhausted -> a process group this trainer created is destroyed.  Returns the last step's value."""
        import torch.distributed as dist
        if augment:
            self.init_detection()
        self.rank = rank
        if world_size > 1 or backend:
            self.ddp_setup(rank, world_size, port, backend)
        optim_gpt, optim_yolox = self.model.configure_optimizers(self.config)
        for o in (optim_gpt, optim_yolox):
            if o is not None:
                o.sync_gradients = sync_gradients
        self.optim_gpt, self.optim_yolox = optim_gpt, optim_yolox
        batches = batches if batches is not None else self.train_dataset
        assert batches is not None, "run() needs an iterable of collated batches"
        n_iters = int(max_iters if max_iters is not None else getattr(self.config, "max_iters", 1))
        it, metrics = iter(batches), None
        for i in range(n_iters):
            try:
                batch = next(it)
            except StopIteration:
                it = iter(batches)
                batch = next(it)
            metrics = step(i, batch, optim_gpt, optim_yolox)
        if self._owns_process_group and dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()                 # src/reinforce.py:362 / src/supervised.py:911
            self._owns_process_group = False
        return metrics

    @contextlib.contextmanager
    def _eval_mode(self):
        """The model in eval mode (src/supervised.py:294), put back as it was on the way out."""
        was_training = self.model.training
        self.model.eval()
        try:
            yield
        finally:
            self.model.train(was_training)
