"""``NeedleGeneralEnv`` — batched needle environment of the reference
(src/env/general_env.py:14-573) with all state on the device, stepped by
libjnroll.so (``jn_env_*``).  n_glimps_levels must be 1 (src/reinforce.py:58).

The images stay where the caller put them: fp32 values in [0, 1], or, with
``uint8_images=True``, the 8-bit pixels themselves (a quarter of the upload and of
the HBM), which every kernel reads as byte / 255 exactly as ToTensor computes it."""
from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, ptr
from .engine import Engine, bare_env_config


class NeedleGeneralEnv:
    def __init__(self, images: Tensor, bboxes: Tensor, patch_size: int, max_ep_len: int,
                 n_glimps_levels: int = 1, stop_enabled: bool = False, engine: Engine = None, *,
                 uint8_images: bool = False, views=None, clamp_to_image: bool = False):
        """views: an ``ImageViews`` (views.py) — the env then sees the augmented images on the views' canvas without
        their ever being written; `images` may be None, `bboxes` are the boxes already on the canvas
        (``views.transform_bboxes``) and ``height`` / ``width`` are the canvas.
        clamp_to_image (views without translation only): every agent stays inside its own image's patch grid
        (``views.grid_extents``) and its boxes are clipped to it, as if the image were padded on its own (infer.py:138-146)
        — the inference semantics; the default lets every agent walk the canvas, the reference's padded collate."""
        self.views = views
        self.grid_extents = None
        self._grid_extents_dev = None                      # device copy, made on first use (get_detection_batch(device=True))
        if clamp_to_image:
            assert views is not None, "clamp_to_image needs views"
            self.grid_extents = views.grid_extents(patch_size)
        if views is not None:
            self._init_views(views, bboxes, patch_size, max_ep_len, n_glimps_levels, stop_enabled, engine)
            return
        assert images.shape[0] == bboxes.shape[0]          # general_env.py:37-39
        assert len(images.shape) == 4
        assert n_glimps_levels > 0
        if n_glimps_levels != 1:
            raise NotImplementedError("only n_glimps_levels == 1 is on the rollout path (src/reinforce.py:58)")
        if not images.is_cuda:
            raise RuntimeError("NeedleGeneralEnv of the HIP engine needs images on the GPU (no CPU fallback)")
        self.patch_size, self.max_ep_len = patch_size, max_ep_len
        self.n_glimps_levels, self.stop_enabled = n_glimps_levels, stop_enabled
        self.batch_size, self.n_channels, self.height, self.width = images.shape
        assert self.n_channels == 3
        assert self.height % self.patch_size == 0          # general_env.py:50-51
        assert self.width % self.patch_size == 0
        self.n_vertical_patches = self.height // patch_size
        self.n_horizontal_patches = self.width // patch_size
        self.device = images.device
        # uint8_images: a uint8 tensor is used in place (jn_env_init_u8); otherwise (or for float images) it becomes fp32
        self.uint8_images = bool(uint8_images) and images.dtype == torch.uint8
        if self.uint8_images:
            self._images = images.contiguous()
        else:
            self._images = images.to(torch.float32).contiguous()
        self.bboxes = bboxes
        self._bboxes_dev = bboxes.to(self.device, torch.int64).contiguous()
        self._engine = None
        self.bind(engine)

    def _init_views(self, views, bboxes, patch_size, max_ep_len, n_glimps_levels, stop_enabled, engine):
        assert len(views) == bboxes.shape[0]
        assert n_glimps_levels > 0
        if n_glimps_levels != 1:
            raise NotImplementedError("only n_glimps_levels == 1 is on the rollout path (src/reinforce.py:58)")
        if views.device.type != "cuda":
            raise RuntimeError("NeedleGeneralEnv of the HIP engine needs images on the GPU (no CPU fallback)")
        self.patch_size, self.max_ep_len = patch_size, max_ep_len
        self.n_glimps_levels, self.stop_enabled = n_glimps_levels, stop_enabled
        self.batch_size, self.n_channels = len(views), 3
        self.height, self.width = views.canvas
        assert self.height % patch_size == 0 and self.width % patch_size == 0
        self.n_vertical_patches = self.height // patch_size
        self.n_horizontal_patches = self.width // patch_size
        self.device = views.device
        self.uint8_images = views.uint8
        self._images = None
        self.bboxes = bboxes
        self._bboxes_dev = bboxes.to(self.device, torch.int64).contiguous()
        self._engine = None
        self.bind(engine)

    # ---- engine binding ----------------------------------------------------------------
    def bind(self, engine: Engine = None):
        """(Re-)create the device state inside `engine` (the model's context for rollouts)."""
        if engine is None:
            engine = Engine(bare_env_config(self.patch_size, self.batch_size, self.device.index or 0,
                                            self.max_ep_len))
        if engine is self._engine:
            return
        self._engine = engine
        nb = self._bboxes_dev.shape[1] if self._bboxes_dev.dim() == 3 else 0
        if self.grid_extents is not None:
            import ctypes as C
            ext = self.grid_extents.contiguous()
            check(engine.lib.jn_env_init_ragged(engine.handle, self.views.table_host(),
                                                C.cast(ext.data_ptr(), C.POINTER(C.c_int32)), ptr(self._bboxes_dev),
                                                self.batch_size, self.height, self.width, nb, self.max_ep_len,
                                                int(self.stop_enabled), self._stream()), "jn_env_init_ragged")
            return
        if self.views is not None:
            check(engine.lib.jn_env_init_views(engine.handle, self.views.table_host(), ptr(self._bboxes_dev), self.batch_size,
                                               self.height, self.width, nb, self.max_ep_len, int(self.stop_enabled),
                                               self._stream()), "jn_env_init_views")
            return
        init = engine.lib.jn_env_init_u8 if self.uint8_images else engine.lib.jn_env_init
        check(init(engine.handle, ptr(self._images), ptr(self._bboxes_dev), self.batch_size,
                   self.height, self.width, nb, self.max_ep_len, int(self.stop_enabled),
                   self._stream()), "jn_env_init")

    def _stream(self):
        return _lib.current_stream(self.device)

    def _view(self, what, shape, dtype):
        import ctypes as C
        p = C.c_void_p()
        check(self._engine.lib.jn_env_state(self._engine.handle, what, C.byref(p)), "jn_env_state")
        n = 1
        for s in shape:
            n *= s
        itemsize = torch.empty((), dtype=dtype).element_size()
        out = torch.empty(shape, dtype=dtype, device=self.device)
        from .hipmem import copy_d2d
        copy_d2d(out.data_ptr(), p.value, n * itemsize, self.device)
        return out

    # ---- reference surface -------------------------------------------------------------
    @property
    def images(self) -> Tensor:
        if self.views is not None:                         # on demand only: the engine never needs the canvas
            return self.views.materialize().unsqueeze(1)
        return self._images.unsqueeze(1)                   # [B, 1, C, H, W] (general_env.py:115); uint8 env: the bytes

    @property
    def positions(self) -> Tensor:
        return self._view(0, (self.batch_size, 2), torch.int64)

    @property
    def bbox_masks(self) -> Tensor:
        g = (self.batch_size, self.n_vertical_patches, self.n_horizontal_patches)
        return self._view(1, g, torch.uint8).bool()

    @property
    def visited_patches(self) -> Tensor:
        g = (self.batch_size, self.n_vertical_patches, self.n_horizontal_patches)
        return self._view(2, g, torch.uint8).bool()

    @property
    def steps(self) -> Tensor:
        return self._view(3, (self.batch_size,), torch.int32).long()

    @property
    def has_stopped(self) -> Tensor:
        return self._view(4, (self.batch_size,), torch.uint8).bool()

    @property
    def patches(self) -> Tensor:
        out = torch.empty((self.batch_size, 3, self.patch_size, self.patch_size), device=self.device)
        check(self._engine.lib.jn_env_patches(self._engine.handle, ptr(out), self._stream()), "jn_env_patches")
        return out.unsqueeze(1)                            # [B, glimps_level = 1, C, P, P]

    def reset(self, positions=None, seed: int = 0) -> Tuple[Tensor, dict]:
        if positions is not None:
            positions = positions.to(self.device, torch.int64).contiguous()
        check(self._engine.lib.jn_env_reset(self._engine.handle, ptr(positions), seed, self._stream()), "jn_env_reset")
        return self.patches, {"positions": self.positions}

    @torch.no_grad()
    def step(self, actions: Tensor):
        actions = actions.to(self.device, torch.int64).contiguous()
        B = self.batch_size
        rewards = torch.empty((B,), device=self.device, dtype=torch.float32)
        term = torch.empty((B,), device=self.device, dtype=torch.uint8)
        trunc = torch.empty((B,), device=self.device, dtype=torch.uint8)
        check(self._engine.lib.jn_env_step(self._engine.handle, ptr(actions), ptr(rewards), ptr(term), ptr(trunc),
                                           self._stream()), "jn_env_step")
        return self.patches, rewards, term.bool(), trunc.bool(), {"positions": self.positions}

    @property
    def terminated(self) -> Tensor:
        if self.stop_enabled:
            return self.has_stopped
        m, v = self.bbox_masks, self.visited_patches
        return ((m & v) != m).sum(dim=(1, 2)) == 0

    @property
    def prop_patches_found(self) -> Tensor:
        m, v = self.bbox_masks, self.visited_patches
        count = (m & v).sum(dim=(1, 2))
        tot = m.sum(dim=(1, 2))
        tot[tot == 0] = 1
        return count / tot

    # ---- detection bookkeeping (src/env/general_env.py:381-573) ----------------------------------------
    def parse_bboxes(self, bboxes: Tensor = None):
        """Ground-truth boxes split over the patch grid: ([B, Gy, Gx, nb, 4] patch-local xyxy, [B, Gy, Gx, nb] masks)."""
        from .detection import split_bboxes_over_patches
        return split_bboxes_over_patches(self.bboxes if bboxes is None else bboxes, self.n_vertical_patches,
                                         self.n_horizontal_patches, self.patch_size)

    def get_detection_targets(self):
        from .detection import detection_targets
        return detection_targets(self.bboxes, self.n_vertical_patches, self.n_horizontal_patches, self.patch_size)

    @torch.no_grad()
    def get_detection_batch(self, sample_neg: int = 1, generator: torch.Generator = None, device: bool = False,
                            seed: int = 0):
        """Patches to train the detector on: every patch holding (a piece of) a box plus `sample_neg` random empty
        patches per image; returns (patches [n, 3, P, P], bboxes [n, nb, 1 + 4]) like general_env.py:503-544.
        device: the cells and targets come from ``detection.detection_cells_device`` on the env's boxes (the
        transformed ones under views; with the grid extents in ragged mode) and the patches from one indexed gather —
        no Python loop over the images, one readback (the row count).  The positive rows are those of the host route,
        in its order; the negatives are drawn from `seed` by the rule of ``detection.detection_cells`` instead of
        ``torch.randperm`` (`generator` is not used).  A batch without boxes (nb = 0) gives negatives only, with
        targets [n, 0, 5], on either route."""
        if device:
            return self._detection_batch_device(int(sample_neg), int(seed))
        boxes, masks = self.parse_bboxes()
        any_box = masks.any(-1).cpu()
        P = self.patch_size
        patches, all_boxes = [], []
        cells = []                                         # uint8 env: (image, y, x) of each patch, one gather below
        for i in range(self.batch_size):
            pos = torch.nonzero(any_box[i])
            neg = torch.nonzero(~any_box[i])
            neg = neg[torch.randperm(len(neg), generator=generator)[:sample_neg]]
            for y, x in torch.cat((pos, neg)).tolist():
                if self.uint8_images or self.views is not None:
                    cells.append((i, y, x))
                else:
                    patches.append(self._images[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P])
                all_boxes.append(torch.nn.functional.pad(boxes[i, y, x], (1, 0)))
        if self.uint8_images or self.views is not None:
            from .trajectory import gather_indexed
            cells = torch.tensor(cells, dtype=torch.int64).reshape(-1, 3)
            return (gather_indexed(self._images, cells[:, 0], cells[:, 1:], P, views=self.views),
                    torch.stack(all_boxes).to(self.device))
        return torch.stack(patches), torch.stack(all_boxes).to(self.device)

    def _detection_batch_device(self, sample_neg: int, seed: int):
        from .detection import detection_cells_device
        from .trajectory import gather_indexed
        ext = None
        if self.grid_extents is not None:
            if self._grid_extents_dev is None:
                self._grid_extents_dev = self.grid_extents.to(self.device, torch.int32).contiguous()
            ext = self._grid_extents_dev
        bb = self._bboxes_dev
        nb = int(bb.shape[1]) if bb.dim() == 3 else 0
        if nb == 0:
            # a batch without any box (the host route then returns negatives only, targets [n, 0, 5]): the kernel takes at
            # least one box per image, so it gets one that touches no cell (x2 // P < x1 // P) and its column is dropped
            bb = torch.tensor([0, 0, -1, -1], dtype=torch.int64, device=self.device).repeat(self.batch_size, 1, 1)
        cells, targets, _, _ = detection_cells_device(bb, self.n_vertical_patches, self.n_horizontal_patches,
                                                      self.patch_size, sample_neg, seed, extents=ext)
        targets = targets[:, :nb]
        # (the cells lie on the grid by construction: the gather's host-side asserts, a readback each, are skipped)
        patches = gather_indexed(self._images, cells[:, 0], cells[:, 1:], self.patch_size, views=self.views,
                                 _check_positions=False)
        return patches, targets

    @property
    def prop_bboxes_found(self) -> Tensor:
        return (self.prop_patches_found > 0).to(torch.float32)
