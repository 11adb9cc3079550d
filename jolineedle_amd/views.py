"""``ImageViews`` — the reference dataset's rotation by a multiple of 90 degrees, whole-pixel translation and
bottom / right padding to one batch canvas (``NeedleDataset.rotate`` / ``translate`` / ``padded_collate_fn``,
src/dataset.py:95-226, 274-278, 308-347) as a per-image descriptor that the patch gather applies while it reads.

The stored images stay where the caller put them and the augmented batch is never written: the engine only ever
reads patches, so ``jn_gather_patches_views`` / ``jn_env_init_views`` map every pixel of the logical canvas back to a
pixel of the stored image (include/jnroll.h: ``jn_image_view``).  ``materialize()`` builds the augmented canvas with
torch ops; it is the oracle of the tests and the baseline of tools/views_ab.py and is never used by the trainers.

Boxes are [B, nb, 4] int64 pixel xyxy with all-zero rows as padding (the collate's padding); padding rows take no
part in the translation margins and stay zero.
"""
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

ANGLES = (0, 90, 180, 270)


def _rotated_hw(Hs: int, Ws: int, rot: int) -> Tuple[int, int]:
    return (Ws, Hs) if rot in (90, 270) else (Hs, Ws)


def rotate_boxes(boxes: np.ndarray, Hs: int, Ws: int, rot: int) -> np.ndarray:
    """``NeedleDataset.rotate``'s box formulas verbatim (src/dataset.py:102, 113-153) on [n, 4] xyxy rows.  The
    reference unpacks ``image.shape`` as ``(_, image_width, image_height)`` — its "width" is the stored HEIGHT — and
    subtracts from the size, not from size - 1: boxes and pixels sit one pixel apart after a rotation, as there."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    image_width, image_height = int(Hs), int(Ws)
    if rot == 0:
        out = (x1, y1, x2, y2)
    elif rot == 90:
        out = (image_width - y2, x1, image_width - y1, x2)
    elif rot == 180:
        out = (image_height - x2, image_width - y2, image_height - x1, image_width - y1)
    elif rot == 270:
        out = (y1, image_height - x2, y2, image_height - x1)
    else:
        raise ValueError(f"rotation {rot} is not one of {ANGLES}")
    return np.stack(out, axis=1).astype(np.int64)


def translate_margins(boxes: np.ndarray, img_height: int, img_width: int) -> Tuple[int, int, int, int]:
    """(up_left.x, up_left.y, bottom_right.x, bottom_right.y) margins of ``translate`` (src/dataset.py:164-180)."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    min_x, min_y = max(int(b[:, 0].min()), 0), max(int(b[:, 1].min()), 0)
    max_x, max_y = min(int(b[:, 2].max()), img_width), min(int(b[:, 3].max()), img_height)
    return (min(img_width // 3, min_x), min(img_height // 3, min_y),
            min(img_width // 3, img_width - max_x), min(img_height // 3, img_height - max_y))


class ImageViews:
    """B stored images seen as B augmented images on one canvas.

    images: one stacked [B, 3, H, W] tensor or a list of [3, Hi, Wi] tensors (contiguous, all fp32 or all uint8);
    they are kept alive here.  rot[i] in {0, 90, 180, 270}; (ty[i], tx[i]) shifts the rotated image down / right.
    canvas: (Hc, Wc), default the smallest multiple of `patch_size` that holds every rotated image."""

    def __init__(self, images: Union[Tensor, Sequence[Tensor]], rot=None, ty=None, tx=None, patch_size: Optional[int] = None,
                 canvas: Optional[Tuple[int, int]] = None):
        if isinstance(images, Tensor):
            assert images.dim() == 4, "a stacked batch is [B, 3, H, W]"
            self._keep = images if images.is_contiguous() else images.contiguous()
            self.sources: List[Tensor] = [self._keep[i] for i in range(self._keep.shape[0])]
        else:
            self.sources = [im if im.is_contiguous() else im.contiguous() for im in images]
            self._keep = self.sources
        B = len(self.sources)
        assert B >= 1
        self.dtype, self.device = self.sources[0].dtype, self.sources[0].device
        assert self.dtype in (torch.float32, torch.uint8), "image views hold fp32 or uint8 images"
        for im in self.sources:
            assert im.dim() == 3 and im.shape[0] == 3, "a stored image is [3, Hs, Ws]"
            assert im.dtype == self.dtype and im.device == self.device, "mixed element types or devices within one batch"

        def ints(v):
            a = np.zeros(B, np.int64) if v is None else np.asarray(torch.as_tensor(v).cpu() if isinstance(v, Tensor) else v, np.int64)
            assert a.shape == (B,)
            return a
        self.rot, self.ty, self.tx = ints(rot), ints(ty), ints(tx)
        assert all(int(r) in ANGLES for r in self.rot), f"rotations must be in {ANGLES}"
        self.stored_hw = [(int(im.shape[1]), int(im.shape[2])) for im in self.sources]
        self.rotated_hw = [_rotated_hw(h, w, int(r)) for (h, w), r in zip(self.stored_hw, self.rot)]
        self.patch_size = None if patch_size is None else int(patch_size)
        if canvas is None:
            assert patch_size is not None, "canvas or patch_size required"
            P = self.patch_size                       # padded_collate_fn: max size, rounded up to a multiple of P
            canvas = tuple(-(-max(hw[k] for hw in self.rotated_hw) // P) * P for k in (0, 1))
        self.canvas = (int(canvas[0]), int(canvas[1]))
        for hr, wr in self.rotated_hw:
            assert hr <= self.canvas[0] and wr <= self.canvas[1], "a rotated image does not fit the canvas"
        if self.patch_size is not None:
            assert self.canvas[0] % self.patch_size == 0 and self.canvas[1] % self.patch_size == 0
        self._table_host = None
        self._table_dev = None

    def __len__(self):
        return len(self.sources)

    @property
    def uint8(self) -> bool:
        return self.dtype == torch.uint8

    def grid_extents(self, patch_size: int) -> Tensor:
        """int32 [B, 2] = (ceil(rotated_h / P), ceil(rotated_w / P)): the patch grid of every image padded on its own
        (infer.py:138-146), which ``NeedleGeneralEnv(..., clamp_to_image=True)`` keeps its agent inside.  Translated
        views have no such grid (the shift moves the image across it)."""
        assert not self.ty.any() and not self.tx.any(), "grid extents are defined for views without translation"
        P = int(patch_size)
        return torch.tensor([[-(-h // P), -(-w // P)] for h, w in self.rotated_hw], dtype=torch.int32)

    # ---- the reference's draws ---------------------------------------------------------------------------
    @classmethod
    def sample(cls, images, bboxes: Tensor, rotations: bool, translations: bool, rng: np.random.Generator,
               patch_size: int) -> "ImageViews":
        """Draw one view per image in the reference's order with its calls on the numpy Generator
        (``transform``, src/dataset.py:274-278): the angle with ``rng.choice(np.arange(4), (1,))`` when `rotations`,
        then x and y of the shift with ``rng.integers(-margin_ul, margin_br, (1,))`` when `translations`, margins
        from the rotated boxes (:165-180), no draw where both margins of an axis are 0.  An image without boxes gets
        no translation and no draw (the reference's ``min([])`` raises there)."""
        srcs = [images[i] for i in range(images.shape[0])] if isinstance(images, Tensor) else list(images)
        bb = np.asarray(bboxes.cpu(), np.int64) if bboxes is not None and bboxes.numel() else np.zeros((len(srcs), 0, 4), np.int64)
        rot, ty, tx = [], [], []
        for i, im in enumerate(srcs):
            Hs, Ws = int(im.shape[1]), int(im.shape[2])
            angle = 0
            if rotations:
                angle = ANGLES[int(rng.choice(np.arange(len(ANGLES)), (1,))[0])]
            t_x = t_y = 0
            real = bb[i][np.any(bb[i] != 0, axis=1)] if bb.shape[1] else bb[i]
            if translations and len(real):
                Hr, Wr = _rotated_hw(Hs, Ws, angle)
                ulx, uly, brx, bry = translate_margins(rotate_boxes(real, Hs, Ws, angle), Hr, Wr)
                if not (ulx == 0 and brx == 0):
                    t_x = int(rng.integers(-ulx, brx, (1,))[0])
                if not (uly == 0 and bry == 0):
                    t_y = int(rng.integers(-uly, bry, (1,))[0])
            rot.append(angle), ty.append(t_y), tx.append(t_x)
        return cls(images, rot, ty, tx, patch_size=patch_size)

    def transform_bboxes(self, bboxes: Tensor) -> Tensor:
        """[B, nb, 4] boxes of the stored images -> boxes on the canvas: ``rotate``'s formulas, then + (tx, ty)
        (src/dataset.py:113-153, 213-225).  All-zero rows are padding and stay zero."""
        bb = np.asarray(bboxes.cpu(), np.int64)
        assert bb.ndim == 3 and bb.shape[0] == len(self) and bb.shape[2] == 4
        out = np.zeros_like(bb)
        for i, (Hs, Ws) in enumerate(self.stored_hw):
            real = np.any(bb[i] != 0, axis=1)
            if real.any():
                r = rotate_boxes(bb[i][real], Hs, Ws, int(self.rot[i]))
                out[i][real] = r + np.array([self.tx[i], self.ty[i], self.tx[i], self.ty[i]], np.int64)
        return torch.from_numpy(out).to(bboxes.device)

    # ---- the oracle --------------------------------------------------------------------------------------
    def materialize(self) -> Tensor:
        """The augmented canvas [B, 3, Hc, Wc] in the sources' element type, with torch ops in the reference's order:
        rotate (transpose + flip), shift with zero fill, pad bottom / right."""
        Hc, Wc = self.canvas
        out = torch.zeros((len(self), 3, Hc, Wc), dtype=self.dtype, device=self.device)
        for i, im in enumerate(self.sources):
            rot, ty, tx = int(self.rot[i]), int(self.ty[i]), int(self.tx[i])
            if rot == 90:
                im = torch.flip(torch.transpose(im, 1, 2), [2])
            elif rot == 180:
                im = torch.flip(im, [1, 2])
            elif rot == 270:
                im = torch.flip(torch.transpose(im, 1, 2), [1])
            Hr, Wr = im.shape[1:]
            # F.affine(angle=0, translate=[tx, ty], fill=0) on whole pixels: out[y, x] = in[y - ty, x - tx] or 0
            y0, y1, x0, x1 = max(ty, 0), min(Hr + ty, Hr), max(tx, 0), min(Wr + tx, Wr)
            if y0 < y1 and x0 < x1:
                out[i, :, y0:y1, x0:x1] = im[:, y0 - ty:y1 - ty, x0 - tx:x1 - tx]
        return out

    # ---- the device table --------------------------------------------------------------------------------
    def table_host(self):
        """ctypes array of jn_image_view (what jn_env_init_views takes)."""
        from ._lib import JnImageView
        if self._table_host is None:
            assert self.device.type == "cuda", "the view table points at device images"
            arr = (JnImageView * len(self))()
            for i, im in enumerate(self.sources):
                Hs, Ws = self.stored_hw[i]
                arr[i] = JnImageView(im.data_ptr(), int(self.uint8), Hs, Ws, int(self.rot[i]), int(self.ty[i]), int(self.tx[i]))
            self._table_host = arr
        return self._table_host

    def table_dev(self) -> Tensor:
        """The same table as a uint8 device tensor (what jn_gather_patches_views takes); validated above."""
        if self._table_dev is None:
            raw = np.frombuffer(bytes(self.table_host()), np.uint8).copy()
            self._table_dev = torch.from_numpy(raw).to(self.device)
        return self._table_dev

    def gather(self, image_index: Tensor, positions: Tensor, patch_size: int, out_uint8: bool = False,
               _check_positions: bool = True) -> Tensor:
        """out[n] = canvas[image_index[n], :, y*P:(y+1)*P, x*P:(x+1)*P] (negative index: zero patch) without the canvas.
        fp32 out (bytes as byte / 255), or with `out_uint8` the transformed bytes of uint8 sources.
        _check_positions (internal): as in ``trajectory.gather_indexed``."""
        from . import _lib
        from ._lib import check, ptr
        P = int(patch_size)
        Hc, Wc = self.canvas
        assert Hc % P == 0 and Wc % P == 0, "the canvas is not a multiple of the patch size"
        assert not out_uint8 or self.uint8, "a byte output needs byte sources"
        ii = image_index.to(self.device, torch.int64).contiguous()
        pos = positions.to(self.device, torch.int64).contiguous()
        N = int(ii.numel())
        if N and _check_positions:
            pc, ic = pos.cpu(), ii.cpu()
            assert bool(((pc[:, 0] >= 0) & (pc[:, 0] < Hc // P) & (pc[:, 1] >= 0) & (pc[:, 1] < Wc // P)).all()), "position outside the grid"
            assert bool((ic < len(self)).all()), "image index out of range"
        out = torch.empty((N, 3, P, P), device=self.device, dtype=torch.uint8 if out_uint8 else torch.float32)
        if N == 0:
            return out
        lib = _lib.load_library()
        check(lib.jn_gather_patches_views(ptr(self.table_dev()), len(self), ptr(ii), ptr(pos), ptr(out), int(out_uint8), N, Hc, Wc,
                                          P, _lib.current_stream(self.device)), "jn_gather_patches_views")
        return out


def stack_bboxes(bboxes, n: int) -> Tensor:
    """[B, nb, 4] int64 from a tensor or a list of [ni, 4] tensors / lists (zero rows pad to the longest)."""
    if isinstance(bboxes, Tensor):
        return bboxes.to(torch.int64).reshape(n, -1, 4)
    rows = [torch.as_tensor(b, dtype=torch.int64).reshape(-1, 4) for b in bboxes]
    nb = max([r.shape[0] for r in rows] + [0])
    return torch.stack([torch.nn.functional.pad(r, (0, 0, 0, nb - r.shape[0])) for r in rows]) if rows else torch.zeros((0, 0, 4), dtype=torch.int64)


def trainer_views(trainer, images, bboxes, patch_size: int):
    """The views a trainer draws for one batch when ``config.rotations`` / ``config.translations`` ask for them
    (main.py:314-315), else None.  One numpy Generator per trainer, seeded like its other per-rank draws
    (``config.seed + 17 * rank``) and consumed batch after batch."""
    cfg = trainer.config
    rotations, translations = bool(getattr(cfg, "rotations", False)), bool(getattr(cfg, "translations", False))
    if not (rotations or translations):
        return None
    if getattr(trainer, "_view_rng", None) is None:
        trainer._view_rng = np.random.default_rng(int(getattr(cfg, "seed", 0)) + 17 * int(getattr(trainer, "rank", 0)))
    n = images.shape[0] if isinstance(images, Tensor) else len(images)
    return ImageViews.sample(images, stack_bboxes(bboxes, n), rotations, translations, trainer._view_rng, patch_size)
