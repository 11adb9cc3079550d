"""CPU restatement of the image-view pixel mapping (include/jnroll.h: jn_image_view), one index computation per canvas
pixel, written from the definition and independent of ``ImageViews.materialize`` (which uses transpose / flip / slices).
"""
import numpy as np


def canvas_ref(src: np.ndarray, rot: int, ty: int, tx: int, Hc: int, Wc: int) -> np.ndarray:
    """src [3, Hs, Ws] -> canvas [3, Hc, Wc] of the same dtype."""
    _, Hs, Ws = src.shape
    Hr, Wr = (Ws, Hs) if rot in (90, 270) else (Hs, Ws)
    Y, X = np.meshgrid(np.arange(Hc), np.arange(Wc), indexing="ij")
    y1, x1 = Y - ty, X - tx
    inside = (Y < Hr) & (X < Wr) & (y1 >= 0) & (y1 < Hr) & (x1 >= 0) & (x1 < Wr)
    if rot == 0:
        sy, sx = y1, x1
    elif rot == 90:
        sy, sx = Hs - 1 - x1, y1
    elif rot == 180:
        sy, sx = Hs - 1 - y1, Ws - 1 - x1
    elif rot == 270:
        sy, sx = x1, Ws - 1 - y1
    else:
        raise ValueError(rot)
    sy, sx = np.where(inside, sy, 0), np.where(inside, sx, 0)
    return np.where(inside[None], src[:, sy, sx], np.zeros((), src.dtype))


def shift_zero_fill(img: np.ndarray, ty: int, tx: int) -> np.ndarray:
    """Whole-pixel shift down / right by (ty, tx) with zero fill: F.affine(angle=0, translate=[tx, ty], fill=0)."""
    out = np.zeros_like(img)
    H, W = img.shape[1:]
    for y in range(H):
        for x in range(W):
            if 0 <= y - ty < H and 0 <= x - tx < W:
                out[:, y, x] = img[:, y - ty, x - tx]
    return out
