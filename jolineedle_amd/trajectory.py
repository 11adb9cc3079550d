"""Teacher trajectories for the supervised step: ``NeedleSimpleEnv`` of the reference
(src/env/simple_env.py:166-764) re-designed as an INDEX generator + one device gather.

The reference walks one image on the host, slicing a [C, P, P] patch out of a CPU image at every step and stacking
them (a 241 MB image per sample crosses PCIe first).  Here the walk produces only integers — grid positions,
actions taken, teacher actions, labels, local boxes — and the patches of a whole batch of trajectories are gathered
from the device-resident images by ONE ``jn_gather_patches_indexed`` launch (bit-exact strided copy; masked steps
are zero patches exactly like the reference's zero-initialised sample).

Random streams are consumed in the reference's order (``numpy.random.default_rng(seed)`` for positions / keypoints /
STOP replacement, Python's ``random`` for nearest-neighbour ties), so a seeded walk reproduces the reference's —
tests/golden/g8_trajectories.npz holds walks recorded from the reference itself.

Positions are (y, x) tuples on the patch grid; boxes are pixel (x1, y1, x2, y2).
"""
import random as _random
from itertools import product
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from .common import ACTION_DELTAS, MOVES, Action

Pos = Tuple[int, int]

_BY_SIGN = {  # (sign dy, sign dx) -> action       (move_towards, src/env/simple_env.py:84-125)
    (1, 0): Action.DOWN, (-1, 0): Action.UP, (0, 1): Action.RIGHT, (0, -1): Action.LEFT,
    (-1, 1): Action.RIGHT_UP, (-1, -1): Action.LEFT_UP, (1, 1): Action.RIGHT_DOWN, (1, -1): Action.LEFT_DOWN,
    (0, 0): Action.STOP,
}


def _sign(v: int) -> int:
    return (v > 0) - (v < 0)


def move_towards(current: Pos, target: Pos) -> Action:
    """One king's-move step from `current` towards `target` (STOP when already there)."""
    return _BY_SIGN[(_sign(target[0] - current[0]), _sign(target[1] - current[1]))]


def _boxes_xyxy(bboxes) -> List[Tuple[int, int, int, int]]:
    """Accepts an [n, 4] xyxy tensor / array or the reference's list of BBox(up_left=(y, x), bottom_right=(y, x))."""
    if isinstance(bboxes, (torch.Tensor, np.ndarray)):
        return [tuple(int(v) for v in row) for row in np.asarray(bboxes.cpu() if isinstance(bboxes, torch.Tensor) else bboxes).reshape(-1, 4)]
    out = []
    for b in bboxes:
        (y1, x1), (y2, x2) = b
        out.append((int(x1), int(y1), int(x2), int(y2)))
    return out


class NeedleSimpleEnv:
    """Single-image teacher.  `image` may be None (index generation only), a [C, H, W] tensor, or — to share one
    device batch between many envs — a ([B, C, H, W] tensor, image index) pair."""

    def __init__(self, image, patch_size: int, bboxes, seed: Optional[int] = None, height: Optional[int] = None,
                 width: Optional[int] = None, py_random=None):
        self.patch_size = int(patch_size)
        self.rng = np.random.default_rng(seed)
        self.py_random = py_random if py_random is not None else _random
        self.raw_bboxes = _boxes_xyxy(bboxes)
        self.image, self.image_index = None, 0
        if image is not None:
            if isinstance(image, tuple):
                self.image, self.image_index = image[0], int(image[1])
            else:
                self.image = image[None]
            self.n_channels, self.height, self.width = (int(s) for s in self.image.shape[1:])
        else:
            assert height is not None and width is not None, "image or (height, width) required"
            self.n_channels, self.height, self.width = 3, int(height), int(width)
        P = self.patch_size
        self.patch_height, self.patch_width = self.height // P, self.width // P
        # boxes on the patch grid, (y1, x1, y2, x2) inclusive
        self.bboxes = [(y1 // P, x1 // P, y2 // P, x2 // P) for x1, y1, x2, y2 in self.raw_bboxes]
        self.position: Pos = (0, 0)
        self.bbox_patches: Set[Pos] = set()
        for box in self.raw_bboxes:
            self.bbox_patches = self.bbox_patches | self.bbox_positions(box)
        self.visited_bbox_patches: Set[Pos] = set()

    # ---- geometry -------------------------------------------------------------------------------------
    def bbox_positions(self, box, area_threshold: float = 0.05) -> Set[Pos]:
        """Grid cells holding more than `area_threshold` of a patch area of the box, plus the cell of the box centre,
        restricted to the grid (src/env/simple_env.py:270-321)."""
        P = self.patch_size
        x1, y1, x2, y2 = box
        cells: Set[Pos] = set()
        for y, x in product(range(y1 // P, y2 // P + 1), range(x1 // P, x2 // P + 1)):
            h = min((y + 1) * P, y2) - max(y * P, y1)
            w = min((x + 1) * P, x2) - max(x * P, x1)
            if h * w / (P ** 2) > area_threshold:
                cells.add((y, x))
        cells.add((((y1 + y2) // 2) // P, ((x1 + x2) // 2) // P))
        cells = {c for c in cells if 0 <= c[1] < self.patch_width}
        cells = {c for c in cells if 0 <= c[0] < self.patch_height}
        return cells

    def local_bboxes(self, position: Optional[Pos] = None) -> np.ndarray:
        """[n_boxes, 6] rows (class 0, x1, y1, x2, y2 relative to the patch, objectness 1) of the parts of the raw
        boxes inside the patch at `position`; zero rows where there is no overlap (src/env/simple_env.py:231-268)."""
        y, x = self.position if position is None else position
        P = self.patch_size
        px, py = x * P, y * P
        out = np.zeros((len(self.raw_bboxes), 6), dtype=np.float32)
        for i, (x1, y1, x2, y2) in enumerate(self.raw_bboxes):
            cx1, cy1, cx2, cy2 = max(px, x1), max(py, y1), min(px + P, x2), min(py + P, y2)
            if cx1 < cx2 and cy1 < cy2:
                out[i] = (0, cx1 - px, cy1 - py, cx2 - px, cy2 - py, 1)
        return out

    # ---- walking --------------------------------------------------------------------------------------
    def reset(self, position: Optional[Pos] = None, visited_bbox_patches: Optional[Set[Pos]] = None) -> Dict:
        if position is None:
            y = int(self.rng.integers(low=0, high=self.patch_height))
            x = int(self.rng.integers(low=0, high=self.patch_width))
            position = (y, x)
        self.position = (int(position[0]), int(position[1]))
        self.visited_bbox_patches = set() if visited_bbox_patches is None else visited_bbox_patches
        if self.position in self.bbox_patches:
            self.visited_bbox_patches.add(self.position)
        return self.gather_infos()

    def step(self, move) -> Dict:
        move = move if isinstance(move, Action) else Action(int(move))
        dy, dx = ACTION_DELTAS[move]
        self.position = (min(max(self.position[0] + dy, 0), self.patch_height - 1),
                         min(max(self.position[1] + dx, 0), self.patch_width - 1))
        if self.position in self.bbox_patches:
            self.visited_bbox_patches.add(self.position)
        return self.gather_infos()

    def gather_infos(self) -> Dict:
        return {"position": self.position, "number_patches_found": len(self.visited_bbox_patches),
                "local_bboxes": self.local_bboxes(), "inside_bbox": self.position in self.bbox_patches}

    def remove_stop_action(self, action: Action) -> Action:
        return MOVES[int(self.rng.choice(len(MOVES)))] if action is Action.STOP else action

    def generate_keypoints(self, n: int) -> List[Pos]:
        pts = []
        for _ in range(n):
            y = int(self.rng.integers(0, self.patch_height))
            x = int(self.rng.integers(0, self.patch_width))
            pts.append((y, x))
        return pts

    def generate_binomial_keypoints(self, n: int, target: Pos) -> List[Pos]:
        """Binomial(grid, 1/2) displacement around `target`, wrapping on the grid (src/env/simple_env.py:684-713)."""
        pts = []
        for _ in range(n):
            dx = int(self.rng.binomial(self.patch_width, 0.5)) - self.patch_width // 2
            dy = int(self.rng.binomial(self.patch_height, 0.5)) - self.patch_height // 2
            pts.append(((target[0] + dy) % self.patch_height, (target[1] + dx) % self.patch_width))
        return pts

    def build_keypoints_trajectory(self) -> List[Pos]:
        """Greedy nearest-neighbour (L1) order over the not-yet-visited box cells, ties broken by Python's `random`;
        one random cell when there is nothing to visit (src/env/simple_env.py:590-629)."""
        todo: Set[Pos] = set()
        for box in self.raw_bboxes:
            todo |= self.bbox_positions(box)
        for p in self.visited_bbox_patches:
            todo.remove(p)
        order, cur = [], self.position
        while todo:
            best, nearest = None, []
            for p in todo:
                d = abs(p[1] - cur[1]) + abs(p[0] - cur[0])
                if best is None or d < best:
                    best, nearest = d, []
                if d == best:
                    nearest.append(p)
            cur = self.py_random.choice(nearest)
            order.append(cur)
            todo.remove(cur)
        if not order:
            order.append(self.generate_keypoints(1)[0])
        return order

    # ---- samples --------------------------------------------------------------------------------------
    def detection_cells(self) -> List[Pos]:
        """Cells whose patches feed the detector loss: every box cell plus one random empty cell
        (init_sample, src/env/simple_env.py:397-419)."""
        cells: Set[Pos] = set()
        for box in self.raw_bboxes:
            for p in self.bbox_positions(box):
                cells.add(p)
        empty = [(y, x) for y, x in product(range(self.patch_height), range(self.patch_width)) if (y, x) not in cells]
        if empty:
            cells.add(empty[int(self.rng.choice(len(empty)))])
        return list(cells)

    def generate_sample_indices(self, max_ep_len: int, min_keypoints: int, max_keypoints: int,
                                binomial_keypoints: bool = False, position: Optional[Pos] = None,
                                visited_bbox_patches: Optional[Set[Pos]] = None) -> Dict[str, np.ndarray]:
        """The integer part of ``generate_sample`` (src/env/simple_env.py:481-588): positions [T, 2], current_actions,
        next_actions, labels [T] int64, masks [T] f32, local_bboxes [T, nb, 6] f32, plus positions_yolox [M, 2] and
        bboxes_yolox [M, nb, 6].  Episodes longer than `max_ep_len` keep their LAST `max_ep_len` steps."""
        det_cells = self.detection_cells()
        steps: List[Tuple[int, int, Pos, int, np.ndarray]] = []      # (action taken, teacher action, pos, label, boxes)

        info = self.reset(position, visited_bbox_patches)
        steps.append((Action.LEFT.value, Action.LEFT.value, info["position"], int(info["inside_bbox"]), info["local_bboxes"]))

        def visit(to_visit: Pos, true_target: Pos):
            self.reset(self.position)
            while self.position != to_visit:
                action = move_towards(self.position, to_visit)
                inf = self.step(action)
                best = self.remove_stop_action(move_towards(self.position, true_target))
                self.reset(self.position)
                steps.append((action.value, best.value, inf["position"], int(inf["inside_bbox"]), inf["local_bboxes"]))

        keypoints = self.build_keypoints_trajectory()
        n_extra = int(self.rng.integers(min_keypoints, max_keypoints + 1))
        insert_at = sorted((int(v) for v in self.rng.integers(0, len(keypoints), size=n_extra)), reverse=True)
        for kid, kp in enumerate(keypoints):
            # the teacher action of the last recorded step now points at this keypoint
            a, _, p, lab, lb = steps[-1]
            steps[-1] = (a, self.remove_stop_action(move_towards(self.position, kp)).value, p, lab, lb)
            while kid in insert_at:
                detour = self.generate_binomial_keypoints(1, kp)[0] if binomial_keypoints else self.generate_keypoints(1)[0]
                visit(detour, kp)
                insert_at.remove(kid)
            visit(kp, kp)

        if len(steps) > max_ep_len:
            steps = steps[len(steps) - max_ep_len:]
        T, nb, n = int(max_ep_len), len(self.raw_bboxes), len(steps)
        out = {"positions": np.zeros((T, 2), np.int64), "current_actions": np.zeros(T, np.int64),
               "next_actions": np.zeros(T, np.int64), "labels": np.zeros(T, np.int64), "masks": np.zeros(T, np.float32),
               "local_bboxes": np.zeros((T, nb, 6), np.float32)}
        for i, (a, best, p, lab, lb) in enumerate(steps):
            out["current_actions"][i], out["next_actions"][i], out["labels"][i] = a, best, lab
            out["positions"][i] = p
            out["local_bboxes"][i] = lb
        out["masks"][:n] = 1.0
        out["positions_yolox"] = np.asarray(det_cells, np.int64).reshape(-1, 2)
        out["bboxes_yolox"] = (np.stack([self.local_bboxes(p) for p in det_cells]) if det_cells
                               else np.zeros((0, nb, 6), np.float32)).astype(np.float32)
        return out

    def generate_sample(self, max_ep_len: int, min_keypoints: int, max_keypoints: int, binomial_keypoints: bool = False,
                        position: Optional[Pos] = None, visited_bbox_patches: Optional[Set[Pos]] = None,
                        device=None) -> Dict[str, torch.Tensor]:
        """The reference's sample dict; patches / patches_yolox gathered on the device that holds the image."""
        assert self.image is not None, "generate_sample needs the image (device tensor); use generate_sample_indices"
        idx = self.generate_sample_indices(max_ep_len, min_keypoints, max_keypoints, binomial_keypoints, position,
                                           visited_bbox_patches)
        return assemble_samples(self.image, [self.image_index], [idx], self.patch_size, stacked=False)


def teacher_action_sets(positions: torch.Tensor, visited: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """The teacher's opinion of B states as action sets, uint8 [B] (host, torch CPU): the deterministic object behind the
    first ``random.choice`` of ``build_keypoints_trajectory``.  positions [B, 2] (y, x); visited, targets [B, Gh, Gw]
    (non-zero = set).  The remaining targets of agent b are ``targets[b] & ~visited[b]``, N those at the minimum L1
    distance, and bit a of the byte is set when action a = ``move_towards(position, q)`` for some q in N (actions 0..7;
    STOP, which ``remove_stop_action`` replaces by a random move, is never a member).  0: nothing left to visit (the
    reference then walks to a random cell and no action is "right")."""
    pos = positions.to("cpu", torch.int64).reshape(-1, 2)
    left = (targets.to("cpu") != 0) & ~(visited.to("cpu") != 0)
    B, Gh, Gw = left.shape
    assert pos.shape[0] == B
    dy = torch.arange(Gh).view(1, Gh, 1) - pos[:, 0].view(B, 1, 1)
    dx = torch.arange(Gw).view(1, 1, Gw) - pos[:, 1].view(B, 1, 1)
    dist = dy.abs() + dx.abs()                                          # [B, Gh, Gw]
    far = Gh + Gw
    dist = torch.where(left, dist, torch.full_like(dist, far))
    nearest = left & (dist == dist.amin(dim=(1, 2), keepdim=True))
    sets = torch.zeros(B, dtype=torch.int64)
    for (sy, sx), action in _BY_SIGN.items():
        if action is Action.STOP:
            continue
        hit = nearest & (dy.sign() == sy) & (dx.sign() == sx)
        sets |= hit.any(dim=2).any(dim=1).to(torch.int64) << action.value
    return sets.to(torch.uint8)


def teacher_action_sets_device(positions: torch.Tensor, visited: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """``teacher_action_sets`` in one launch (``jn_teacher_actions``, one wave per agent) on device tensors: positions
    [B, 2] int64, visited / targets [B, Gh, Gw] bool or uint8; returns uint8 [B] on the device without a readback."""
    from . import _lib
    from ._lib import check, ptr
    assert positions.is_cuda and visited.is_cuda and targets.is_cuda, "device tensors required (host: teacher_action_sets)"
    dev = positions.device
    pos = positions.to(torch.int64).reshape(-1, 2).contiguous()
    vis, tg = visited.to(torch.uint8).contiguous(), targets.to(torch.uint8).contiguous()
    B, Gh, Gw = tg.shape
    assert pos.shape[0] == B and vis.shape == tg.shape
    out = torch.empty((B,), device=dev, dtype=torch.uint8)
    if B:
        check(_lib.load_library().jn_teacher_actions(ptr(pos), ptr(vis), ptr(tg), B, Gh, Gw, ptr(out),
                                                     _lib.current_stream(dev)), "jn_teacher_actions")
    return out


def teacher_agreement(sets: torch.Tensor, actions: torch.Tensor) -> float:
    """Share of the steps with a non-empty teacher set whose action is a member of it (sets uint8 [S], actions [S]);
    0.0 when there is no such step (the reference zeroes the NaN of an empty mean, src/supervised.py:390-396)."""
    sets, actions = sets.to("cpu", torch.int64).flatten(), actions.to("cpu", torch.int64).flatten()
    judged = sets != 0
    if not bool(judged.any()):
        return 0.0
    member = ((sets >> actions.clamp(max=62)) & 1).bool()
    return float((member & judged).sum()) / float(judged.sum())


def simple_env_targets(bboxes, height: int, width: int, patch_size: int) -> torch.Tensor:
    """uint8 [height // P, width // P]: the cells ``NeedleSimpleEnv`` counts as targets (``bbox_positions`` with its
    area threshold, plus each box's centre cell), for xyxy boxes of an image of height x width pixels."""
    env = NeedleSimpleEnv(None, patch_size, bboxes, height=height, width=width)
    grid = torch.zeros((env.patch_height, env.patch_width), dtype=torch.uint8)
    for y, x in env.bbox_patches:
        grid[y, x] = 1
    return grid


def gather_indexed(images: torch.Tensor, image_index: torch.Tensor, positions: torch.Tensor, patch_size: int,
                   views=None, _check_positions: bool = True) -> torch.Tensor:
    """out[n] = images[image_index[n], :, y*P:(y+1)*P, x*P:(x+1)*P]; a negative image index gives a zero patch.
    uint8 images are read in place and give byte / 255 (fp32, as ToTensor computes it).
    views: an ``ImageViews`` — the patches are cut from its augmented canvas instead (`images` is not used).
    _check_positions (internal): False skips the host-side asserts, and the readback they cost, for indices and
    positions that are valid by construction (the cells ``jn_detection_cells`` names)."""
    if views is not None:
        return views.gather(image_index, positions, patch_size, _check_positions=_check_positions)
    from . import _lib
    from ._lib import check, ptr
    assert images.is_cuda and images.dtype in (torch.float32, torch.uint8) and images.is_contiguous(), \
        "images must be a contiguous f32 or uint8 device tensor"
    nimg, Cc, H, W = images.shape
    P = int(patch_size)
    assert H % P == 0 and W % P == 0
    ii = image_index.to(images.device, torch.int64).contiguous()
    pos = positions.to(images.device, torch.int64).contiguous()
    N = int(ii.numel())
    if N and _check_positions:
        ph, pw = H // P, W // P
        pc, ic = pos.cpu(), ii.cpu()
        assert bool(((pc[:, 0] >= 0) & (pc[:, 0] < ph) & (pc[:, 1] >= 0) & (pc[:, 1] < pw)).all()), "position outside the grid"
        assert bool((ic < nimg).all()), "image index out of range"
    out = torch.empty((N, Cc, P, P), device=images.device, dtype=torch.float32)
    lib = _lib.load_library()
    if N == 0:                                # empty tensors have no storage to point at
        return out
    fn = lib.jn_gather_patches_indexed_u8 if images.dtype == torch.uint8 else lib.jn_gather_patches_indexed
    check(fn(ptr(images), ptr(ii), ptr(pos), ptr(out), N, nimg, Cc, H, W, P,
             _lib.current_stream(images.device)), "jn_gather_patches_indexed")
    return out


def assemble_samples(images: torch.Tensor, image_ids: Sequence[int], indices: Sequence[Dict[str, np.ndarray]],
                     patch_size: int, stacked: bool = True, views=None) -> Dict[str, torch.Tensor]:
    """Turn per-image index dicts into the reference's (collated) tensors with two device gathers: trajectory patches
    [B, T, C, P, P] and detector patches [sum M_i, C, P, P]; boxes are zero-row padded to the longest list
    (NeedleSimpleEnv.collate_fn, src/env/simple_env.py:720-763)."""
    dev = images.device if views is None else views.device
    B, T = len(indices), indices[0]["masks"].shape[0]
    nb = max(int(d["local_bboxes"].shape[1]) for d in indices)

    def pad(a):
        return a if a.shape[1] == nb else np.concatenate([a, np.zeros((a.shape[0], nb - a.shape[1], 6), np.float32)], 1)

    ii = np.concatenate([np.where(d["masks"] > 0, i, -1) for i, d in zip(image_ids, indices)]).astype(np.int64)
    pos = np.concatenate([d["positions"] for d in indices])
    patches = gather_indexed(images, torch.from_numpy(ii), torch.from_numpy(pos), patch_size, views=views)
    iy = np.concatenate([np.full(d["positions_yolox"].shape[0], i, np.int64) for i, d in zip(image_ids, indices)])
    py = np.concatenate([d["positions_yolox"] for d in indices])
    out = {"patches": patches.view(B, T, *patches.shape[1:]),
           "patches_yolox": gather_indexed(images, torch.from_numpy(iy), torch.from_numpy(py), patch_size, views=views),
           "bboxes_yolox": torch.from_numpy(np.concatenate([pad(d["bboxes_yolox"]) for d in indices])).to(dev)}
    for k in ("current_actions", "next_actions", "positions", "masks", "labels"):
        out[k] = torch.from_numpy(np.stack([d[k] for d in indices])).to(dev)
    out["local_bboxes"] = torch.from_numpy(np.stack([pad(d["local_bboxes"]) for d in indices])).to(dev)
    if not stacked:
        assert B == 1
        out = {k: (v if k in ("patches_yolox", "bboxes_yolox") else v[0]) for k, v in out.items()}
    return out


# ---- teacher walks of a whole batch: the host statement of ``jn_teacher_walks`` and its device twin ------------------------
WALK_TAG_R = 0x54574B52          # third Philox counter word of stream R (the role of NeedleSimpleEnv.rng)
WALK_TAG_Y = 0x54574B59          # ... of stream Y (the role of py_random: the tie choice among equally near targets)
MAX_WALK_CELLS = 4096            # JN_TWALK_MAX_CELLS: cells per image the walk kernel keeps in LDS
MAX_WALK_STEPS = 4096            # JN_TWALK_MAX_T: steps of the kernel's LDS ring
MAX_WALK_KEYPOINTS = 64          # JN_TWALK_MAX_KEYPOINTS: the kernel's detour table, one lane per detour


class PhiloxDraws:
    """A counter-based stand-in for ``numpy.random.Generator`` / Python's ``random`` in ``NeedleSimpleEnv``: draw k is
    ``philox4x32(seed; image, k, tag, 0).x`` (csrc/jn_device.h, ``ragged._philox4x32``), k counting the draws made."""

    def __init__(self, seed: int, image: int, tag: int):
        self.seed, self.image, self.tag, self.k = int(seed) & 0xFFFFFFFFFFFFFFFF, int(image), int(tag), 0

    def draw(self) -> int:
        from .ragged import _philox4x32
        r = _philox4x32(self.seed, self.image, self.k, self.tag, 0)[0]
        self.k += 1
        return r

    def integers(self, low, high=None, size=None):
        """lo + r % (hi - lo), one draw; with `size` n draws in order (none for n = 0)."""
        if high is None:
            low, high = 0, low
        low, high = int(low), int(high)
        if size is None:
            return low + self.draw() % (high - low)
        return np.array([low + self.draw() % (high - low) for _ in range(int(size))], dtype=np.int64)

    def choice(self, options):
        """An int n: r % n.  A list: element r % len of the list sorted (cells: row-major).  One draw either way."""
        if isinstance(options, (int, np.integer)):
            return self.draw() % int(options)
        options = sorted(options)
        return options[self.draw() % len(options)]

    def binomial(self, n, p=0.5) -> int:
        """Binomial(n, 1/2) as the set bits among n random bits: ceil(n / 32) draws, draw j supplies bits 32j .. 32j + 31,
        the last one its low n - 32j bits."""
        assert p == 0.5, "only the fair coin is a bit count"
        n, total = int(n), 0
        for j in range((n + 31) // 32):
            bits = min(32, n - 32 * j)
            total += bin(self.draw() & ((1 << bits) - 1)).count("1")
        return total


def _walk_targets(boxes, gh: int, gw: int, P: int) -> np.ndarray:
    """uint8 [gh, gw]: ``bbox_positions`` of every box on integers — cell (y, x) of the box's own cell range with
    20 * h * w > P * P (h * w / P**2 > 0.05), plus the cell of its centre; cells outside the grid are dropped."""
    grid = np.zeros((gh, gw), np.uint8)
    for x1, y1, x2, y2 in boxes:
        for y in range(max(y1 // P, 0), min(y2 // P, gh - 1) + 1):
            for x in range(max(x1 // P, 0), min(x2 // P, gw - 1) + 1):
                h = min((y + 1) * P, y2) - max(y * P, y1)
                w = min((x + 1) * P, x2) - max(x * P, x1)
                if 20 * h * w > P * P:
                    grid[y, x] = 1
        cy, cx = ((y1 + y2) // 2) // P, ((x1 + x2) // 2) // P
        if 0 <= cy < gh and 0 <= cx < gw:
            grid[cy, cx] = 1
    return grid


def _walk_local_bboxes(boxes, nb: int, P: int, y: int, x: int) -> np.ndarray:
    """f32 [nb, 6]: ``NeedleSimpleEnv.local_bboxes`` at cell (y, x); the rows past len(boxes) are zero."""
    out = np.zeros((nb, 6), np.float32)
    px, py = x * P, y * P
    for j, (x1, y1, x2, y2) in enumerate(boxes):
        cx1, cy1, cx2, cy2 = max(px, x1), max(py, y1), min(px + P, x2), min(py + P, y2)
        if cx1 < cx2 and cy1 < cy2:
            out[j] = (0, cx1 - px, cy1 - py, cx2 - px, cy2 - py, 1)
    return out


_TOWARDS = (4, 2, 5, 0, 8, 1, 6, 3, 7)      # action id at [(sign dy + 1) * 3 + sign dx + 1] (csrc/jn_device.h: kTowards)
_DELTA_Y = (0, 0, -1, 1, -1, -1, 1, 1, 0)
_DELTA_X = (-1, 1, 0, 0, -1, 1, -1, 1, 0)


def teacher_walks(bboxes, gh: int, gw: int, P: int, T: int, min_keypoints: int, max_keypoints: int,
                  binomial_keypoints: bool, seed: int, start_positions=None) -> Dict[str, torch.Tensor]:
    """The teacher walks of a whole batch on plain integers: the host statement of the rule ``jn_teacher_walks``
    computes (include/jnroll.h) — ``NeedleSimpleEnv.generate_sample_indices`` with its two random sources replaced by the
    Philox streams of ``PhiloxDraws`` (R, tag ``WALK_TAG_R``, for ``rng``; Y, tag ``WALK_TAG_Y``, for the tie choice, which
    picks among the nearest cells in row-major order), per image b of `seed`.  bboxes [B, nb, 4] xyxy int64, nb >= 0; an
    all-zero row is padding and is skipped, column j of every box output is the j-th non-zero row.  start_positions
    [B, 2] (y, x) replaces the random start.  Draw order of R: the negative detector cell (if the image has an empty
    cell), the start (y, x), the one random keypoint (y, x) when nothing is left to visit, the number of detours, their
    places, then the detours (binomial: x before y) and STOP replacements as the walk meets them.

    Returns on the CPU: positions int64 [B, T, 2], current_actions / next_actions / labels int64 [B, T], masks f32 [B, T],
    local_bboxes f32 [B, T, nb, 6], n_steps int32 [B] (the walk's length before the cut to its last T steps), targets
    uint8 [B, gh, gw], cells_yolox int64 [M, 3] = (image, y, x) — per image its target cells in row-major order, then the
    one negative cell — bboxes_yolox f32 [M, nb, 6] and offsets int32 [B + 1]."""
    gh, gw, P, T = int(gh), int(gw), int(P), int(T)
    bb = np.asarray(bboxes.detach().cpu() if isinstance(bboxes, torch.Tensor) else bboxes, dtype=np.int64)
    assert bb.ndim == 3 and bb.shape[2] == 4, "bboxes are [B, nb, 4]"
    B, nb = bb.shape[0], bb.shape[1]
    assert gh >= 1 and gw >= 1 and P >= 1 and T >= 1 and 0 <= int(min_keypoints) <= int(max_keypoints)
    starts = None
    if start_positions is not None:
        starts = np.asarray(torch.as_tensor(start_positions).cpu(), dtype=np.int64).reshape(B, 2)
        assert ((starts >= 0) & (starts < np.array([gh, gw]))).all(), "start position outside the grid"
    out = {"positions": np.zeros((B, T, 2), np.int64), "current_actions": np.zeros((B, T), np.int64),
           "next_actions": np.zeros((B, T), np.int64), "labels": np.zeros((B, T), np.int64),
           "masks": np.zeros((B, T), np.float32), "local_bboxes": np.zeros((B, T, nb, 6), np.float32),
           "n_steps": np.zeros((B,), np.int32), "targets": np.zeros((B, gh, gw), np.uint8)}
    cells_yolox, bboxes_yolox, offsets = [], [], [0]
    for b in range(B):
        boxes = [tuple(int(v) for v in row) for row in bb[b] if any(int(v) != 0 for v in row)]
        R, Y = PhiloxDraws(seed, b, WALK_TAG_R), PhiloxDraws(seed, b, WALK_TAG_Y)
        target = _walk_targets(boxes, gh, gw, P)
        out["targets"][b] = target
        flat = target.reshape(-1)
        rows = [int(c) for c in np.flatnonzero(flat)]
        empty = [int(c) for c in np.flatnonzero(flat == 0)]
        if empty:
            rows.append(empty[R.draw() % len(empty)])
        for c in rows:
            cells_yolox.append((b, c // gw, c % gw))
            bboxes_yolox.append(_walk_local_bboxes(boxes, nb, P, c // gw, c % gw))
        offsets.append(offsets[-1] + len(rows))

        if starts is None:
            y = R.draw() % gh
            x = R.draw() % gw
        else:
            y, x = int(starts[b, 0]), int(starts[b, 1])
        todo = flat.copy()
        todo[y * gw + x] = 0
        n_keypoints = int(todo.sum())
        random_keypoint = None
        if n_keypoints == 0:
            ky = R.draw() % gh
            random_keypoint = (ky, R.draw() % gw)
            n_keypoints = 1
        n_extra = int(min_keypoints) + R.draw() % (int(max_keypoints) + 1 - int(min_keypoints))
        insert_at = [R.draw() % n_keypoints for _ in range(n_extra)]
        steps = [[0, 0, y, x, int(flat[y * gw + x])]]            # action taken, teacher action, y, x, label

        def towards(ty, tx):
            a = _TOWARDS[((ty > y) - (ty < y) + 1) * 3 + (tx > x) - (tx < x) + 1]
            return R.draw() % 8 if a == 8 else a, a

        for kid in range(n_keypoints):
            if random_keypoint is not None:
                ky, kx = random_keypoint
            else:
                left = np.flatnonzero(todo)
                dist = np.abs(left // gw - y) + np.abs(left % gw - x)
                nearest = left[dist == dist.min()]               # row-major
                c = int(nearest[Y.draw() % len(nearest)])
                todo[c] = 0
                ky, kx = c // gw, c % gw
            steps[-1][1] = towards(ky, kx)[0]
            for _ in range(insert_at.count(kid)):                # each detour is walked before the next one is drawn
                if binomial_keypoints:
                    dx = R.binomial(gw) - gw // 2
                    dy = R.binomial(gh) - gh // 2
                    ty, tx = (ky + dy) % gh, (kx + dx) % gw
                else:
                    ty = R.draw() % gh
                    tx = R.draw() % gw
                while (y, x) != (ty, tx):
                    _, a = towards(ty, tx)
                    y, x = y + _DELTA_Y[a], x + _DELTA_X[a]
                    steps.append([a, towards(ky, kx)[0], y, x, int(flat[y * gw + x])])
            while (y, x) != (ky, kx):
                _, a = towards(ky, kx)
                y, x = y + _DELTA_Y[a], x + _DELTA_X[a]
                steps.append([a, towards(ky, kx)[0], y, x, int(flat[y * gw + x])])

        out["n_steps"][b] = len(steps)
        for i, (a, best, sy, sx, lab) in enumerate(steps[-T:]):
            out["current_actions"][b, i], out["next_actions"][b, i], out["labels"][b, i] = a, best, lab
            out["positions"][b, i] = (sy, sx)
            out["masks"][b, i] = 1.0
            out["local_bboxes"][b, i] = _walk_local_bboxes(boxes, nb, P, sy, sx)
    out = {k: torch.from_numpy(v) for k, v in out.items()}
    out["cells_yolox"] = torch.tensor(cells_yolox, dtype=torch.int64).reshape(-1, 3)
    out["bboxes_yolox"] = torch.from_numpy(np.stack(bboxes_yolox) if bboxes_yolox else np.zeros((0, nb, 6), np.float32))
    out["offsets"] = torch.tensor(offsets, dtype=torch.int32)
    return out


def teacher_walks_device(bboxes: torch.Tensor, gh: int, gw: int, P: int, T: int, min_keypoints: int, max_keypoints: int,
                         binomial_keypoints: bool, seed: int, start_positions=None) -> Dict[str, torch.Tensor]:
    """``teacher_walks`` on the device (``jn_teacher_walks``: three launches, no Python loop): bboxes [B, nb, 4] on the
    GPU; the same dict with every tensor on the device except ``offsets``, which is read back once — the one
    synchronisation, for the number of detector rows.  The detector buffers hold B * gh * gw rows, which always suffices.
    start_positions given on the host are checked on the host; given on the device they are read back for the check (a
    second synchronisation).  Beyond ``MAX_WALK_CELLS`` cells, ``MAX_WALK_STEPS`` steps or ``MAX_WALK_KEYPOINTS`` detours
    the entry point refuses."""
    from . import _lib
    from ._lib import check, ptr
    if not bboxes.is_cuda:
        raise RuntimeError("teacher_walks_device needs the boxes on the GPU (teacher_walks is the host function)")
    dev = bboxes.device
    bb = bboxes.to(torch.int64).contiguous()
    assert bb.dim() == 3 and bb.shape[2] == 4, "bboxes are [B, nb, 4]"
    B, nb = int(bb.shape[0]), int(bb.shape[1])
    gh, gw, T = int(gh), int(gw), int(T)
    starts = None
    if start_positions is not None:
        sp = torch.as_tensor(start_positions).to(torch.int64).reshape(B, 2)
        host = sp.cpu()
        assert bool(((host >= 0) & (host < torch.tensor([gh, gw]))).all()), "start position outside the grid"
        starts = sp.to(dev).contiguous()
    cap = B * max(gh, 0) * max(gw, 0)
    Tn = max(T, 0)
    i64 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.int64)
    out = {"positions": i64(B, Tn, 2), "current_actions": i64(B, Tn), "next_actions": i64(B, Tn), "labels": i64(B, Tn),
           "masks": torch.empty((B, Tn), device=dev, dtype=torch.float32),
           "local_bboxes": torch.empty((B, Tn, nb, 6), device=dev, dtype=torch.float32),
           "n_steps": torch.empty((B,), device=dev, dtype=torch.int32),
           "targets": torch.empty((B, max(gh, 0), max(gw, 0)), device=dev, dtype=torch.uint8),
           "cells_yolox": i64(cap, 3), "bboxes_yolox": torch.empty((cap, nb, 6), device=dev, dtype=torch.float32),
           "offsets": torch.empty((B + 1,), device=dev, dtype=torch.int32)}
    names = ("positions", "current_actions", "next_actions", "labels", "masks", "local_bboxes", "n_steps", "targets",
             "cells_yolox", "bboxes_yolox", "offsets")
    check(_lib.load_library().jn_teacher_walks(ptr(bb), ptr(starts), B, nb, gh, gw, int(P), T, int(min_keypoints),
                                               int(max_keypoints), int(bool(binomial_keypoints)),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, cap, *(ptr(out[k]) for k in names),
                                               _lib.current_stream(dev)), "jn_teacher_walks")
    out["offsets"] = out["offsets"].cpu()
    n = int(out["offsets"][B])
    out["cells_yolox"], out["bboxes_yolox"] = out["cells_yolox"][:n], out["bboxes_yolox"][:n]
    return out
