"""Batched inference over images of unequal size: per-agent grid extents inside the engine (jn_env_init_ragged), the
per-image assembly of a rollout's detections on the device (jn_rollout_boxes_to_image), and ``infer_images`` /
``eval_on_images`` built on them.  The yardstick throughout is the per-image loop of the same engine: one ``B = 1`` env
per image padded on its own (infer.py:138-146).

Bars of the rollout comparison: the existing suite holds the engine's logits to 1e-4 and its boxes to 1e-3 px against the
oracle at any batch size, so two runs of the engine are held to twice that against each other.  Equal trajectories
need a stable argmax and a stable confidence cut; both are PRECONDITIONS asserted on the per-image run (top-2 logit gap
>= 1e-3 at every executed step, no candidate score within 1e-2 of the threshold), for every image, none excluded.

The weight and image seeds below were chosen with ``tests/ragged_ref.find_seeds``: the CPU oracle's per-image rollouts
of seeds 0, 1, 2, ... until every image clears both preconditions with a factor 3 to spare and at least one box is found;
the first such seed is committed."""
import ctypes as C

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib, detection, ragged
from jolineedle_amd._lib import JnError, check, ptr
from jolineedle_amd.config import model_config
from jolineedle_amd.engine import Engine, bare_env_config
from jolineedle_amd.views import ImageViews
from tests import ragged_ref
from tests.ragged_ref import LOGIT_GAP, SCORE_GAP, THR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOGIT_BAR, BOX_BAR = 2e-4, 2e-3

# (sizes, seed) found by find_seeds; see the module docstring
SIZES_64 = [(100, 150), (64, 128), (180, 120), (130, 200), (100, 150), (64, 128), (180, 120)]      # seven images, four sizes
SEED_64 = 0
SIZES_448 = [(500, 900), (448, 448), (1000, 600)]
SEED_448 = 0


def _cfg(**kw):
    return ja.CfgNode(max_seq_len=kw.pop("T", 6), entropy_weight=0.01, stop_enabled=kw.pop("stop", True),
                      reward_norm=kw.pop("reward_norm", True), seed=1, **kw)


def _product(P, T, sizes, seed, max_batch):
    images = ragged_ref.image_set(sizes, seed)
    oracle = ragged_ref.build_oracle(seed, P, T, ragged_ref.calib_patches(images, P))
    product = ja.GPT(model_config(patch_size=P, block_size=T, image_processor="yolox-nano", detector_conf_threshold=THR,
                                  max_det_per_patch=512),
                     max_batch=max_batch)
    product.load_state_dict(oracle.state_dict())
    product.eval()
    return product, images


def _as(img_u8, dtype):
    return img_u8.to(DEV) if dtype == torch.uint8 else img_u8.to(DEV).float().div(255)


def _own_env(img_u8, boxes, P, T, stop, dtype, engine=None):
    """The loop's env: the image padded on its own, B = 1."""
    x = _as(ragged_ref.pad_own(img_u8, P), dtype).unsqueeze(0).contiguous()
    return ja.NeedleGeneralEnv(x, boxes.reshape(1, -1, 4), P, T, 1, stop, engine=engine, uint8_images=dtype == torch.uint8)


# ---- 1. env walks -----------------------------------------------------------------------------------------------------
GRIDS = [(1, 2), (2, 3), (3, 2), (4, 5), (5, 4), (3, 3)]
ROTS = [0, 90, 180, 270, 90, 0]
# LEFT 0, RIGHT 1, UP 2, DOWN 3, UP_LEFT 4, UP_RIGHT 5, DOWN_LEFT 6, DOWN_RIGHT 7 from (0, 0): against the left and the
# top border, five steps right and six down (past the right and the bottom border of every grid), diagonals in the corner,
# back across to the left border and up again
WALK = [0, 2, 4, 1, 1, 1, 1, 1, 5, 3, 3, 3, 3, 3, 3, 7, 1, 6, 0, 0, 0, 0, 0, 6, 4, 2, 2, 2, 2, 2, 5]


def _walk_views(dtype, P=64):
    g = torch.Generator().manual_seed(3)
    srcs, boxes = [], []
    for i, ((gh, gw), rot) in enumerate(zip(GRIDS, ROTS)):
        hr, wr = gh * P - (7 * i) % P, gw * P - (11 * i + 5) % P          # the rotated image: inside its grid, not a multiple of P
        hs, ws = (wr, hr) if rot in (90, 270) else (hr, wr)
        img = torch.randint(0, 256, (3, hs, ws), generator=g, dtype=torch.uint8)
        srcs.append(_as(img, dtype).contiguous())
        # one box inside the image, one that sticks out of it to the right and below (clipped to gh*P x gw*P by its own
        # env, whereas the canvas would give it more patches)
        boxes.append([[wr // 3, hr // 3, wr // 3 + 9, hr // 3 + 9], [wr - 20, hr - 20, wr + 3 * P, hr + 3 * P]])
    views = ImageViews(srcs, rot=ROTS, patch_size=P)
    return views, torch.tensor(boxes, dtype=torch.long)


@pytest.mark.parametrize("dtype,stop", [(torch.float32, False), (torch.uint8, True)])
def test_ragged_env_walks_like_six_envs_of_one_image(dtype, stop):
    P, T = 64, len(WALK) + 1                            # ... and STOP as the last action
    views, boxes = _walk_views(dtype, P)
    assert views.canvas == (5 * P, 5 * P)
    ext = views.grid_extents(P)
    assert ext.tolist() == [list(g) for g in GRIDS]
    env = ja.NeedleGeneralEnv(None, boxes, P, T, 1, stop, views=views, clamp_to_image=True)
    canvas = views.materialize()
    own = [ja.NeedleGeneralEnv(canvas[i:i + 1, :, :gh * P, :gw * P].contiguous(), boxes[i:i + 1], P, T, 1, stop,
                               uint8_images=dtype == torch.uint8) for i, (gh, gw) in enumerate(GRIDS)]
    start = torch.zeros((len(GRIDS), 2), dtype=torch.long)
    pb, _ = env.reset(start)
    po = [e.reset(start[:1])[0] for e in own]

    def compare(step):
        pos = env.positions.cpu()
        assert bool((pos >= 0).all()) and bool((pos < ext.long()).all()), f"step {step}: an agent left its image: {pos.tolist()}"
        for i, (gh, gw) in enumerate(GRIDS):
            assert torch.equal(pos[i:i + 1], own[i].positions.cpu()), (step, i)
            assert torch.equal(env.visited_patches[i, :gh, :gw], own[i].visited_patches[0]), (step, i)
            assert torch.equal(env.bbox_masks[i, :gh, :gw], own[i].bbox_masks[0]), (step, i)
            assert torch.equal(env.prop_patches_found[i:i + 1], own[i].prop_patches_found), (step, i)
            assert torch.equal(env.terminated[i:i + 1], own[i].terminated), (step, i)
        outside = torch.ones_like(env.visited_patches)
        for i, (gh, gw) in enumerate(GRIDS):
            outside[i, :gh, :gw] = False
        assert not bool((env.visited_patches & outside).any()) and not bool((env.bbox_masks & outside).any())

    compare(-1)
    for i in range(len(GRIDS)):
        assert torch.equal(pb[i:i + 1], po[i])
    for t, a in enumerate(WALK + [8]):
        act = torch.full((len(GRIDS),), a, dtype=torch.long)
        pb, rb, tb, ub, _ = env.step(act)
        for i, e in enumerate(own):
            p1, r1, t1, u1, _ = e.step(act[:1])
            assert torch.equal(rb[i:i + 1], r1) and torch.equal(tb[i:i + 1], t1) and torch.equal(ub[i:i + 1], u1), (t, i)
            assert torch.equal(pb[i:i + 1], p1), (t, i)
        compare(t)
    # every border was reached: each agent has stood in all four corners' rows / columns of its own grid
    v = env.visited_patches
    for i, (gh, gw) in enumerate(GRIDS):
        assert bool(v[i, 0, :gw].any()) and bool(v[i, gh - 1, :gw].any()) and bool(v[i, :gh, 0].any()) and bool(v[i, :gh, gw - 1].any())


def test_ragged_random_reset_stays_inside_and_covers_the_small_image():
    P = 64
    views, boxes = _walk_views(torch.uint8, P)
    env = ja.NeedleGeneralEnv(None, boxes, P, 4, 1, False, views=views, clamp_to_image=True)
    ext = views.grid_extents(P).long()
    seen = set()
    for seed in range(256):
        _, info = env.reset(seed=seed)
        pos = info["positions"].cpu()
        assert bool((pos >= 0).all()) and bool((pos < ext).all()), (seed, pos.tolist())
        seen.add(tuple(pos[0].tolist()))
        assert bool(env.visited_patches.sum(dim=(1, 2)).eq(1).all())
    assert seen == {(0, 0), (0, 1)}


# ---- 5. rejections ----------------------------------------------------------------------------------------------------
def _init_ragged(engine, views, extents, boxes, P, T=4):
    ext = torch.tensor(extents, dtype=torch.int32).contiguous()
    bb = boxes.to(DEV).contiguous()
    check(engine.lib.jn_env_init_ragged(engine.handle, views.table_host(), C.cast(ext.data_ptr(), C.POINTER(C.c_int32)), ptr(bb),
                                        len(views), views.canvas[0], views.canvas[1], bb.shape[1], T, 0,
                                        _lib.current_stream(torch.device(DEV))), "jn_env_init_ragged")
    torch.cuda.synchronize()


def test_env_init_ragged_rejects_bad_extents_and_plain_envs_are_unchanged_afterwards():
    P = 64
    srcs = [torch.zeros((3, 2 * P, 3 * P), dtype=torch.uint8, device=DEV), torch.zeros((3, P, P), dtype=torch.uint8, device=DEV)]
    views = ImageViews(srcs, patch_size=P)
    boxes = torch.tensor([[[0, 0, 5, 5]], [[0, 0, 5, 5]]], dtype=torch.long)
    engine = Engine(bare_env_config(P, 2, 0, 8))
    good = [[2, 3], [1, 1]]
    _init_ragged(engine, views, good, boxes, P)
    p = C.c_void_p()
    check(engine.lib.jn_env_state(engine.handle, 5, C.byref(p)), "jn_env_state")
    assert p.value
    for bad in ([[2, 3], [0, 1]], [[2, 3], [1, 0]], [[3, 3], [1, 1]], [[2, 4], [1, 1]], [[1, 3], [1, 1]], [[2, 2], [1, 1]]):
        with pytest.raises(JnError):
            _init_ragged(engine, views, bad, boxes, P)
    with pytest.raises(JnError):                       # a translated view
        _init_ragged(engine, ImageViews(srcs, tx=[0, 4], patch_size=P), good, boxes, P)
    with pytest.raises(JnError):
        _init_ragged(engine, ImageViews(srcs, ty=[-3, 0], patch_size=P), good, boxes, P)
    with pytest.raises(AssertionError):
        ImageViews(srcs, tx=[0, 4], patch_size=P).grid_extents(P)
    # an ordinary view env on the same engine: extents cleared, the agent of the small image walks the canvas
    env = ja.NeedleGeneralEnv(None, boxes, P, 8, 1, False, engine=engine, views=views)
    check(engine.lib.jn_env_state(engine.handle, 5, C.byref(p)), "jn_env_state")
    assert not p.value
    env.reset(torch.zeros((2, 2), dtype=torch.long))
    for a in (1, 1, 1, 3, 3):
        env.step(torch.full((2,), a, dtype=torch.long))
    assert env.positions.cpu().tolist() == [[1, 2], [1, 2]]
    # ... and clamped again
    env = ja.NeedleGeneralEnv(None, boxes, P, 8, 1, False, engine=engine, views=views, clamp_to_image=True)
    env.reset(torch.zeros((2, 2), dtype=torch.long))
    for a in (1, 1, 1, 3, 3):
        env.step(torch.full((2,), a, dtype=torch.long))
    assert env.positions.cpu().tolist() == [[1, 2], [0, 0]]


# ---- 3. box assembly --------------------------------------------------------------------------------------------------
def _synthetic_rollout(B, T, S, K, seed):
    g = torch.Generator().manual_seed(seed)
    boxes = (torch.rand((B, T + 1, K, 7), generator=g) * 64).to(DEV)
    counts = torch.randint(0, K + 1, (B, T + 1), generator=g).to(torch.int32)
    counts[0] = 0                                      # an image with no detection at all
    counts[1, 2] = K                                   # K boxes in one patch
    counts[2, :] = K
    counts[3, 0] = 2
    masks = torch.ones((B, T + 1), dtype=torch.bool)
    masks[1, 4:] = False                               # a masked tail
    masks[3, 1:] = False
    pos = torch.randint(0, 9, (B, T + 1, 2), generator=g)
    counts, masks, pos = counts.to(DEV), masks.to(DEV), pos.to(DEV)
    cnt = counts.tolist()
    lists = [[boxes[b, t, :cnt[b][t]].clone() if cnt[b][t] > 0 else None for t in range(S + 1)] for b in range(B)]
    return {"det_boxes": boxes[:, :S + 1], "det_counts": counts[:, :S + 1], "positions": pos[:, :S + 1],
            "masks": masks[:, :S + 1], "bboxes": lists}


def _assert_same_assembly(ro, P):
    want = detection.patch_bboxes2full_image(ro["bboxes"], ro["positions"][:, :, [1, 0]] * P, ro["masks"])
    got = detection.rollout_boxes_to_image(ro, P)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert torch.equal(g, w)
    return want


@pytest.mark.parametrize("B,T,S,K", [(4, 7, 5, 6), (4, 7, 7, 6), (5, 300, 290, 3), (4, 3, 3, 64)])
def test_box_assembly_equals_the_python_loop_on_synthetic_rollouts(B, T, S, K):
    ro = _synthetic_rollout(B, T, S, K, seed=B + T)
    want = _assert_same_assembly(ro, 64)
    assert want[0] is None and want[2].shape[0] == (S + 1) * K and want[3].shape[0] == int(ro["det_counts"][3, 0])
    _assert_same_assembly({k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in ro.items()}, 448)
    # the copying route: counts of another integer type, and boxes whose image stride is not the counts'
    _assert_same_assembly(dict(ro, det_counts=ro["det_counts"].long()), 64)
    wide = torch.zeros((B, T + 3, K, 7), device=DEV)
    wide[:, :S + 1] = ro["det_boxes"]
    _assert_same_assembly(dict(ro, det_boxes=wide[:, :S + 1]), 64)
    one = {k: (v[1:2] if torch.is_tensor(v) else v[1:2]) for k, v in ro.items()}
    _assert_same_assembly(one, 64)


# ---- 2. greedy rollouts with detection --------------------------------------------------------------------------------
def _candidate_scores(product, patches):
    eng = product.engine()
    N, P = patches.shape[0], patches.shape[-1]
    A = sum((P // s) ** 2 for s in (8, 16, 32))
    raw = torch.empty((N, A, 6), device=DEV)
    boxes = torch.zeros((N, eng.cfg.max_det_per_patch, 7), device=DEV)
    counts = torch.zeros(N, device=DEV, dtype=torch.int32)
    check(eng.lib.jn_detect(eng.handle, ptr(patches.contiguous()), N, ptr(boxes), ptr(counts), ptr(raw),
                            _lib.current_stream(torch.device(DEV))), "jn_detect")
    torch.cuda.synchronize()
    return raw[..., 4] * raw[..., 5]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
@pytest.mark.parametrize("P,T,sizes,seed", [(64, 6, SIZES_64, SEED_64), (448, 3, SIZES_448, SEED_448)], ids=["p64", "p448"])
def test_batched_greedy_rollout_with_detection_equals_the_per_image_loop(P, T, sizes, seed, dtype):
    B = len(sizes)
    product, images = _product(P, T, sizes, seed, max_batch=max(B, T + 1))
    tr = ja.ReinforceTrainer(_cfg(T=T), product)
    start = torch.zeros((B, 2), dtype=torch.long)
    loop = []
    for i, (img, boxes) in enumerate(images):
        ro = tr.rollout(_own_env(img, boxes, P, T, True, dtype, engine=product.engine()), do_detection=True,
                        sample_actions=False, start_positions=start[:1])
        top = ro["logits"][0].topk(2, dim=-1).values
        gap = float((top[:, 0] - top[:, 1]).min())
        near = float((_candidate_scores(product, ro["patches"][0]) - THR).abs().min())
        print(f"image {i}: steps {ro['rewards'].shape[1]} logit gap {gap:.3e} score distance {near:.3e} boxes {int(ro['det_counts'].sum())}")
        assert gap >= LOGIT_GAP, f"precondition: image {i} has a top-2 logit gap of {gap}"
        assert near >= SCORE_GAP, f"precondition: image {i} has a candidate score {near} from the threshold"
        loop.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in ro.items()})
    env = ragged.image_env(tr, [_as(im, dtype) for im, _ in images], [b for _, b in images])
    rb = tr.rollout(env, do_detection=True, sample_actions=False, start_positions=start, bbox_lists=False)
    assert rb["bboxes"] == [[] for _ in range(B)]
    steps = ragged.own_steps(rb)
    full = detection.rollout_boxes_to_image(rb, P)
    n_boxes = 0
    for i, ro in enumerate(loop):
        S = ro["rewards"].shape[1]
        assert steps[i] == S, (i, steps[i], S)
        mine = ragged.slice_rollout(rb, i, S)
        for k in ("positions", "actions", "masks", "det_counts", "logit_masks"):
            assert torch.equal(mine[k], ro[k]), (i, k)
        for k in ("rewards", "returns"):
            assert torch.equal(mine[k], ro[k]), (i, k)
        err = float((mine["logits"] - ro["logits"]).abs().max())
        want = detection.patch_bboxes2full_image(ro["bboxes"], ro["positions"][:, :, [1, 0]] * P, ro["masks"])[0]
        assert (want is None) == (full[i] is None), i
        berr = 0.0
        if want is not None:
            assert want.shape == full[i].shape, i
            berr = float((want[:, :4] - full[i][:, :4]).abs().max())
            assert torch.equal(want[:, 6], full[i][:, 6]) and float((want[:, 4:6] - full[i][:, 4:6]).abs().max()) <= 1e-5
            n_boxes += want.shape[0]
        print(f"image {i}: logits differ by {err:.3e}, boxes by {berr:.3e} px")
        assert err <= LOGIT_BAR and berr <= BOX_BAR, (i, err, berr)
    assert n_boxes > 0, "no box anywhere: the comparison of the detections is empty"
    # the device assembly on a rollout that also carries the Python lists
    _assert_same_assembly(loop[-1], P)
    _assert_same_assembly(tr.rollout(env, do_detection=True, sample_actions=False, start_positions=start), P)


def test_sampled_ragged_rollout_stays_inside_the_extents():
    P, T = 64, 6
    product, images = _product(P, T, SIZES_64, SEED_64, max_batch=len(SIZES_64))
    tr = ja.ReinforceTrainer(_cfg(T=T, stop=False), product)
    env = ragged.image_env(tr, [im for im, _ in images], [b for _, b in images])
    ext = env.grid_extents.long().unsqueeze(1)
    for _ in range(8):
        pos = tr.rollout(env, sample_actions=True, stop_early=False, keep_patches=False)["positions"].cpu()
        assert bool((pos >= 0).all()) and bool((pos < ext).all())


# ---- 4. infer_images and eval_on_images -------------------------------------------------------------------------------
def _close(a, b, rel=1e-5):
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-30) or a == b


def _assert_same_inference(a, b, n):
    assert list(a) == list(b) and list(a["metrics"]) == list(b["metrics"])
    assert a["steps"] == b["steps"]
    n_boxes = 0
    for i in range(n):
        assert torch.equal(a["positions"][i], b["positions"][i]), i
        assert (a["boxes"][i] is None) == (b["boxes"][i] is None), i
        if b["boxes"][i] is not None:
            assert a["boxes"][i].shape == b["boxes"][i].shape
            err = float((a["boxes"][i] - b["boxes"][i]).abs().max())
            print(f"image {i}: boxes differ by {err:.3e} px")
            assert err <= BOX_BAR, (i, err)
            n_boxes += len(b["boxes"][i])
    for k, v in b["metrics"].items():
        print(k, v, a["metrics"][k])
        assert _close(v, a["metrics"][k]), (k, v, a["metrics"][k])
    return n_boxes


def test_infer_images_batched_matches_the_loop():
    """Seven images of four sizes, one without targets, random starts: ``infer_images(batch_size=4)`` against the loop.

    The loop scales a uint8 image on the device (``x.float() / 255``, infer.py of this package, untouched here), where
    torch multiplies by the rounded reciprocal of 255: for some bytes that is one ulp off the correctly rounded b / 255
    that ToTensor computes on the CPU and that the engine's byte readers reproduce (printed below).  The comparison with
    the loop is therefore made on the ToTensor values handed over as fp32 images, so that both calls see the same pixels;
    the byte path is then held to the same bars against the batched fp32 run, in a mixed list that also splits the chunks
    by element type."""
    P, T = 64, 6
    product, images = _product(P, T, SIZES_64, SEED_64, max_batch=8)
    n = len(images)
    as_f32 = [im.float().div(255) for im, _ in images]                                 # ToTensor's values (CPU division)
    mixed = [as_f32[i] if i in (2, 5) else im for i, (im, _) in enumerate(images)]     # bytes stay bytes
    off = max(float((im.to(DEV).float() / 255 - f.to(DEV)).abs().max()) for (im, _), f in zip(images, as_f32))
    print(f"device-side x.float() / 255 against the correctly rounded b / 255: max difference {off:.3e}")
    targets = [None if i == 3 else b for i, (_, b) in enumerate(images)]

    def run(imgs, bs):
        tr = ja.ReinforceTrainer(_cfg(T=T, detection_enabled=True, patch_size=P), product)
        res = ja.infer_images(tr, imgs, targets, sample_actions=False, do_detection=True, batch_size=bs)
        assert tr._rollouts == n
        return res, tr.last_return_values
    (loop, lv), (bat, bv), (bat_mixed, mv) = run(as_f32, None), run(as_f32, 4), run(mixed, 4)
    assert _assert_same_inference(bat, loop, n) > 0
    assert _assert_same_inference(bat_mixed, bat, n) > 0
    # the reward-norm window: one entry per image with targets, in input order, also where the element types split a group
    assert len(lv) == len(bv) == len(mv) == n - 1 and len({tuple(v.shape) for v in lv}) > 0
    for a, b, c in zip(lv, bv, mv):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert all(d > 0 for d in bat["duration_ms"]) and len(bat["duration_ms"]) == n
    assert len({tuple(p[0].tolist()) for p in loop["positions"]}) > 1, "every image starts in the same cell: the random reset is not exercised"


@pytest.mark.parametrize("stop", [True, False])
def test_eval_on_images_matches_eval_on_batch_per_image(stop):
    P, T = 64, 6
    product, images = _product(P, T, SIZES_64, SEED_64, max_batch=8)
    imgs = [im.float().div(255) if i in (2, 5) else im for i, (im, _) in enumerate(images)]
    boxes = [b for _, b in images]
    cfg = dict(T=T, stop=stop, detection_enabled=True, merge_bboxes=True)
    tr_loop, tr_bat = ja.ReinforceTrainer(_cfg(**cfg), product), ja.ReinforceTrainer(_cfg(**cfg), product)
    want = []
    for im, b in zip(imgs, boxes):
        dtype = im.dtype
        x = ragged_ref.pad_own(im, P).unsqueeze(0).to(DEV).contiguous()
        env = ja.NeedleGeneralEnv(x, b.reshape(1, -1, 4), P, T, 1, stop, engine=product.engine(), uint8_images=dtype == torch.uint8)
        want.append(tr_loop.eval_on_batch(env))
    got = tr_bat.eval_on_images(imgs, boxes, batch_size=4)
    assert list(got) == list(want[0])
    for k in got:
        assert len(got[k]) == len(imgs)
        for i, w in enumerate(want):
            print(k, i, float(w[k]), got[k][i])
            assert _close(float(w[k]), got[k][i]), (k, i, float(w[k]), got[k][i])
    assert tr_bat._rollouts == tr_loop._rollouts == len(imgs)
    assert len(tr_bat.last_return_values) == len(tr_loop.last_return_values) == len(imgs)
    for a, b in zip(tr_bat.last_return_values, tr_loop.last_return_values):
        assert torch.equal(a, b)
