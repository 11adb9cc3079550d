"""Image views (``ImageViews``, jn_env_init_views, jn_gather_patches_views): rotation by a multiple of 90 degrees,
whole-pixel translation and padding to one canvas applied inside the patch reads.  Everything computed through views
equals what the same entry point computes on ``views.materialize()`` — the augmented canvas written out with torch ops —
bit for bit where the path is deterministic and within the project's fixed bars where it is not (train-mode BatchNorm
sums on fp64 atomics)."""
import random

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd.trajectory import gather_indexed
from jolineedle_amd.views import ImageViews
from tests.helpers import make_pair, synth_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# "same values, different read path": the loss to 1e-6 relative and every gradient tensor to 1e-5 relative L2; two runs
# on the materialised canvas are held to the same bars as the control.
LOSS_BAR, GRAD_BAR = 1e-6, 1e-5

ROTS = (0, 90, 180, 270)


def _cfg(**kw):
    return ja.CfgNode(max_seq_len=kw.pop("T", 6), entropy_weight=0.01, stop_enabled=kw.pop("stop", True),
                      reward_norm=True, seed=1, **kw)


def _image(Hs, Ws, dtype, seed, offset=0):
    """One stored image [3, Hs, Ws]; offset = 1 puts it one element past an aligned address (a storage-offset view),
    which forces the scalar routes: a byte image then sits at an odd address, an fp32 image 4 bytes past 16."""
    n = 3 * Hs * Ws
    if dtype == torch.uint8:
        vals = ((torch.arange(n, device=DEV, dtype=torch.int64) * 37 + 11 + seed) % 256).to(torch.uint8)
    else:
        vals = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    buf = torch.empty(n + 4 + offset, dtype=dtype, device=DEV)
    buf[offset:offset + n] = vals
    img = buf[offset:offset + n].view(3, Hs, Ws)
    assert img.is_contiguous() and (img.data_ptr() // img.element_size()) % 4 == offset
    return img


def _all_cells(views, P):
    Gh, Gw = views.canvas[0] // P, views.canvas[1] // P
    cells = [(i, y, x) for i in range(len(views)) for y in range(Gh) for x in range(Gw)] + [(-1, 0, 0)]
    return cells, torch.tensor(cells, dtype=torch.int64)


def _check_gather(views, P):
    canvas = views.materialize()
    assert canvas.dtype == views.dtype
    cells, c = _all_cells(views, P)
    want = torch.stack([canvas[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P] for i, y, x in cells[:-1]])
    got = views.gather(c[:, 0], c[:, 1:], P)
    assert got.dtype == torch.float32
    want_f = want.cpu().float().div(255).to(DEV) if views.uint8 else want
    assert torch.equal(got[:-1], want_f) and int(got[-1].abs().sum()) == 0
    assert torch.equal(gather_indexed(None, c[:, 0], c[:, 1:], P, views=views), got)
    if views.uint8:
        raw = views.gather(c[:, 0], c[:, 1:], P, out_uint8=True)
        assert raw.dtype == torch.uint8 and torch.equal(raw[:-1], want) and int(raw[-1].sum()) == 0
    return int((want != 0).sum())


# translations of both signs, multiples of 4 (the vector route stays) and not, and ones that push part of the image out
SHIFTS = [(0, 0), (4, 8), (-8, -4), (3, -5), (-7, 2), (1, 1), (40, -50), (-100, 90)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
@pytest.mark.parametrize("P,offset", [(64, 0), (30, 1)], ids=["P64-vector", "P30-odd-scalar"])
def test_view_gathers_equal_slices_of_the_materialised_canvas(dtype, P, offset):
    # non-square stored images of different sizes on one canvas
    sizes = [(2 * P, 3 * P), (3 * P, 2 * P), (3 * P, 3 * P), (P, 2 * P)]
    srcs = [_image(h, w, dtype, 5 + i, offset) for i, (h, w) in enumerate(sizes)]
    nonzero = 0
    for rot in ROTS:
        for ty, tx in SHIFTS:
            views = ImageViews(srcs, [rot] * 4, [ty, -ty, ty, tx], [tx, tx, -tx, ty], canvas=(3 * P, 3 * P))
            nonzero += _check_gather(views, P)
    # all four rotations in one table, the default canvas
    views = ImageViews(srcs, [0, 90, 180, 270], [3, -4, 8, 0], [-8, 5, 0, 12], patch_size=P)
    assert views.canvas == (3 * P, 3 * P)
    nonzero += _check_gather(views, P)
    assert nonzero > 1000
    # a stacked batch as well (what the trainers pass)
    stacked = torch.stack([_image(2 * P, 3 * P, dtype, 40 + i) for i in range(3)])
    _check_gather(ImageViews(stacked, [270, 0, 90], [0, 4, -3], [8, 0, 2], patch_size=P), P)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
def test_identity_view_equals_the_existing_gather(dtype):
    P, B, G = 64, 3, 3
    images = torch.stack([_image(G * P, G * P, dtype, 60 + i) for i in range(B)])
    views = ImageViews(images, patch_size=P)
    cells, c = _all_cells(views, P)
    assert torch.equal(views.gather(c[:, 0], c[:, 1:], P), gather_indexed(images, c[:, 0], c[:, 1:], P))


def _env_pair(views, bboxes, P, T, engine=None):
    tb = views.transform_bboxes(bboxes)
    env_v = ja.NeedleGeneralEnv(None, tb, P, T, 1, True, views=views, engine=engine)
    env_m = ja.NeedleGeneralEnv(views.materialize(), tb, P, T, 1, True, uint8_images=views.uint8, engine=engine)
    return env_v, env_m


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
def test_env_patches_rollout_stack_and_detection_batch(dtype):
    P, T, B, G = 64, 3, 4, 3
    srcs = [_image(h * P, w * P, dtype, 70 + i) for i, (h, w) in enumerate([(3, 3), (2, 3), (3, 2), (3, 3)])]
    views = ImageViews(srcs, [90, 0, 270, 180], [5, -9, 0, 16], [-6, 4, 11, -20], patch_size=P)
    _, bboxes, start = synth_batch(B, 2, 2, P, seed=21)
    env_v, env_m = _env_pair(views, bboxes, P, T)
    assert (env_v.height, env_v.width) == views.canvas == (G * P, G * P)
    assert torch.equal(env_v.bbox_masks, env_m.bbox_masks)
    assert torch.equal(env_v.images, env_m.images)              # on demand: the materialised canvas
    for env in (env_v, env_m):
        env.reset(start)
    assert env_v.patches.dtype == torch.float32 and torch.equal(env_v.patches, env_m.patches)
    acts = torch.tensor([1, 3, 5, 7], device=DEV)
    env_v.step(acts); env_m.step(acts)
    assert torch.equal(env_v.patches, env_m.patches) and float(env_v.patches.abs().sum()) > 0
    product, _ = make_pair(5, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
    tr = ja.ReinforceTrainer(_cfg(T=T), product)
    with torch.no_grad():
        rm = tr.rollout(env_m, sample_actions=False, start_positions=start)
        rv = tr.rollout(env_v, sample_actions=False, start_positions=start)
    assert torch.equal(rv["positions"], rm["positions"]) and torch.equal(rv["patches"], rm["patches"])
    dv = env_v.get_detection_batch(2, generator=torch.Generator().manual_seed(4))
    dm = env_m.get_detection_batch(2, generator=torch.Generator().manual_seed(4))
    assert torch.equal(dv[0], dm[0]) and torch.equal(dv[1], dm[1])
    # the model's context was last in view mode: jn_env_init / jn_env_init_u8 put it back into plain mode
    canvas = views.materialize()
    plain = ja.NeedleGeneralEnv(canvas, views.transform_bboxes(bboxes), P, T, 1, True, uint8_images=views.uint8,
                                engine=product.engine())
    plain.reset(start)
    want = torch.stack([canvas[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P] for i, (y, x) in enumerate(start.tolist())])
    want = want.cpu().float().div(255).to(DEV) if views.uint8 else want
    assert torch.equal(plain.patches[:, 0], want)


def test_env_init_views_rejects_bad_tables():
    P, T = 64, 3
    img = _image(2 * P, 3 * P, torch.float32, 1)
    boxes = torch.zeros((1, 1, 4), dtype=torch.int64)

    def make(**kw):
        v = ImageViews([img], canvas=(3 * P, 3 * P))
        for k, val in kw.items():
            setattr(v.table_host()[0], k, val)
        return ja.NeedleGeneralEnv(None, boxes, P, T, 1, True, views=v)
    make()
    for bad in (dict(rot=45), dict(src=None), dict(Hs=4 * P), dict(Ws=4 * P)):
        with pytest.raises(ja._lib.JnError):
            make(**bad)
    v = ImageViews([img], [90], canvas=(3 * P, 3 * P))                  # 192 x 128 rotated: fits
    v.canvas = (3 * P, P)                                                # ... but not a canvas one patch wide
    with pytest.raises(ja._lib.JnError):
        ja.NeedleGeneralEnv(None, boxes, P, T, 1, True, views=v)
    v = ImageViews([img, img], canvas=(3 * P, 3 * P))
    v.table_host()[1].src_u8 = 1                                         # mixed element types
    with pytest.raises(ja._lib.JnError):
        ja.NeedleGeneralEnv(None, torch.zeros((2, 1, 4), dtype=torch.int64), P, T, 1, True, views=v)


@pytest.mark.parametrize("P,B,T,arch,dtype,ragged", [
    (64, 4, 5, dict(image_processor="yolox-nano", detector_conf_threshold=0.05), torch.uint8, True),     # the smoke shapes
    (448, 8, 3, dict(image_processor="yolox-nano"), torch.float32, False),
    (64, 4, 5, dict(image_processor="yolox-nano", gpt_backbone="yolox-nano", act_dtype="bf16",           # bf16 storage
                    detector_conf_threshold=0.05), torch.float32, False),
    (96, 4, 5, dict(with_detector=False, image_processor=None, gpt_backbone="yolox-s"), torch.uint8, False),   # dense stem
])
def test_view_eval_rollout_is_bit_identical(P, B, T, arch, dtype, ragged):
    G = 3
    product, _ = make_pair(5, patch_size=P, block_size=T, max_batch=B, **arch)
    shapes = [(G, G), (2, 3), (3, 2), (1, 2)] if ragged else [(G, G)] * B
    srcs = [_image(shapes[i % len(shapes)][0] * P, shapes[i % len(shapes)][1] * P, dtype, P + i) for i in range(B)]
    g = torch.Generator().manual_seed(P + B)
    rot = [ROTS[(i + P) % 4] for i in range(B)]
    ty = torch.randint(-P // 2, P // 2, (B,), generator=g).tolist()
    tx = torch.randint(-P // 2, P // 2, (B,), generator=g).tolist()
    views = ImageViews(srcs if ragged else torch.stack(srcs), rot, ty, tx, patch_size=P)
    assert views.canvas == (G * P, G * P)
    _, bboxes, _ = synth_batch(B, 1 if ragged else G, 1 if ragged else G, P, seed=23)
    start = torch.randint(0, G, (B, 2), generator=g)
    det = arch.get("with_detector", True)
    tr = ja.ReinforceTrainer(_cfg(T=T), product)
    out = []
    for env in _env_pair(views, bboxes, P, T):
        with torch.no_grad():
            r = tr.rollout(env, do_detection=det, sample_actions=False, start_positions=start, keep_patches=False)
        torch.cuda.synchronize()
        out.append(r)
    rv, rm = out
    for k in ("positions", "rewards", "masks", "actions", "logits", "final_emb"):
        assert torch.equal(rv[k], rm[k]), k
    if det:
        assert torch.equal(rv["det_counts"], rm["det_counts"])
        for bv, bm in zip(rv["bboxes"], rm["bboxes"]):
            for a, b in zip(bv, bm):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        print(f"detections compared: {int(rv['det_counts'].sum())}")


def _rel_l2(a, b):
    return float((a - b).norm() / a.norm())


def _check_training_pair(ref, got, tag):
    """({name: loss}, grads) of two runs against the fixed bars; returns the worst gradient error seen."""
    (la, ga), (lb, gb) = ref, got
    errs = {k: _rel_l2(a, gb[k]) for k, a in ga.items() if float(a.abs().max()) >= 1e-12}
    worst = max(errs, key=errs.get)
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print(f"{tag}: losses {la} vs {lb}; worst gradient rel L2 {top} over {len(errs)} tensors")
    for k in la:
        assert abs(la[k] - lb[k]) <= LOSS_BAR * abs(la[k]), (tag, k, la[k], lb[k])
    assert len(errs) > 100, (tag, len(errs))
    for k, e in errs.items():
        assert e <= GRAD_BAR, (tag, k, e)
    return errs[worst]


def test_view_training_iteration_matches_the_materialised_canvas():
    """REINFORCE iteration with forced actions and detector training at 448 px (train-mode BatchNorm): views over fp32
    and over uint8 sources against the env on the materialised canvas, and two such envs as the control."""
    P, T, B, G = 448, 3, 16, 3
    u8 = torch.randint(0, 256, (B, 3, G * P, G * P), device=DEV, dtype=torch.uint8,
                       generator=torch.Generator(device=DEV).manual_seed(29))
    f32 = u8.cpu().float().div(255).to(DEV)
    _, bboxes, start = synth_batch(B, G, G, 64, seed=31)
    bboxes = bboxes * (P // 64)
    g = torch.Generator().manual_seed(7)
    rot = [ROTS[i % 4] for i in range(B)]
    ty = torch.randint(-150, 150, (B,), generator=g).tolist()
    tx = torch.randint(-150, 150, (B,), generator=g).tolist()
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(6))
    vf, vu = ImageViews(f32, rot, ty, tx, patch_size=P), ImageViews(u8, rot, ty, tx, patch_size=P)
    tb = vf.transform_bboxes(bboxes)
    runs = []
    for kind in ("canvas", "canvas", "views fp32", "views uint8"):
        product, _ = make_pair(7, bn_seed=None, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
        cfg = _cfg(T=T, learning_rate=1e-3, gradient_accumulation=1)
        cfg.detection_enabled, cfg.yolo_lr = True, 2e-3
        tr = ja.ReinforceTrainer(cfg, product)
        if kind == "canvas":
            env = ja.NeedleGeneralEnv(vf.materialize(), tb, P, T, 1, True)
        else:
            env = ja.NeedleGeneralEnv(None, tb, P, T, 1, True, views=vf if kind == "views fp32" else vu)
        torch.manual_seed(13)                  # the detection batch's negative patches (torch.randperm): the same draws
        m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
        assert m["steps"] == T and "yolo_total_loss" in m
        runs.append(({k: float(m[k]) for k in ("loss", "yolo_total_loss")}, product.engine_grads()))
        del product, tr, env
        torch.cuda.empty_cache()
    _check_training_pair(runs[0], runs[1], "canvas vs canvas (control)")
    _check_training_pair(runs[0], runs[2], "canvas vs views fp32")
    _check_training_pair(runs[0], runs[3], "canvas vs views uint8")


def test_view_supervised_trajectories_and_iteration_match_the_materialised_canvas():
    P, T, B, G = 64, 6, 3, 4
    images = torch.rand((B, 3, G * P, G * P), device=DEV, generator=torch.Generator(device=DEV).manual_seed(33))
    _, bboxes, _ = synth_batch(B, G, G, P, seed=3)
    cid = torch.zeros(B, dtype=torch.long)
    traj, runs, views = {}, {}, None
    for tag in ("views", "canvas", "canvas again"):
        product, _ = make_pair(9, patch_size=P, block_size=T, image_processor="yolox-nano", gpt_backbone="yolox-nano",
                               max_batch=B * T)
        aug = tag == "views"
        cfg = ja.CfgNode(patch_size=P, max_seq_len=T, min_keypoints=0, max_keypoints=1, binomial_keypoints=False,
                         stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, yolo_lr=1e-3, gradient_accumulation=1,
                         detection_enabled=True, rotations=aug, translations=aug, seed=4)
        tr = ja.SupervisedTrainer(cfg, product)
        if aug:
            batch = {"image": images, "bboxes": bboxes, "class_id": cid}
        else:
            batch = {"image": views.materialize(), "bboxes": views.transform_bboxes(bboxes), "class_id": cid}
        random.seed(13)                        # ties of the teacher walks
        m = tr.train_iteration(batch, optimizer_step=False, seed=5)
        if aug:
            views = tr.last_views
            assert views is not None
            print(f"drawn views: rot {views.rot.tolist()} ty {views.ty.tolist()} tx {views.tx.tolist()}")
        else:
            assert tr.last_views is None
        traj[tag] = m["trajectories"]
        runs[tag] = ({k: float(m[k]) for k in ("loss", "yolo_total_loss")}, product.engine_grads())
        del product, tr
        torch.cuda.empty_cache()
    a, b = traj["canvas"], traj["views"]
    for k in ("patches", "patches_yolox", "current_actions", "next_actions", "positions", "masks", "bboxes_yolox",
              "local_bboxes"):
        assert torch.equal(a[k], b[k]), k
    _check_training_pair(runs["canvas"], runs["canvas again"], "supervised canvas vs canvas (control)")
    _check_training_pair(runs["canvas"], runs["views"], "supervised canvas vs views")


def test_trainers_apply_the_flags_and_draw_reproducibly(monkeypatch):
    P, T, B, G = 64, 3, 4, 3
    images, bboxes, _ = synth_batch(B, G, G, P, seed=41)
    batch = {"image": images.to(DEV), "bboxes": bboxes, "class_id": torch.zeros(B, dtype=torch.long)}
    drawn = []
    for _ in range(2):
        product, _ = make_pair(5, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B * T)
        cfg = _cfg(T=T, learning_rate=1e-3, gradient_accumulation=1, rotations=True, translations=True, patch_size=P,
                   min_keypoints=0, max_keypoints=1, stop_weight=1.0, detection_enabled=False)
        cfg.seed = 11
        tr = ja.ReinforceTrainer(cfg, product)
        og, oy = product.configure_optimizers(cfg)
        m = tr.training_step(batch, og, oy)
        assert torch.isfinite(m["loss"])
        v = tr.last_views
        assert v is not None and tr.last_env.views is v
        ref = ja.NeedleGeneralEnv(v.materialize(), v.transform_bboxes(bboxes), P, T, 1, True)
        assert torch.equal(tr.last_env.bbox_masks, ref.bbox_masks)
        st = ja.SupervisedTrainer(cfg, product)
        random.seed(3)
        ms = st.training_step(batch, og, oy, seed=2)
        assert torch.isfinite(ms["loss"]) and st.last_views is not None
        drawn.append([(x.rot.tolist(), x.ty.tolist(), x.tx.tolist()) for x in (v, st.last_views)])
        del product, tr, st
        torch.cuda.empty_cache()
    assert drawn[0] == drawn[1]
    assert any(any(part) for part in drawn[0][0])            # something was drawn

    # both flags false: no ImageViews is ever constructed
    from jolineedle_amd import views as views_mod

    class Boom:
        def __init__(self, *a, **k):
            raise AssertionError("ImageViews constructed without the augmentation flags")
    monkeypatch.setattr(views_mod, "ImageViews", Boom)
    product, _ = make_pair(5, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B * T)
    cfg = _cfg(T=T, learning_rate=1e-3, gradient_accumulation=1, rotations=False, translations=False, patch_size=P,
               min_keypoints=0, max_keypoints=1, stop_weight=1.0, detection_enabled=False)
    tr, st = ja.ReinforceTrainer(cfg, product), ja.SupervisedTrainer(cfg, product)
    og, oy = product.configure_optimizers(cfg)
    assert torch.isfinite(tr.training_step(batch, og, oy)["loss"]) and tr.last_views is None
    random.seed(3)
    assert torch.isfinite(st.training_step(batch, og, oy, seed=2)["loss"]) and st.last_views is None


def test_view_env_allocates_no_canvas():
    """Creating a view env takes less than 1 MB of torch memory (the table) and never a canvas; over one training
    iteration the device memory that views add stays within the staging stack (T + 1) B 3 P^2 elements of the source type
    plus 1 MB.  (At the headline sizes: 0.81 GB for uint8 sources and 3.2 GB for fp32, against 3.85 GB and 15.4 GB for
    the materialised batch.)

    How the second bound is measured: a fresh context runs one training iteration and the fall of the device's free
    memory (torch's own pool taken out) is what the context allocated; a view-mode context minus a plain-mode context on
    the materialised canvas is what views add.  The first contexts of a process also pay for what the runtime keeps when
    a context is freed (measured in a fresh process: 1 358 954 496, then 1 337 982 976 bytes for the first two view
    contexts, 1 327 497 216 for every later one; 1 317 011 456 for every plain one), so one context of each kind is
    created and dropped first, then the two kinds alternate, three contexts each.  In a process with a history (this
    file inside the whole suite) a context now and then finds a 2 MiB granule that an earlier one left in the runtime's
    pool of small allocations and reports that much LESS, whichever its kind (measured: plain 1 314 914 304 and
    1 317 011 456, views 1 327 497 216 and 1 325 400 064 in one run): such a discount only ever lowers a figure, so what
    a kind costs is the LARGEST figure of its repeats, and the largest of the view contexts is held against the largest
    of the plain ones.  Undiscounted, the difference is the staging stack alone: 9 633 792 bytes, handed out as 10 MiB."""
    P, T, B, G = 448, 3, 4, 3
    u8 = torch.randint(0, 256, (B, 3, G * P, G * P), device=DEV, dtype=torch.uint8,
                       generator=torch.Generator(device=DEV).manual_seed(35))
    _, bboxes, start = synth_batch(B, G, G, 64, seed=37)
    bboxes = bboxes * (P // 64)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(6))
    views = ImageViews(u8, [90, 0, 270, 180], [30, -7, 0, 100], [-12, 64, 5, 0], patch_size=P)
    tb = views.transform_bboxes(bboxes)

    def iteration(make_env):
        """(torch bytes the env took, device bytes the iteration took beyond torch's own) of a fresh context"""
        product, _ = make_pair(5, bn_seed=None, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
        tr = ja.ReinforceTrainer(_cfg(T=T, learning_rate=1e-3, gradient_accumulation=1), product)
        eng = product.engine()
        product.sync_weights()
        torch.cuda.synchronize()
        t0 = torch.cuda.memory_allocated()
        env = make_env(eng)
        torch.cuda.synchronize()
        env_bytes = torch.cuda.memory_allocated() - t0
        free0, r0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
        tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
        torch.cuda.synchronize()
        free1, r1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
        ctx_bytes = (free0 - free1) - (r1 - r0)             # what the context allocated, torch's pool taken out
        del product, tr, env
        torch.cuda.empty_cache()
        return env_bytes, ctx_bytes

    canvas = views.materialize()
    make = {"views": lambda eng: ja.NeedleGeneralEnv(None, tb, P, T, 1, True, views=views, engine=eng),
            "plain": lambda eng: ja.NeedleGeneralEnv(canvas, tb, P, T, 1, True, uint8_images=True, engine=eng)}
    for kind in ("views", "plain"):                      # loads the kernels, lets the runtime's own pools settle
        iteration(make[kind])
    env_b, ctx_b = {"views": [], "plain": []}, {"views": [], "plain": []}
    for kind in ("plain", "views") * 3:
        e, c = iteration(make[kind])
        env_b[kind].append(e), ctx_b[kind].append(c)
    stage = (T + 1) * B * 3 * P * P * u8.element_size()
    print(f"env bytes {env_b}; context growth {ctx_b}; staging bound {stage}")
    assert max(env_b["views"]) < (1 << 20), env_b
    assert max(ctx_b["views"]) - max(ctx_b["plain"]) <= stage + (1 << 20), (ctx_b, stage)
    assert stage < canvas.numel()
