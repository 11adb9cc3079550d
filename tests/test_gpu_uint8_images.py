"""uint8 images read in place (NeedleGeneralEnv(..., uint8_images=True), jn_env_init_u8, jn_gather_patches*_u8): every
result computed from the bytes equals the result computed from ``u8.cpu().float().div(255)`` as an fp32 image, bit for
bit where the fp32 path is deterministic and within fixed bars where it is not (train-mode BatchNorm sums on fp64
atomics)."""
import random

import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd.trajectory import gather_indexed
from tests.helpers import make_pair, synth_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# The training bars (item 3 of the feature): the loss to 1e-6 relative and every gradient tensor to 1e-5 relative L2.
# Two fp32 runs of the same iteration are held to the same bars as the control.
LOSS_BAR, GRAD_BAR = 1e-6, 1e-5


def _cfg(**kw):
    return ja.CfgNode(max_seq_len=kw.pop("T", 6), entropy_weight=0.01, stop_enabled=kw.pop("stop", True),
                      reward_norm=True, seed=1, **kw)


def _as_float(u8):
    """The fp32 image the bytes stand for: ToTensor's u8.float().div(255), computed on the CPU."""
    return u8.cpu().float().div(255).to(DEV)


def _cycling_bytes(B, H, W, offset=0):
    """Pixels that cycle through all 256 byte values (a stride prime to 256 mixes rows and channels); offset = 1 puts the
    data one byte past an aligned address (a storage-offset view), which forces the scalar routes."""
    n = B * 3 * H * W
    vals = ((torch.arange(n, device=DEV, dtype=torch.int64) * 37 + 11) % 256).to(torch.uint8)
    buf = torch.empty(n + offset, dtype=torch.uint8, device=DEV)
    buf[offset:] = vals
    img = buf[offset:].view(B, 3, H, W)
    assert img.is_contiguous() and img.data_ptr() % 4 == offset
    return img


def _random_bytes(B, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), device=DEV, generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("offset", [0, 1])
def test_uint8_gathers_equal_the_gathers_of_the_converted_image(offset):
    P, T, B, G = 64, 3, 4, 3
    u8 = _cycling_bytes(B, G * P, G * P, offset)
    f32 = _as_float(u8)
    _, bboxes, start = synth_batch(B, G, G, P, seed=21)
    product, _ = make_pair(5, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
    env_u = ja.NeedleGeneralEnv(u8, bboxes, P, T, 1, True, uint8_images=True)
    env_f = ja.NeedleGeneralEnv(f32, bboxes, P, T, 1, True)
    assert env_u.images.dtype == torch.uint8 and env_u.images.data_ptr() == u8.data_ptr()
    # env.patches after reset and after a step (both routes of jn_env_patches)
    for env in (env_u, env_f):
        env.reset(start)
    pu, pf = env_u.patches, env_f.patches
    assert pu.dtype == torch.float32 and torch.equal(pu, pf)
    assert len(torch.unique(pu)) == 256                        # every byte value went through the conversion
    acts = torch.tensor([1, 3, 5, 7][:B], device=DEV)
    env_u.step(acts); env_f.step(acts)
    assert torch.equal(env_u.patches, env_f.patches)
    # the rollout's patch stack
    tr = ja.ReinforceTrainer(_cfg(T=T), product)
    with torch.no_grad():
        ru = tr.rollout(env_u, sample_actions=False, start_positions=start)
        rf = tr.rollout(env_f, sample_actions=False, start_positions=start)
    assert torch.equal(ru["positions"], rf["positions"])
    assert torch.equal(ru["patches"], rf["patches"])
    # the indexed gather, every cell of every image and a zero patch
    cells = [(i, y, x) for i in range(B) for y in range(G) for x in range(G)] + [(-1, 0, 0)]
    c = torch.tensor(cells, dtype=torch.int64)
    gu = gather_indexed(u8, c[:, 0], c[:, 1:], P)
    gf = gather_indexed(f32, c[:, 0], c[:, 1:], P)
    assert torch.equal(gu, gf)
    want = torch.stack([f32[i, :, y * P:(y + 1) * P, x * P:(x + 1) * P] for i, y, x in cells[:-1]])
    assert torch.equal(gu[:-1], want) and int(gu[-1].abs().sum()) == 0
    # the detection batch: one indexed u8 gather against the fp32 env's slicing, same generator
    du = env_u.get_detection_batch(2, generator=torch.Generator().manual_seed(4))
    df = env_f.get_detection_batch(2, generator=torch.Generator().manual_seed(4))
    assert torch.equal(du[0], df[0]) and torch.equal(du[1], df[1])


def _rollout_pair(product, u8, bboxes, start, P, T, do_detection):
    tr = ja.ReinforceTrainer(_cfg(T=T), product)
    out = []
    for img, flag in ((u8, True), (_as_float(u8), False)):
        env = ja.NeedleGeneralEnv(img, bboxes, P, T, 1, True, uint8_images=flag)
        with torch.no_grad():
            r = tr.rollout(env, do_detection=do_detection, sample_actions=False, start_positions=start, keep_patches=False)
        torch.cuda.synchronize()
        out.append(r)
    return out


@pytest.mark.parametrize("P,B,T,arch", [
    (64, 4, 5, dict(image_processor="yolox-nano", detector_conf_threshold=0.05)),              # the smoke shapes
    (448, 8, 3, dict(image_processor="yolox-nano")),
    (64, 4, 5, dict(image_processor="yolox-nano", gpt_backbone="yolox-nano", act_dtype="bf16",       # bf16 storage
                    detector_conf_threshold=0.05)),
    (96, 4, 5, dict(with_detector=False, image_processor=None, gpt_backbone="yolox-s")),       # dense encoder stem
])
def test_uint8_eval_rollout_is_bit_identical(P, B, T, arch):
    G = 3
    product, _ = make_pair(5, patch_size=P, block_size=T, max_batch=B, **arch)
    u8 = _random_bytes(B, G * P, G * P, seed=P + B)
    _, bboxes, start = synth_batch(B, G, G, P, seed=23)
    det = arch.get("with_detector", True)
    ru, rf = _rollout_pair(product, u8, bboxes, start, P, T, det)
    for k in ("positions", "rewards", "masks", "actions", "logits", "final_emb"):
        assert torch.equal(ru[k], rf[k]), k
    if det:
        assert torch.equal(ru["det_counts"], rf["det_counts"])
        for bu, bf in zip(ru["bboxes"], rf["bboxes"]):
            for a, b in zip(bu, bf):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
        print(f"detections compared: {int(ru['det_counts'].sum())}")


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


def test_uint8_training_iteration_matches_fp32():
    """REINFORCE iteration with forced actions and detector training at 448 px (train-mode BatchNorm): the uint8 env
    against the fp32 env of the converted image, and two fp32 runs as the control, all to the same fixed bars."""
    P, T, B, G = 448, 3, 16, 3
    u8 = _random_bytes(B, G * P, G * P, seed=29)
    f32 = _as_float(u8)
    _, bboxes, start = synth_batch(B, G, G, 64, seed=31)
    bboxes = bboxes * (P // 64)
    forced = torch.randint(0, 8, (B, T), generator=torch.Generator().manual_seed(6))
    runs = []
    for img, flag in ((f32, False), (f32, False), (u8, True)):
        product, _ = make_pair(7, bn_seed=None, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
        cfg = _cfg(T=T, learning_rate=1e-3, gradient_accumulation=1)
        cfg.detection_enabled, cfg.yolo_lr = True, 2e-3
        tr = ja.ReinforceTrainer(cfg, product)
        env = ja.NeedleGeneralEnv(img, bboxes, P, T, 1, True, uint8_images=flag)
        torch.manual_seed(13)                  # the detection batch's negative patches (torch.randperm): the same draws
        m = tr.train_iteration(env, forced_actions=forced, start_positions=start, optimizer_step=False)
        assert m["steps"] == T and "yolo_total_loss" in m
        runs.append(({k: float(m[k]) for k in ("loss", "yolo_total_loss")}, product.engine_grads()))
        del product, tr, env
        torch.cuda.empty_cache()
    _check_training_pair(runs[0], runs[1], "fp32 vs fp32 (control)")
    _check_training_pair(runs[0], runs[2], "fp32 vs uint8")


def test_uint8_supervised_trajectories_and_iteration_match_fp32():
    P, T, B, G = 64, 6, 3, 4
    u8 = _random_bytes(B, G * P, G * P, seed=33)
    _, bboxes, _ = synth_batch(B, G, G, P, seed=3)
    cid = torch.zeros(B, dtype=torch.long)
    batches = {"u8": {"image": u8, "bboxes": bboxes, "class_id": cid},
               "f32": {"image": _as_float(u8), "bboxes": bboxes, "class_id": cid}}
    traj, runs = {}, {}
    for tag in ("f32", "f32 again", "u8"):
        product, _ = make_pair(9, patch_size=P, block_size=T, image_processor="yolox-nano", gpt_backbone="yolox-nano",
                               max_batch=B * T)
        cfg = ja.CfgNode(patch_size=P, max_seq_len=T, min_keypoints=0, max_keypoints=1, binomial_keypoints=False,
                         stop_enabled=True, stop_weight=1.0, learning_rate=1e-3, yolo_lr=1e-3, gradient_accumulation=1,
                         detection_enabled=True, uint8_images=True)
        tr = ja.SupervisedTrainer(cfg, product)
        batch = batches[tag.split()[0]]
        random.seed(13)                        # ties of the teacher walks
        traj[tag] = tr.generate_trajectories(batch, seed=5)
        random.seed(13)
        m = tr.train_iteration(batch, optimizer_step=False, seed=5)
        runs[tag] = ({k: float(m[k]) for k in ("loss", "yolo_total_loss")}, product.engine_grads())
        del product, tr
        torch.cuda.empty_cache()
    a, b = traj["f32"], traj["u8"]
    assert a["patches"].dtype == b["patches"].dtype == torch.float32
    for k in ("patches", "patches_yolox", "current_actions", "next_actions", "positions", "masks", "bboxes_yolox",
              "local_bboxes"):
        assert torch.equal(a[k], b[k]), k
    _check_training_pair(runs["f32"], runs["f32 again"], "supervised fp32 vs fp32 (control)")
    _check_training_pair(runs["f32"], runs["u8"], "supervised fp32 vs uint8")


def test_uint8_env_keeps_the_callers_bytes():
    P, T, B, G = 448, 3, 4, 3
    product, _ = make_pair(5, patch_size=P, block_size=T, image_processor="yolox-nano", max_batch=B)
    eng = product.engine()
    u8 = _random_bytes(B, G * P, G * P, seed=35)
    _, bboxes, start = synth_batch(B, G, G, P, seed=37)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    env = ja.NeedleGeneralEnv(u8, bboxes, P, T, 1, True, engine=eng, uint8_images=True)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert grown < u8.numel(), grown
    assert env.images.data_ptr() == u8.data_ptr() and env.images.shape == (B, 1, 3, G * P, G * P)
    assert torch.equal(env.images[:, 0], u8)
    env.reset(start)
    assert env.patches.dtype == torch.float32 and float(env.patches.max()) <= 1.0
    # without the option a uint8 tensor keeps today's meaning: an fp32 copy of the byte values
    env_old = ja.NeedleGeneralEnv(u8, bboxes, P, T, 1, True, engine=eng)
    assert env_old.images.dtype == torch.float32 and env_old.images.data_ptr() != u8.data_ptr()
    assert torch.equal(env_old.images[:, 0], u8.float())
