"""Oracle-side helpers of the ragged-batch tests: seeded images of unequal size, each image padded on its own
(infer.py:138-146), and a CPU model whose detector gives confident, well separated scores — built only from ``oracle/``,
so that the seeds the GPU tests commit can be searched without a device (``find_seeds``)."""
import torch

from oracle import env_ref, rollout_ref
from oracle.gpt_ref import build_gpt_ref
from tests.helpers import randomize_bn

THR = 0.5            # the detector's confidence threshold in every ragged-batch test
LOGIT_GAP = 1e-3     # precondition of the batched-vs-loop comparison: top-2 logit gap at every executed step ...
SCORE_GAP = 1e-2     # ... and no candidate score this close to THR


def blocky_u8(h: int, w: int, seed: int) -> torch.Tensor:
    """uint8 [3, h, w]: random blocks at three resolutions plus noise (white noise alone gives features that hardly
    depend on the position)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(1, 3, h, w)
    for r in (4, 8, 16):
        x += torch.nn.functional.interpolate(torch.rand(1, 3, -(-h // r), -(-w // r), generator=g), size=(h, w), mode="nearest")
    x = (x / 3 + 0.1 * torch.rand(1, 3, h, w, generator=g)).clamp(0, 1)
    return (x[0] * 255).round().to(torch.uint8)


def image_set(sizes, seed: int):
    """[(uint8 image, [n, 4] boxes inside it)] for every (h, w) of `sizes`; one or two boxes each."""
    g = torch.Generator().manual_seed(seed + 1000)
    out = []
    for i, (h, w) in enumerate(sizes):
        n = 1 + i % 2
        rows = []
        for _ in range(n):
            bw, bh = (int(torch.randint(4, max(5, d // 3), (1,), generator=g)) for d in (w, h))
            x, y = int(torch.randint(0, w - bw, (1,), generator=g)), int(torch.randint(0, h - bh, (1,), generator=g))
            rows.append([x, y, x + bw, y + bh])
        out.append((blocky_u8(h, w, seed * 100 + i), torch.tensor(rows, dtype=torch.long)))
    return out


def pad_own(img: torch.Tensor, P: int) -> torch.Tensor:
    """[3, h, w] -> zero-padded bottom / right to its own multiple of P."""
    h, w = img.shape[-2:]
    return torch.nn.functional.pad(img, (0, -(-w // P) * P - w, 0, -(-h // P) * P - h), value=0)


def build_oracle(weight_seed: int, P: int, T: int, calib: torch.Tensor, scale: float = 2000.0, keep: float = 0.03, **kw):
    """CPU oracle model (gpt-nano, yolox-nano encoder and detector unless `kw` says otherwise) with BatchNorm statistics
    of real patches in the detector and saturated predictors: with l the objectness (class) logit of the random-init
    head and v its 1 - `keep` (`keep`) quantile over the calibration patches, the logit becomes scale * (l - v), so that
    about `keep` of the candidates score ~1, the rest ~0 and hardly any sits near THR."""
    kw.setdefault("image_processor", "yolox-nano")
    oracle = build_gpt_ref(weight_seed, patch_size=P, block_size=T, detector_conf_threshold=THR, **kw)
    randomize_bn(oracle, 5)
    bns = [m for m in oracle.yolox.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    oracle.yolox.train()
    h = oracle.yolox.head
    with torch.no_grad():
        f = oracle.yolox.backbone(calib)
        for k in range(3):
            t = h.stems[k](f[k]); h.cls_convs[k](t); h.reg_convs[k](t)
    for m in bns:
        m.momentum = 0.03
    oracle.eval()
    with torch.no_grad():
        raw = h(oracle.yolox.backbone(calib))
        for preds, col, q in ((h.obj_preds, 4, 1.0 - keep), (h.cls_preds, 5, keep)):
            v = float(torch.quantile(torch.logit(raw[..., col].flatten().double()), q))
            for k in range(3):
                preds[k].weight.mul_(scale)
                preds[k].bias.copy_(scale * (preds[k].bias - v))
    return oracle


def calib_patches(images, P: int) -> torch.Tensor:
    """The top-left patch of every image padded on its own, fp32 in [0, 1]."""
    return torch.stack([pad_own(im, P)[:, :P, :P].float().div(255) for im, _ in images])


@torch.no_grad()
def margins(oracle, images, P: int, T: int, stop: bool = True):
    """Per image, from its own greedy ``B = 1`` oracle rollout with detection from the start patch (0, 0):
    (smallest top-2 logit gap over the executed steps, smallest |obj * cls - THR| over every candidate of every visited
    patch, number of boxes found, steps)."""
    out = []
    for im, boxes in images:
        x = pad_own(im, P).float().div(255).unsqueeze(0)
        env = env_ref.EnvRef(x, boxes.unsqueeze(0), P, T, 1, stop)
        ro = rollout_ref.rollout(oracle, env, do_detection=True, sample_actions=False, start_positions=torch.zeros((1, 2), dtype=torch.long))
        top = ro["logits"][0].topk(2, dim=-1).values
        raw = oracle.yolox.head(oracle.yolox.backbone(ro["patches"][0]))
        score = raw[..., 4] * raw[..., 5]
        n = sum(0 if b is None else len(b) for b in ro["bboxes"][0])
        out.append((float((top[:, 0] - top[:, 1]).min()), float((score - THR).abs().min()), n, ro["rewards"].shape[1]))
    return out


def find_seeds(sizes, P: int, T: int, tries: int = 50, safety: float = 3.0, **kw):
    """The first (weight seed, image seed) whose every image clears the preconditions with `safety` to spare and finds
    at least one box somewhere; how the seeds in tests/test_gpu_ragged_batch.py were chosen."""
    for s in range(tries):
        images = image_set(sizes, s)
        oracle = build_oracle(s, P, T, calib_patches(images, P), **kw)
        m = margins(oracle, images, P, T)
        ok = all(g >= safety * LOGIT_GAP and d >= safety * SCORE_GAP for g, d, _, _ in m) and sum(n for _, _, n, _ in m) > 0
        print(s, ok, [(round(g, 4), round(d, 4), n, st) for g, d, n, st in m], flush=True)
        if ok:
            return s
    return None
