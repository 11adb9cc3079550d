"""Image views on the CPU side: the draws, box arithmetic and pixel mapping of ``ImageViews`` against what the
reference's ``NeedleDataset.rotate`` / ``translate`` produced (tests/golden/g9_image_views.npz, recorded by
tests/golden/make_golden_views.py), the direction of the shift, the C struct and the new entry points."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib
from jolineedle_amd.views import ImageViews, rotate_boxes
from tests.views_ref import canvas_ref, shift_zero_fill

ROOT = Path(__file__).resolve().parent.parent
G9 = np.load(ROOT / "tests" / "golden" / "g9_image_views.npz")
NAMES = [str(n) for n in G9["names"]]
P = 8            # every stored size of the fixture is a multiple of 8


def _ramp(Hs, Ws):
    return torch.arange(3 * Hs * Ws, dtype=torch.float32).reshape(3, Hs, Ws)


def _case(name):
    Hs, Ws, seed, rotations, translations = (int(v) for v in G9[f"{name}.args"])
    boxes = torch.from_numpy(G9[f"{name}.boxes"])[None]
    views = ImageViews.sample(_ramp(Hs, Ws)[None], boxes, bool(rotations), bool(translations),
                              np.random.default_rng(seed), P)
    return views, boxes, seed, bool(rotations), bool(translations)


def test_fixture_covers_all_four_angles_and_a_zero_margin():
    angles = set()
    for name in NAMES:
        views, *_ = _case(name)
        angles.add(int(views.rot[0]))
    assert angles == {0, 90, 180, 270}
    assert len(NAMES) >= 12
    assert any(0 in G9[f"{n}.translate_xy"].tolist() for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_sample_reproduces_the_reference_draws_and_boxes(name):
    views, boxes, seed, rotations, translations = _case(name)
    Hs, Ws = views.stored_hw[0]
    rotated = G9[f"{name}.rotated"]
    # the angle: the one whose mapping gives the reference's rotated ramp (the ramp's values are all different)
    want_rot = []
    for k in (0, 90, 180, 270):
        hw = (Ws, Hs) if k in (90, 270) else (Hs, Ws)
        if hw == tuple(rotated.shape[1:]) and np.array_equal(canvas_ref(_ramp(Hs, Ws).numpy(), k, 0, 0, *hw), rotated.astype(np.float32)):
            want_rot.append(k)
    assert want_rot == [int(views.rot[0])]
    tx, ty = (int(v) for v in G9[f"{name}.translate_xy"])
    assert (int(views.tx[0]), int(views.ty[0])) == (tx, ty)
    assert np.array_equal(rotate_boxes(boxes[0].numpy(), Hs, Ws, int(views.rot[0])), G9[f"{name}.rotated_boxes"])
    assert np.array_equal(views.transform_bboxes(boxes)[0].numpy(), G9[f"{name}.final_boxes"])
    # ... and the generator stands where the reference left it: no draw too many, none too few
    rng = np.random.default_rng(seed)
    ImageViews.sample(_ramp(Hs, Ws)[None], boxes, rotations, translations, rng, P)
    assert int(rng.integers(0, 1 << 30, (1,))[0]) == int(G9[f"{name}.rng_after"][0])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_materialize_is_the_rotated_ramp_shifted_with_zero_fill(name, dtype):
    Hs, Ws, seed, rotations, translations = (int(v) for v in G9[f"{name}.args"])
    src = _ramp(Hs, Ws) if dtype == torch.float32 else (_ramp(Hs, Ws) % 251).to(torch.uint8)
    boxes = torch.from_numpy(G9[f"{name}.boxes"])[None]
    views = ImageViews.sample(src[None], boxes, bool(rotations), bool(translations), np.random.default_rng(seed), P)
    got = views.materialize()
    assert got.dtype == dtype and tuple(got.shape[2:]) == views.canvas
    rotated = G9[f"{name}.rotated"].astype(np.float32)
    if dtype == torch.uint8:
        rotated = (rotated % 251).astype(np.uint8)
    tx, ty = (int(v) for v in G9[f"{name}.translate_xy"])
    want = shift_zero_fill(rotated, ty, tx)
    Hr, Wr = want.shape[1:]
    assert views.canvas == (-(-Hr // P) * P, -(-Wr // P) * P)        # padded_collate_fn's canvas
    assert np.array_equal(got[0, :, :Hr, :Wr].numpy(), want)
    assert not got[0, :, Hr:].any() and not got[0, :, :, Wr:].any()
    # the definition of the C header, pixel by pixel
    assert np.array_equal(got[0].numpy(), canvas_ref(src.numpy(), int(views.rot[0]), ty, tx, *views.canvas))


def test_unrotated_content_follows_the_moved_box():
    """Fixes the direction of the shift without torchvision: the reference moves a box by +(tx, ty); the pixels under
    the moved box must be the stored pixels under the original box."""
    src = _ramp(32, 48)
    box = torch.tensor([[[10, 8, 20, 17]]])
    for ty, tx in [(0, 0), (3, 5), (-4, 7), (6, -9), (-8, -10), (14, 27)]:
        views = ImageViews(src[None], [0], [ty], [tx], patch_size=P)
        x1, y1, x2, y2 = views.transform_bboxes(box)[0, 0].tolist()
        assert (x1, y1, x2, y2) == (10 + tx, 8 + ty, 20 + tx, 17 + ty)
        assert torch.equal(views.materialize()[0, :, y1:y2 + 1, x1:x2 + 1], src[:, 8:18, 10:21])


def test_list_of_images_of_different_sizes_shares_one_canvas():
    srcs = [_ramp(16, 24), _ramp(24, 8), _ramp(8, 8)]
    views = ImageViews(srcs, [90, 0, 180], [1, -2, 0], [0, 3, -1], patch_size=P)
    assert views.canvas == (24, 16)
    got = views.materialize()
    for i, s in enumerate(srcs):
        assert np.array_equal(got[i].numpy(), canvas_ref(s.numpy(), int(views.rot[i]), int(views.ty[i]), int(views.tx[i]), 24, 16))
    with pytest.raises(AssertionError):
        ImageViews(srcs, [0, 0, 0], canvas=(16, 16))                 # the second image does not fit


def test_image_without_boxes_gets_no_translation_and_no_draw():
    rng = np.random.default_rng(5)
    boxes = torch.zeros((2, 1, 4), dtype=torch.int64)
    boxes[1, 0] = torch.tensor([3, 3, 9, 9])
    views = ImageViews.sample(torch.stack([_ramp(16, 16), _ramp(16, 16)]), boxes, False, True, rng, P)
    assert (int(views.ty[0]), int(views.tx[0])) == (0, 0)
    want = np.random.default_rng(5)
    tx = int(want.integers(-3, 5, (1,))[0])          # margins of image 1: min(16 // 3, 3) and min(16 // 3, 16 - 9)
    ty = int(want.integers(-3, 5, (1,))[0])
    assert (int(views.tx[1]), int(views.ty[1])) == (tx, ty)
    assert torch.equal(views.transform_bboxes(boxes)[0], boxes[0])     # a padding row stays zero


def test_struct_layout_and_symbols():
    header = (ROOT / "include" / "jnroll.h").read_text()
    body = header[header.index("typedef struct jn_image_view {"):header.index("} jn_image_view;")]
    fields = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip()
        m = re.match(r"(const void\*|int32_t)\s+([^;]+);", line)
        if m:
            fields += [f.strip() for f in m.group(2).split(",")]
    assert fields == [f[0] for f in _lib.JnImageView._fields_]
    assert C.sizeof(_lib.JnImageView) == 32 and _lib.JnImageView.src_u8.offset == 8 and _lib.JnImageView.tx.offset == 28
    lib = _lib.load_library()
    for name in ("jn_env_init_views", "jn_gather_patches_views"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert lib.jn_abi_version() == 2
    # null arguments are refused before anything touches a device
    assert lib.jn_env_init_views(None, None, None, 1, 8, 8, 0, 1, 0, None) == -1
    assert lib.jn_gather_patches_views(None, 1, None, None, None, 0, 1, 8, 8, 8, None) == -1


def test_args_to_config_carries_the_augmentation_flags():
    args = ja.get_args(["--augment-rotate", "--augment-translate", "--min-keypoints", "1", "--max-keypoints", "3",
                        "--binomial-keypoints", "--loss", "on-self-trajectory"])
    t, _ = ja.args_to_config(args)
    assert t.rotations is True and t.translations is True
    assert (t.min_keypoints, t.max_keypoints, t.binomial_keypoints, t.loss_mode) == (1, 3, True, "on-self-trajectory")
    t, _ = ja.args_to_config(ja.get_args([]))
    assert t.rotations is False and t.translations is False and t.loss_mode == "on-optimal-trajectory"


def test_trainers_draw_nothing_without_the_flags(monkeypatch):
    from jolineedle_amd import views as views_mod

    class Boom:
        def __init__(self, *a, **k):
            raise AssertionError("ImageViews constructed without --augment-rotate / --augment-translate")
        sample = classmethod(lambda cls, *a, **k: cls())
    monkeypatch.setattr(views_mod, "ImageViews", Boom)

    class T:
        config = ja.CfgNode(rotations=False, translations=False, seed=3)
        rank = 0
    assert views_mod.trainer_views(T(), torch.zeros(1, 3, 8, 8), torch.zeros(1, 0, 4), 8) is None
    T.config = ja.CfgNode(rotations=True, translations=False, seed=3)
    with pytest.raises(AssertionError):
        views_mod.trainer_views(T(), torch.zeros(1, 3, 8, 8), torch.zeros(1, 0, 4), 8)


def test_trainer_draws_are_seeded_per_rank():
    from jolineedle_amd.views import trainer_views

    def draws(rank):
        class T:
            config = ja.CfgNode(rotations=True, translations=True, seed=7)
        t = T()
        t.rank = rank
        imgs = torch.stack([_ramp(32, 32)] * 6)
        boxes = torch.tensor([[[8, 8, 20, 20]]] * 6)
        out = []
        for _ in range(2):                            # the generator goes on from batch to batch
            v = trainer_views(t, imgs, boxes, 8)
            out.append((v.rot.tolist(), v.ty.tolist(), v.tx.tolist()))
        return out
    assert draws(0) == draws(0) and draws(1) == draws(1)
    assert draws(0) != draws(1) and draws(0)[0] != draws(0)[1]
