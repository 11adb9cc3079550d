"""uint8 images without a GPU: the byte-image entry points of the C ABI, their argument checks, the byte arithmetic the
kernels use, and the uint8 forms of the batch helpers."""
import ctypes as C

import numpy as np
import pytest
import torch

import jolineedle_amd as ja
from jolineedle_amd import _lib

U8_ENTRY_POINTS = ("jn_env_init_u8", "jn_gather_patches_u8", "jn_gather_patches_indexed_u8")


def _library():
    try:
        return _lib.load_library()
    except _lib.LibraryNotBuilt as e:          # the suite's other library tests need the build as well
        pytest.fail(str(e))


def test_uint8_entry_points_are_exported_and_bound():
    lib = _library()
    header = open(_lib.Path(__file__).resolve().parent.parent / "include" / "jnroll.h").read()
    for name in U8_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert f"{name}(" in header, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == _lib.SIGNATURES[name][1]
    # each takes the arguments of its fp32 twin
    for name in U8_ENTRY_POINTS:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-3]], name


def test_uint8_gathers_reject_null_pointers_with_a_message():
    lib = _library()
    rc = lib.jn_gather_patches_u8(None, None, None, 1, 3, 64, 64, 32, None)
    assert rc == -1                                                  # JN_EINVAL
    assert b"jn_gather_patches_u8" in lib.jn_last_error()
    rc = lib.jn_gather_patches_indexed_u8(None, None, None, None, 1, 1, 3, 64, 64, 32, None)
    assert rc == -1
    assert b"jn_gather_patches_indexed_u8" in lib.jn_last_error()
    rc = lib.jn_env_init_u8(None, None, None, 1, 64, 64, 0, 1, 0, None)
    assert rc == -1
    assert b"jn_env_init_u8" in lib.jn_last_error()


def test_byte_to_unit_arithmetic_is_exact_for_every_byte():
    """The kernels compute b / 255 as q = b * fl(1/255), then q + fma(-q, 255, b) * fl(1/255) (jn_types.h: u8_unit).
    Evaluated here with exact rationals and one rounding per operation, it equals ToTensor's u8.float().div(255) for all
    256 bytes; the plain product does not (126 bytes differ)."""
    from fractions import Fraction

    def rn(x: Fraction) -> np.float32:                               # round to nearest-even fp32 (normal range)
        if x == 0:
            return np.float32(0.0)
        m, e = abs(x), 0
        while m >= 2:
            m, e = m / 2, e + 1
        while m < 1:
            m, e = m * 2, e - 1
        s = m * (1 << 23)
        n, rem = s.numerator // s.denominator, s - s.numerator // s.denominator
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
            n += 1
        return np.float32((1 if x > 0 else -1) * float(Fraction(n, 1 << 23) * Fraction(2) ** e))

    want = torch.arange(256, dtype=torch.uint8).float().div(255).numpy()
    assert np.array_equal(want, np.arange(256, dtype=np.float32) / np.float32(255))
    r = Fraction(float(np.float32(1) / np.float32(255)))
    plain = corrected = 0
    for b in range(256):
        q = rn(Fraction(b) * r)
        e = rn(Fraction(b) - Fraction(float(q)) * 255)               # fma(-q, 255, b)
        q1 = rn(Fraction(float(e)) * r + Fraction(float(q)))        # fma(e, r, q)
        plain += q != want[b]
        corrected += q1 != want[b]
    assert corrected == 0
    assert plain == 126


def test_synthetic_batch_uint8_is_deterministic_spans_the_bytes_and_keeps_boxes_and_starts():
    a = ja.synthetic_batch(3, 3, 64, seed=11, device="cpu", dtype=torch.uint8)
    b = ja.synthetic_batch(3, 3, 64, seed=11, device="cpu", dtype=torch.uint8)
    f = ja.synthetic_batch(3, 3, 64, seed=11, device="cpu")
    assert a["image"].dtype == torch.uint8 and a["image"].shape == (3, 3, 192, 192)
    assert torch.equal(a["image"], b["image"])
    assert int(a["image"].min()) == 0 and int(a["image"].max()) == 255
    assert len(torch.unique(a["image"])) == 256
    assert f["image"].dtype == torch.float32
    for k in ("bboxes", "start_positions", "class_id"):
        assert torch.equal(a[k], f[k]), k
    c = ja.synthetic_batch(3, 3, 64, seed=12, device="cpu", dtype=torch.uint8)
    assert not torch.equal(a["image"], c["image"])


def test_padded_collate_keeps_uint8():
    ims = [torch.randint(0, 256, (3, 50, 70), dtype=torch.uint8), torch.randint(0, 256, (3, 64, 40), dtype=torch.uint8)]
    boxes = [torch.tensor([[1, 2, 10, 20]]), torch.zeros((0, 4), dtype=torch.long)]
    out = ja.padded_collate(ims, boxes, 32)
    assert out["image"].dtype == torch.uint8 and out["image"].shape == (2, 3, 64, 96)
    assert torch.equal(out["image"][0, :, :50, :70], ims[0])
    assert torch.equal(out["image"][1, :, :64, :40], ims[1])
    assert int(out["image"][0, :, 50:].abs().sum()) == 0
