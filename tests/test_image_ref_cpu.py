"""CPU: tests/image_ref.py, the restatement that pins the contract of c3dgs_image_from_u8, checked on hand cases and against its
own fp64 form on the shapes the GPU test runs."""
import numpy as np
import pytest

from tests import image_ref
from tests.image_ref import BOUND, SHAPES, image_from_u8


def _bytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def test_same_size_is_the_texel_value():
    for C in (3, 4):
        src = _bytes((7, 5, C), 1)
        out = image_from_u8(src, 7, 5)
        want = src[:, :, :3].astype(np.float32) / np.float32(255)
        if C == 4:
            want = want * (src[:, :, 3:4].astype(np.float32) / np.float32(255))
        assert out.dtype == np.float32 and out.shape == (3, 7, 5)
        assert np.array_equal(out, want.transpose(2, 0, 1))
    every = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    assert np.array_equal(image_from_u8(every, 16, 16)[0].ravel(), np.arange(256, dtype=np.float32) / np.float32(255))


def test_two_by_two_to_one_is_the_mean():
    src = np.array([[[0, 10, 255], [100, 20, 255]], [[200, 30, 255], [60, 40, 255]]], dtype=np.uint8)
    out = image_from_u8(src, 1, 1, dtype=np.float64)
    assert np.allclose(out.ravel(), src.reshape(4, 3).mean(axis=0) / 255.0, rtol=0, atol=1e-15)
    assert np.abs(image_from_u8(src, 1, 1).astype(np.float64) - out).max() <= BOUND


def test_enlarging_a_line_clamps_at_the_edges():
    row = _bytes((1, 4, 3), 2)
    out = image_from_u8(row, 3, 16)
    first, last = row[0, 0].astype(np.float32) / np.float32(255), row[0, -1].astype(np.float32) / np.float32(255)
    assert np.array_equal(out[:, :, 0], np.repeat(first[:, None], 3, axis=1))      # f < 0 at the left edge: tap 0, weight 0
    assert np.array_equal(out[:, :, 1], out[:, :, 0])
    assert np.array_equal(out[:, :, -1], np.repeat(last[:, None], 3, axis=1))
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])   # one source row: rows repeat
    col = row.transpose(1, 0, 2)
    assert np.array_equal(image_from_u8(col, 16, 3), out.transpose(0, 2, 1))


def test_taps_follow_the_documented_rule():
    s0, s1, f = image_ref.taps(4, 9)                       # scale 2.25: f = (d + .5) * 2.25 - .5
    assert s0.tolist() == [0, 2, 5, 7] and s1.tolist() == [1, 3, 6, 8]
    assert f.tolist() == [0.625, 0.875, 0.125, 0.375]
    s0, s1, f = image_ref.taps(5, 1)
    assert s0.tolist() == [0] * 5 and s1.tolist() == [0] * 5 and f.tolist() == [0.0] * 5
    s0, s1, f = image_ref.taps(6, 3)                       # scale .5: -0.25 .25 .75 1.25 1.75 2.25
    assert s0.tolist() == [0, 0, 0, 1, 1, 2] and s1.tolist() == [1, 1, 1, 2, 2, 2]
    assert f.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.0]


@pytest.mark.parametrize("C", (3, 4))
def test_flip_is_the_reference_on_the_flipped_array(C):
    src = _bytes((23, 37, C), 3)
    for Hd, Wd in ((9, 16), (31, 53), (23, 37)):
        assert np.array_equal(image_from_u8(src, Hd, Wd, flip=1), image_from_u8(np.ascontiguousarray(src[::-1, ::-1]), Hd, Wd))
    assert not np.array_equal(image_from_u8(src, 9, 16, flip=1), image_from_u8(src, 9, 16))


def test_alpha_and_background():
    rgb = _bytes((6, 5, 3), 4)
    bg = np.array([0.25, 1.0, 0.6], dtype=np.float32)
    plain = image_from_u8(rgb, 6, 5)
    opaque = np.concatenate([rgb, np.full((6, 5, 1), 255, np.uint8)], axis=2)
    clear = np.concatenate([rgb, np.zeros((6, 5, 1), np.uint8)], axis=2)
    assert np.array_equal(image_from_u8(opaque, 6, 5), plain)
    assert np.array_equal(image_from_u8(opaque, 6, 5, bg=bg), plain)
    assert not image_from_u8(clear, 6, 5).any()
    assert np.array_equal(image_from_u8(clear, 6, 5, bg=bg), np.broadcast_to(bg[:, None, None], (3, 6, 5)))
    mixed = np.concatenate([rgb, _bytes((6, 5, 1), 5)], axis=2)
    assert np.array_equal(image_from_u8(mixed, 4, 3, bg=np.zeros(3, np.float32)), image_from_u8(mixed, 4, 3))
    a = mixed[:, :, 3:4].astype(np.float64) / 255
    want = rgb / 255.0 * a + bg.astype(np.float64) * (1 - a)
    assert np.abs(image_from_u8(mixed, 6, 5, bg=bg).transpose(1, 2, 0) - want).max() <= 4 * 2.0 ** -24
    with pytest.raises(ValueError):
        image_from_u8(rgb, 6, 5, bg=bg)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_fp32_form_is_within_the_bound_of_the_fp64_form(shape):
    (Hs, Ws), (Hd, Wd) = shape
    worst = 0.0
    for C in (3, 4):
        src = _bytes((Hs, Ws, C), 10 + C)
        for flip in (0, 1):
            for bg in (None,) if C == 3 else (None, np.ones(3, np.float32), np.array([0.1, 0.7, 0.33], np.float32)):
                lo, hi = image_from_u8(src, Hd, Wd, flip, bg), image_from_u8(src, Hd, Wd, flip, bg, dtype=np.float64)
                assert lo.dtype == np.float32 and hi.dtype == np.float64 and lo.shape == hi.shape == (3, Hd, Wd)
                worst = max(worst, float(np.abs(lo.astype(np.float64) - hi).max()))
    print(f"{shape}: max |fp32 - fp64| = {worst / 2.0 ** -24:.3f} u")
    assert worst <= BOUND


def test_division_free_quotient_is_the_correctly_rounded_one():
    """csrc/image_io.hip forms fl(u / 255) with one multiply and two fused multiply-adds; for all 256 bytes that is the correctly
    rounded quotient, which is also what numpy's fp32 division gives."""
    for u in range(256):
        got, want = image_ref.unit_by_fma(u)
        assert got == want, u
        assert float(want) == float(np.float32(u) / np.float32(255)), u
