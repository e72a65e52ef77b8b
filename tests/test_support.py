"""device_support.same, the comparison every bit-exact test ends in (no GPU needed): the cases in which its earlier per-file copies gave
different answers."""
import numpy as np
import pytest

from device_support import same

F = np.float32


def test_identical_arrays_pass_nan_payloads_included():
    a = np.random.default_rng(1).random((41, 67, 4)).astype(F)
    a.view(np.uint32)[3, 5] = (0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001)  # quiet and signalling NaNs, each with its own payload
    assert np.isnan(a[3, 5]).all()
    same(a, a.copy(), "identical")


def test_minus_zero_against_plus_zero_names_the_pixel_and_the_count():
    a = np.zeros((41, 67, 4), F)
    b = a.copy()
    b[7, 30, 2] = b[9, 11, 0] = -0.0
    assert (a == b).all()
    with pytest.raises(AssertionError, match=r"zeros: 2 pixels differ, first at \(x=30, y=7\)"):
        same(a, b, "zeros")


def test_equal_bytes_of_another_dtype_are_refused():
    a = np.random.default_rng(2).random((5, 6, 4)).astype(F)
    with pytest.raises(AssertionError, match="float32.*uint32"):
        same(a, a.view(np.uint32), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        same(a, a.reshape(6, 5, 4), "shape")


def test_a_display_image_and_a_slice_that_is_not_contiguous():
    img = np.random.default_rng(3).integers(0, 256, (41, 67, 4), dtype=np.uint8)
    same(img, img.copy(), "uint8")
    other = img.copy()
    other[40, 0, 3] ^= 1
    with pytest.raises(AssertionError, match=r"1 pixels differ, first at \(x=0, y=40\)"):
        same(img, other, "uint8")
    f = np.random.default_rng(4).random((41, 67, 4)).astype(F)
    g = f.copy()
    assert not f[..., 3:].flags["C_CONTIGUOUS"]
    same(f[..., 3:], g[..., 3:], "alpha")
    same(f[..., 3], g[..., 3], "alpha, H x W")
    g[2, 1, 3] = 9
    same(f[..., :3], g[..., :3], "rgb")
    with pytest.raises(AssertionError, match=r"1 pixels differ, first at \(x=1, y=2\)"):
        same(f[..., 3], g[..., 3], "alpha, H x W")


def test_a_difference_at_the_last_pixel_is_reported_there():
    a = np.random.default_rng(5).random((41, 67, 4)).astype(F)
    b = a.copy()
    b[40, 66, 3] = np.nextafter(b[40, 66, 3], F(2))
    with pytest.raises(AssertionError, match=r"last: 1 pixels differ, first at \(x=66, y=40\)"):
        same(a, b, "last")
