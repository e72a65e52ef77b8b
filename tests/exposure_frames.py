"""Images for the auto-exposure tests (tests/test_exposure_ref.py on the CPU, tests/test_gpu_exposure.py on the device): accumulation-
format H x W x 4 float32 made with numpy from a seed, pixels with a luminance that is exact to the bit, and the cases both files walk."""
import numpy as np

from heatray_amd import exposure
from heatray_amd.denoise import lum

F = np.float32


def bits(u):
    return np.array([u], np.uint32).view(F)[0]


def pixel_with_luminance(target):
    """(0, 0, b, a) whose luminance (0.2126 * 0 + 0.7152 * 0) + 0.0722 * (b / a) is `target` to the bit (target > 0)"""
    target = F(target)
    for a in (1, 3, 5, 7, 9, 11, 13):
        b0 = F(np.float64(target) * a / np.float64(F(0.0722)))
        for step in range(-4, 5):
            b = b0
            for _ in range(abs(step)):
                b = np.nextafter(b, F(np.inf) if step > 0 else F(0), dtype=F)
            if lum(F(0), F(0), F(b / F(a))).tobytes() == target.tobytes():
                return F([0, 0, b, a])
    raise AssertionError(f"no pixel found for luminance {target!r}")


# name: (the pixel, the class: a bin, or one of the four counters)
CLASS_PIXELS = {
    "+0": (F([0, 0, 0, 1]), "below"),
    "-0": (F([-0.0, -0.0, -0.0, 1]), "below"),
    "-1": (F([0, 0, -1, 2]), "below"),
    "largest denormal": (pixel_with_luminance(bits(0x007FFFFF)), "below"),
    "predecessor of 2^-16": (pixel_with_luminance(bits((111 << 23) - 1)), "below"),
    "2^-16": (pixel_with_luminance(bits(111 << 23)), 0),
    "1": (pixel_with_luminance(F(1)), 128),
    "predecessor of 2^16": (pixel_with_luminance(bits((143 << 23) - 1)), 255),
    "2^16": (pixel_with_luminance(bits(143 << 23)), "above"),
    "huge": (F([3e38, 3e38, 3e38, 1]), "above"),
    "NaN": (F([np.nan, 1, 1, 1]), "nonfinite"),
    "+Inf": (F([np.inf, 1, 1, 1]), "nonfinite"),
    "-Inf": (F([1, -np.inf, 1, 4]), "nonfinite"),
    "a = 0": (F([1, 1, 1, 0]), "invalid"),
    "a < 0": (F([1, 1, 1, -2]), "invalid"),
    "a = NaN": (F([1, 1, 1, np.nan]), "invalid"),
}


def class_row():
    """a 1-row image of CLASS_PIXELS, in its order"""
    return np.stack([p for p, _ in CLASS_PIXELS.values()])[None]


def seeded(W, H, seed, median=1.0, sigma=2.0, classes=True, max_n=9):
    """A log-normal image (sigma in octaves about `median`) with per-pixel sample counts 1 .. max_n, and with `classes` some pixels of
    every class of CLASS_PIXELS strewn in (a third of them unsampled, as in interactive mode's first frames)."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, max_n + 1, (H, W)).astype(F)
    c = (F(median) * np.exp2(F(sigma) * rng.standard_normal((H, W, 1)) + F(0.3) * rng.standard_normal((H, W, 3)))).astype(F)
    img = np.zeros((H, W, 4), F)
    img[..., :3], img[..., 3] = c * n[..., None], n
    if classes:
        px = np.stack([p for p, _ in CLASS_PIXELS.values()])
        pick = rng.random((H, W))
        img[pick < 0.1] = 0  # holes
        odd = (pick >= 0.1) & (pick < 0.2)
        img[odd] = px[rng.integers(0, len(px), int(odd.sum()))]
    return img


def flat(W, H, colour=(0.5, 0.25, 0.125), n=4):
    img = np.zeros((H, W, 4), F)
    img[..., :3], img[..., 3] = F(colour) * F(n), n
    return img


def all_bins(W, H):
    """every run of 256 consecutive pixels (row-major) holds every one of the 256 bins once: pixel i sits in bin i % 256"""
    i = np.arange(W * H)
    L = ((((i % 256) + 888).astype(np.uint32) << np.uint32(20)) | np.uint32(0x40000)).view(F)  # inside the bin, off its edge
    img = np.zeros((H * W, 4), F)
    img[:, 1], img[:, 3] = L / F(0.7152), 1  # (0.2126 * 0 + 0.7152 * g) + 0 lands in L's bin: the quotient's error is far from the edge
    return img.reshape(H, W, 4)


def windows(W, H):
    """name -> x0 y0 x1 y1: one pixel, one row, one column, everything but the border, the last pixel only (those the size allows)"""
    out = {"whole": (0, 0, 0, 0), "one pixel": (W // 2, H // 2, W // 2 + 1, H // 2 + 1), "one row": (0, H // 2, W, H // 2 + 1),
           "one column": (W // 3, 0, W // 3 + 1, H), "last pixel": (W - 1, H - 1, W, H)}
    if W > 2 and H > 2:
        out["inner"] = (1, 1, W - 1, H - 1)
    return out


def params(window=(0, 0, 0, 0), **kw):
    p = exposure.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    p.window[:] = window
    return p


def same_result(got, want, what):
    """two results (Engine.exposure_meter's dict, exposure.reference's) agree in every field, the floats to the bit"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = got[k], want[k]
        if isinstance(w, float):
            assert F(g).tobytes() == F(w).tobytes(), (what, k, got, want)
        else:
            assert int(g) == int(w), (what, k, got, want)
