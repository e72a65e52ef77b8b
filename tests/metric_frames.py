"""Images for the convergence-metric tests (tests/test_metric_ref.py on the CPU, tests/test_gpu_metric.py on the device): pairs of
accumulation-format H x W x 4 float32 images made with numpy from a seed, pairs whose terms are known to the bit, frames with their
MOMENTS plane for the estimate, and the comparisons both files make."""
import numpy as np

from exposure_frames import windows  # noqa: F401  (the same named windows: one pixel, one row, one column, inner, last pixel)
from heatray_amd import metric

F = np.float32
SIZES = [(1, 1), (67, 35), (257, 3), (3, 257), (256, 4)]

# name: (the image's pixel, the reference's pixel, the class, differing)
CLASS_PIXELS = {
    "identical": (F([2, 1, 0.5, 4]), F([2, 1, 0.5, 4]), "counted", False),
    "same colour, other count": (F([2, 1, 0.5, 4]), F([1, 0.5, 0.25, 2]), "counted", False),
    "differing": (F([2, 1, 0.5, 4]), F([2, 1, 0.75, 4]), "counted", True),
    "a = 0 in the image": (F([1, 1, 1, 0]), F([2, 1, 0.5, 4]), "counted", True),
    "a < 0 in the image": (F([1, 1, 1, -2]), F([2, 1, 0.5, 4]), "counted", True),
    "a = 0 in the reference": (F([2, 1, 0.5, 4]), F([1, 1, 1, 0]), "counted", True),
    "a < 0 in both": (F([1, 2, 3, -1]), F([3, 2, 1, -4]), "counted", False),
    "a = NaN in the image": (F([1, 1, 1, np.nan]), F([0, 0, 0, 1]), "counted", False),
    "a tiny difference whose square is denormal": (F([1e-20, 0, 0, 1]), F([0, 0, 0, 1]), "counted", True),
    "a difference whose square underflows to 0": (F([1e-30, 0, 0, 1]), F([0, 0, 0, 1]), "counted", True),
    "NaN in the image": (F([np.nan, 1, 1, 1]), F([1, 1, 1, 1]), "nonfinite", False),
    "NaN in the reference": (F([1, 1, 1, 1]), F([1, np.nan, 1, 1]), "nonfinite", False),
    "+Inf in the image": (F([1, 1, np.inf, 1]), F([1, 1, 1, 1]), "nonfinite", False),
    "-Inf in the reference": (F([1, 1, 1, 1]), F([-np.inf, 1, 1, 2]), "nonfinite", False),
    "1e30 in the image: d * d overflows": (F([1e30, 1, 1, 1]), F([1, 1, 1, 1]), "nonfinite", False),
    "1e30 in the reference: cR * cR overflows": (F([1, 1, 1, 1]), F([1, 1e30, 1, 1]), "nonfinite", False),
}


def class_rows():
    """two 1-row images of CLASS_PIXELS, in its order"""
    return np.stack([p[0] for p in CLASS_PIXELS.values()])[None], np.stack([p[1] for p in CLASS_PIXELS.values()])[None]


def seeded_pair(W, H, seed, median=1.0, sigma=2.0, noise=0.2, classes=True, max_n=9):
    """(image, reference): a log-normal reference (sigma in octaves about `median`, 64 samples per pixel) and an image of 1 .. max_n
    samples per pixel that is the reference's colour times a log-normal factor; with `classes`, pixels of CLASS_PIXELS and holes strewn in"""
    rng = np.random.default_rng(seed)
    c = (F(median) * np.exp2(F(sigma) * rng.standard_normal((H, W, 1)) + F(0.3) * rng.standard_normal((H, W, 3)))).astype(F)
    n = rng.integers(1, max_n + 1, (H, W)).astype(F)
    ref, img = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    ref[..., :3], ref[..., 3] = c * F(64), 64
    img[..., :3], img[..., 3] = (c * np.exp2(F(noise) * rng.standard_normal((H, W, 3))).astype(F)) * n[..., None], n
    if classes:
        pick = rng.random((H, W))
        img[pick < 0.1] = 0  # holes, as in interactive mode's first frames
        same = (pick >= 0.1) & (pick < 0.15)
        img[same] = ref[same]
        odd = (pick >= 0.15) & (pick < 0.3)
        which = rng.integers(0, len(CLASS_PIXELS), int(odd.sum()))
        img[odd] = np.stack([p[0] for p in CLASS_PIXELS.values()])[which]
        ref[odd] = np.stack([p[1] for p in CLASS_PIXELS.values()])[which]
    return img, ref


def constant_difference(W, H):
    """every channel of every pixel differs by 2^-3, exactly; the reference is 0.5 everywhere: every x is 2^-6 and every y 2^-2, one bin each"""
    ref, img = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    ref[...] = (1.0, 1.0, 1.0, 2.0)
    img[...] = (2.5, 2.5, 2.5, 4.0)
    return img, ref


def bin_value(e):
    """a float32 d whose square lies well inside exponent bin e (0: a denormal square)"""
    target = 2.0 ** -128 if e == 0 else 1.5 * 2.0 ** (e - 127)
    return F(np.sqrt(target))


def all_bins_pair(W, H):
    """channel k of pixel i has d = cR with d * d in bin (3 i + k) % 255: any 85 consecutive pixels (row-major) put one term into every
    bin 0 .. 254 of both sums"""
    d = np.array([bin_value(e) for e in range(255)], F)
    idx = (3 * np.arange(W * H)[:, None] + np.arange(3)[None, :]) % 255
    ref, img = np.ones((W * H, 4), F), np.ones((W * H, 4), F)
    ref[:, :3] = d[idx]
    img[:, :3] = F(2) * d[idx]  # (2 d - d = d exactly)
    return img.reshape(H, W, 4), ref.reshape(H, W, 4)


def last_pixel_differs(W, H, seed=3):
    _, ref = seeded_pair(W, H, seed, classes=False)
    img = ref.copy()
    img[-1, -1, 1] += F(0.5) * img[-1, -1, 3]
    return img, ref


def estimate_frame(W, H, seed, samples=16, sigma=0.15):
    """(frame, moments, truth): `samples` iid Gaussian samples per pixel about a smooth image `truth` (H x W x 3), summed into the frame
    (a = samples) and, squared, into the MOMENTS plane.  A sample's noise is one Gaussian added to all three channels: lum(vc), the
    weighted mean of the channels' variances (adError's line), is the luminance's variance exactly when the channels' noise is common;
    for independent channels it overstates it."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    truth = np.stack([0.6 + 0.3 * np.sin(x / 9.0), 0.5 + 0.3 * np.cos(y / 7.0), 0.4 + 0.2 * np.sin((x + y) / 11.0)], -1)
    s = (truth[None] + sigma * rng.standard_normal((samples, H, W, 1))).astype(F)
    frame, moments = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    for k in range(samples):  # (summed in float32 in sample order, as the device accumulates)
        frame[..., :3] += s[k]
        moments[..., :3] += s[k] * s[k]
    frame[..., 3] = samples
    return frame, moments, truth.astype(F)


def estimate_with_classes(W, H, seed):
    """estimate_frame with pixels of every class strewn in: fewer than 2 samples (0, 1, a negative count, NaN), non-finite sums and moments"""
    frame, moments, _ = estimate_frame(W, H, seed, samples=5)
    rng = np.random.default_rng(seed + 1)
    pick = rng.random((H, W))
    frame[pick < 0.1] = 0
    one = (pick >= 0.1) & (pick < 0.15)
    frame[one] /= F(5)
    frame[(pick >= 0.15) & (pick < 0.17), 3] = -3
    frame[(pick >= 0.17) & (pick < 0.19), 3] = np.nan
    frame[(pick >= 0.19) & (pick < 0.22), 0] = np.inf
    frame[(pick >= 0.22) & (pick < 0.24), 1] = np.nan
    moments[(pick >= 0.24) & (pick < 0.27), 2] = np.inf
    moments[(pick >= 0.27) & (pick < 0.30), 0] = np.nan  # (e = NaN is clamped to 0 by `e > 0 ? e : 0`: counted)
    frame[(pick >= 0.30) & (pick < 0.32), :3] = 1e25      # l * l overflows
    return frame, moments


def luminance_rel_l2(frame, truth):
    """the actual relative L2 distance of the frame's luminance image from the noise-free one, in binary64"""
    c = frame[..., :3].astype(np.float64) / frame[..., 3:4]
    w = np.array([0.2126, 0.7152, 0.0722])
    return float(np.linalg.norm((c @ w - truth.astype(np.float64) @ w).ravel()) / np.linalg.norm((truth.astype(np.float64) @ w).ravel()))


def params(window=(0, 0, 0, 0)):
    p = metric.default_params()
    p.window[:] = window
    return p


def same_result(got, want, what, skip=()):
    """two results (Engine.metric_compare's dict, metric.reference_compare's) agree in every field, the floats to the bit"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        if k in skip:
            continue
        g, w = got[k], want[k]
        if k == "max_abs":
            assert F(g).tobytes() == F(w).tobytes(), (what, k, got, want)
        elif isinstance(w, float):
            assert np.float64(g).tobytes() == np.float64(w).tobytes(), (what, k, got, want)
        else:
            assert int(g) == int(w), (what, k, got, want)


def same_bins(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint64 and got.tobytes() == want.tobytes(), (what, np.nonzero(got != want)[0][:8], got.sum(), want.sum())

