"""Frames for the tests of firefly suppression (tests/test_despeckle_ref.py without a GPU, tests/test_gpu_despeckle.py on one): a noisy
frame with injected fireflies whose truth is known, the planted classes, and parameter sets."""
import numpy as np

from heatray_amd import despeckle

F = np.float32
FLAT = (0.5, 0.25, 0.125)


def params(rank=2, min_taps=8, ratio=2.0, sigmas=3.0, floor=0.0):
    p = despeckle.default_params()
    p.rank, p.min_taps, p.ratio, p.sigmas, p.floor = rank, min_taps, ratio, sigmas, floor
    return p


def base_colour(W, H):
    """a smooth base colour, H x W x 3"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = x / max(W, 2), y / max(H, 2)
    return np.stack([0.3 + 0.5 * u, 0.6 - 0.3 * v, 0.2 + 0.3 * u * v], -1)


def speckled(W, H, n, seed, rate=0.002, gain=200):
    """(frame, moments, injected, truth): n passes of gamma(2, 0.5) noise per channel (mean 1) around base_colour; in every pass a share
    `rate` of the pixels has its sample multiplied by `gain`.  injected: the pixels that got such a sample in some pass; truth: the
    mean the samples converge to, injected energy included, base * (1 + rate * (gain - 1))."""
    rng = np.random.default_rng(seed)
    base = base_colour(W, H)
    frame, mom = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    injected = np.zeros((H, W), bool)
    for _ in range(n):
        s = (base * rng.gamma(2.0, 0.5, (H, W, 3))).astype(F)
        hot = rng.random((H, W)) < rate
        s = np.where(hot[..., None], s * F(gain), s).astype(F)
        injected |= hot
        frame[..., :3] += s
        frame[..., 3] += F(1)
        mom[..., :3] += s * s
        mom[..., 3] += F(1)
    return frame, mom, injected, (base * (1 + rate * (gain - 1))).astype(F)


def flat(W, H, n, colour=FLAT):
    """n samples of one colour everywhere: zero variance"""
    c = np.asarray(colour, F)
    frame, mom = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    frame[..., :3], frame[..., 3] = c * F(n), n
    mom[..., :3], mom[..., 3] = (c * c) * F(n), n
    return frame, mom


def with_spot(W, H, n, x, y, value=8.0):
    """flat(), and n samples of the colour (value, value, value) at (x, y): a bright pixel whose samples agree"""
    frame, mom = flat(W, H, n)
    frame[y, x, :3], mom[y, x, :3] = F(value) * F(n), F(value) * F(value) * F(n)
    return frame, mom


def plant_classes(frame, mom, seed):
    """holes, NaN and +inf in F, NaN and +inf in M, at seeded places (at most one kind per pixel); returns the masks by kind"""
    rng = np.random.default_rng(seed)
    H, W = frame.shape[:2]
    u = rng.random((H, W))
    kinds = {"hole": u < 0.06, "nan_f": (u >= 0.06) & (u < 0.08), "inf_f": (u >= 0.08) & (u < 0.10), "nan_m": (u >= 0.10) & (u < 0.12),
             "inf_m": (u >= 0.12) & (u < 0.14), "inf_n": (u >= 0.14) & (u < 0.15)}
    frame[kinds["hole"]], mom[kinds["hole"]] = 0, 0
    frame[kinds["nan_f"], 1] = np.nan
    frame[kinds["inf_f"], 0] = np.inf
    mom[kinds["nan_m"], 2] = np.nan
    mom[kinds["inf_m"], 0] = np.inf
    frame[kinds["inf_n"], 3] = np.inf
    return kinds


def fireflies_at(frame, mom, places, gain=500.0):
    """one more sample, `gain` times the pixel's mean, at each (x, y) of places that lies inside the frame"""
    H, W = frame.shape[:2]
    for x, y in places:
        if 0 <= x < W and 0 <= y < H and frame[y, x, 3] > 0 and np.isfinite(frame[y, x]).all():
            s = (frame[y, x, :3] / frame[y, x, 3] * F(gain)).astype(F)
            frame[y, x, :3] += s
            mom[y, x, :3] += s * s
            frame[y, x, 3] += F(1)
            mom[y, x, 3] += F(1)


def border_places(W, H):
    """every corner, the middle of every edge, and both sides of the workgroup boundaries at x = 15 | 16 and y = 15 | 16"""
    xs, ys = (0, W // 2, W - 1), (0, H // 2, H - 1)
    places = [(x, y) for x in xs for y in ys if x in (0, W - 1) or y in (0, H - 1)]
    places += [(15, H // 2), (16, H // 2), (15, 0), (16, H - 1), (W // 2, 15), (W // 2, 16), (15, 15), (16, 16), (15, 16), (16, 15)]
    return sorted(set(places))


def same_counters(got, want, what):
    keys = ("valid_pixels", "clamped_pixels", "kept_pixels", "starved_pixels", "nonfinite_pixels")
    assert {k: int(got[k]) for k in keys} == {k: int(want[k]) for k in keys}, (what, got, want)
