"""The arithmetic of the convergence metric without a GPU: heatray_amd/csrc/hr_metric.h compiled for the CPU (tests/host/metric_cpu.cpp,
plain and once more under AddressSanitizer + UBSan) against its numpy restatement heatray_amd.metric.reference_compare /
reference_estimate, byte for byte, on seeded images and on hand-made inputs whose answers are known (include/hrcore_metric.h is the
contract).  tests/test_gpu_metric.py holds the device to the same reference."""
import math

import numpy as np
import pytest

import cpu_header
from heatray_amd import convergence, metric
from metric_frames import (CLASS_PIXELS, F, SIZES, all_bins_pair, bin_value, class_rows, constant_difference, estimate_frame, estimate_with_classes,
                           luminance_rel_l2, params, same_bins, same_result, seeded_pair, windows)

WORDS = 517  # hr_metric.h's kMtWords: 2 x 256 bins, four counters, the bits of max_abs


def _runner(exe):
    def run(mode, a=None, b=None, p=None, bins=None, counted=0, kind=metric.COMPARE):
        """(the result dict, the bins of num, the bins of den) from the header's host build: mode 0 compare(a, b), 1 estimate(a, b),
        2 the fold of `bins` (512 uint64)"""
        H, W = a.shape[:2] if a is not None else (0, 0)
        head = np.array([mode, W, H, *(p.window if p is not None else (0, 0, 0, 0))], np.int32)
        if mode == 2:
            payload = np.asarray(bins, np.uint64).tobytes() + np.array([counted, kind], np.uint64).tobytes()
        else:
            payload = np.ascontiguousarray(a, F).tobytes() + np.ascontiguousarray(b, F).tobytes()
        raw = cpu_header.run(exe, head.tobytes() + payload)
        assert len(raw) == WORDS * 8 + 4 * 8 + 4
        words = np.frombuffer(raw[:WORDS * 8], np.uint64)
        num, den, value, mse = (float(v) for v in np.frombuffer(raw[WORDS * 8:WORDS * 8 + 32], np.float64))
        flags = int(np.frombuffer(raw[-4:], np.uint32)[0])
        res = {"num": num, "den": den, "value": value, "mse": mse, "counted": int(words[512]), "differing": int(words[513]), "nonfinite": int(words[514]),
               "skipped": int(words[515]), "max_abs": float(np.array([words[516]], np.uint32).view(F)[0]), "passes": 0,
               "kind": metric.ESTIMATE if mode == 1 else kind, "flags": flags}
        return res, words[:256].copy(), words[256:512].copy()
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cpu(request, tmp_path_factory):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _runner(cpu_header.build("metric", tmp_path_factory.mktemp("metric_" + request.param), flags=flags))


def _window_pixels(p, W, H):
    x0, y0, x1, y1 = p.window
    return (x1 - x0) * (y1 - y0) if any(p.window) else W * H


def _check_compare(cpu, img, ref, p, what):
    want, want_num, want_den = metric.reference_compare(img, ref, p)
    got, got_num, got_den = cpu(0, img, ref, p)
    same_bins(got_num, want_num, what + ": num bins")
    same_bins(got_den, want_den, what + ": den bins")
    same_result(got, want, what)
    H, W = img.shape[:2]
    assert want["counted"] + want["nonfinite"] == _window_pixels(p, W, H) and want["skipped"] == 0, (what, want)  # every pixel is in one class
    assert want_num[255] == 0 and want_den[255] == 0
    return want, want_num, want_den


def _check_estimate(cpu, frame, moments, p, what):
    want, want_num, want_den = metric.reference_estimate(frame, moments, p)
    got, got_num, got_den = cpu(1, frame, moments, p)
    same_bins(got_num, want_num, what + ": num bins")
    same_bins(got_den, want_den, what + ": den bins")
    same_result(got, want, what)
    H, W = frame.shape[:2]
    assert want["counted"] + want["nonfinite"] + want["skipped"] == _window_pixels(p, W, H), (what, want)
    assert want["differing"] == 0 and want["max_abs"] == 0.0
    return want, want_num, want_den


def _check_fold(cpu, num_bins, den_bins, counted, kind=metric.COMPARE):
    want = metric.finish(kind, num_bins, den_bins, counted)
    got, _, _ = cpu(2, bins=np.concatenate([np.asarray(num_bins, np.uint64), np.asarray(den_bins, np.uint64)]), counted=counted, kind=kind)
    same_result(got, want, "fold")
    return want


def _one_bin(e, v):
    b = np.zeros(256, np.uint64)
    b[e] = v
    return b


def _exact(b):
    """the exact sum the bins hold, as a Fraction-free pair: (integer, in units of 2^-149)"""
    return sum(int(v) << (max(e, 1) - 1) for e, v in enumerate(b))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cpu_header_equals_numpy_reference_byte_for_byte(cpu, size):
    W, H = size
    img, ref = seeded_pair(W, H, seed=W * 1000 + H)
    frame, moments = estimate_with_classes(W, H, seed=W * 1000 + H)
    for name, win in windows(W, H).items():
        _check_compare(cpu, img, ref, params(win), f"compare {W}x{H} {name}")
        _check_estimate(cpu, frame, moments, params(win), f"estimate {W}x{H} {name}")
    if W * H > 100:  # (the whole image: the inputs exercise every class)
        whole, _, _ = metric.reference_compare(img, ref)
        assert whole["counted"] > 0 and whole["nonfinite"] > 0 and 0 < whole["differing"] < whole["counted"], whole
        whole, _, _ = metric.reference_estimate(frame, moments)
        assert whole["counted"] > 0 and whole["nonfinite"] > 0 and whole["skipped"] > 0, whole


def test_identical_images_give_zero(cpu):
    img, _ = seeded_pair(67, 35, seed=1, classes=False)
    want, num, _ = _check_compare(cpu, img, img.copy(), params(), "identical")
    assert want["num"] == 0.0 and want["differing"] == 0 and want["value"] == 0.0 and want["mse"] == 0.0 and want["max_abs"] == 0.0 and not num.any()
    assert want["counted"] == 67 * 35 and want["den"] > 0 and want["flags"] == 0


def test_a_constant_difference_fills_one_bin(cpu):
    W, H = 67, 35
    N = W * H
    img, ref = constant_difference(W, H)
    want, num, den = _check_compare(cpu, img, ref, params(), "constant difference")
    assert num[127 - 6] == 3 * N * 2 ** 23 and np.count_nonzero(num) == 1  # x = 2^-6: exponent field 121, mantissa 2^23
    assert den[127 - 2] == 3 * N * 2 ** 23 and np.count_nonzero(den) == 1  # y = 2^-2
    assert want["num"] == 3 * N / 64 and want["den"] == 3 * N / 4 and want["value"] == 0.25 and want["mse"] == 1 / 64
    assert want["differing"] == N and want["max_abs"] == 0.125


def test_terms_in_every_exponent_bin_fold_to_fsum(cpu):
    img, ref = all_bins_pair(256, 4)
    want, num, den = _check_compare(cpu, img, ref, params(), "all bins")
    assert (num[:255] > 0).all() and (den[:255] > 0).all() and num[255] == 0
    t = metric.terms_compare(img, ref)
    assert t["counted"].all() and t["x"].min() > 0 and t["x"].min() < 2.0 ** -126  # denormal squares included
    assert want["num"] == math.fsum(t["x"].astype(np.float64).ravel()) and want["den"] == math.fsum(t["y"].astype(np.float64).ravel())
    # one term per bin, by hand: bin e holds the term's mantissa
    d = np.array([bin_value(e) for e in range(255)], F)
    x = d * d
    b = metric.bins(x)
    assert (np.nonzero(b)[0] == np.arange(255)).all() and metric.fold(b) == math.fsum(x.astype(np.float64))


def test_the_fold_carries_across_its_words_and_rounds_ties_to_even(cpu):
    zero = np.zeros(256, np.uint64)
    # bins of 2^63 in neighbouring exponents: every add carries into the next limb
    for e0 in (1, 31, 32, 33, 63, 64, 65, 127, 190, 251):
        b = np.zeros(256, np.uint64)
        b[e0:e0 + 4] = 1 << 63
        want = _check_fold(cpu, b, zero, 1)
        assert want["num"] == math.ldexp(15.0, 63 + e0 - 1 - 149)
    full = np.full(256, (1 << 64) - 1, np.uint64)
    full[255] = 0
    want = _check_fold(cpu, full, full, 7)
    assert want["num"] == _exact(full) / (1 << 149) and want["value"] == 1.0
    # ties at the 53rd bit, hand-made: bin 1 holds units of 2^-149
    tie_even, tie_odd = (1 << 53) + 1, (1 << 53) + 3  # 54-bit integers ending in 01 and 11: halfway cases
    assert _check_fold(cpu, _one_bin(1, tie_even), zero, 1)["num"] == math.ldexp(1 << 53, -149)              # down to even
    assert _check_fold(cpu, _one_bin(1, tie_odd), zero, 1)["num"] == math.ldexp((1 << 53) + 4, -149)         # up to even
    # the same ties broken by a sticky bit far below: bin 1 shifted up by 200 exponents, one unit in bin 0
    sticky = _one_bin(201, tie_even)
    assert _check_fold(cpu, sticky, zero, 1)["num"] == math.ldexp(1 << 53, 200 - 149)
    sticky[0] = 1
    assert _check_fold(cpu, sticky, zero, 1)["num"] == math.ldexp((1 << 53) + 2, 200 - 149)
    # a carry out of the rounding: 2^54 - 1 rounds to 2^54
    assert _check_fold(cpu, _one_bin(1, (1 << 54) - 1), zero, 1)["num"] == math.ldexp(1.0, 54 - 149)
    # bins 0 and 1 share a scale: a denormal's mantissa and a unit of the smallest normal exponent
    assert _check_fold(cpu, _one_bin(0, 5) + _one_bin(1, 7), zero, 1)["num"] == math.ldexp(12.0, -149)
    # exact below 2^53
    assert _check_fold(cpu, _one_bin(0, 1), _one_bin(0, 4), 1)["value"] == 0.5


def test_every_class_lands_where_the_contract_says(cpu):
    img, ref = class_rows()
    for i, (name, (_, _, cls, differing)) in enumerate(CLASS_PIXELS.items()):
        want, num, den = _check_compare(cpu, img, ref, params((i, 0, i + 1, 1)), name)
        assert want[cls] == 1 and want["differing"] == int(differing), (name, want)
        if cls == "nonfinite":  # the sums stay unchanged
            assert not num.any() and not den.any() and want["flags"] == metric.EMPTY | metric.ZERO_DENOMINATOR and want["value"] == 0.0, (name, want)
    want, _, _ = _check_compare(cpu, img, ref, params(), "the whole row")
    counted = sum(1 for p in CLASS_PIXELS.values() if p[2] == "counted")
    assert (want["counted"], want["nonfinite"]) == (counted, len(CLASS_PIXELS) - counted) and want["differing"] == sum(p[3] for p in CLASS_PIXELS.values())
    # a == 0 and a < 0 count as black: the image's pixel against (0.5 0.25 0.125)
    for name in ("a = 0 in the image", "a < 0 in the image"):
        i = list(CLASS_PIXELS).index(name)
        want, _, _ = _check_compare(cpu, img, ref, params((i, 0, i + 1, 1)), name)
        assert want["num"] == want["den"] == 0.25 + 0.0625 + 0.015625 and want["value"] == 1.0 and want["max_abs"] == 0.5
    # a square that underflows: differing, and nothing added
    i = list(CLASS_PIXELS).index("a difference whose square underflows to 0")
    want, num, _ = _check_compare(cpu, img, ref, params((i, 0, i + 1, 1)), "underflow")
    assert want["differing"] == 1 and not num.any() and want["max_abs"] == float(F(1e-30))
    i = list(CLASS_PIXELS).index("a tiny difference whose square is denormal")
    want, num, _ = _check_compare(cpu, img, ref, params((i, 0, i + 1, 1)), "denormal")
    assert num[0] > 0 and np.count_nonzero(num) == 1 and want["num"] == float(F(1e-20) * F(1e-20))


def test_nonfinite_pixels_leave_the_sums_unchanged(cpu):
    img, ref = seeded_pair(67, 35, seed=8, classes=False)
    base, num, den = _check_compare(cpu, img, ref, params(), "clean")
    assert base["nonfinite"] == 0
    img2, ref2 = img.copy(), ref.copy()
    img2[3, 5, 0], ref2[7, 9, 1], img2[11, 2, 2], ref2[20, 40, 0] = np.nan, np.inf, 1e30 * img2[11, 2, 3], -np.inf
    bad = np.zeros((35, 67), bool)
    bad[3, 5] = bad[7, 9] = bad[11, 2] = bad[20, 40] = True
    want, num2, den2 = _check_compare(cpu, img2, ref2, params(), "four bad pixels")
    assert want["nonfinite"] == 4 and want["counted"] == 67 * 35 - 4
    img3, ref3 = img.copy(), ref.copy()
    img3[bad], ref3[bad] = 0, 0  # black in both: x = y = 0, nothing added
    clean, num3, den3 = _check_compare(cpu, img3, ref3, params(), "the same pixels black")
    same_bins(num2, num3, "num")
    same_bins(den2, den3, "den")
    assert (want["num"], want["den"], want["value"]) == (clean["num"], clean["den"], clean["value"])


def test_empty_and_zero_denominator(cpu):
    nan = np.full((3, 5, 4), np.nan, F)
    nan[..., 3] = 1
    want, _, _ = _check_compare(cpu, nan, nan, params(), "all NaN")
    assert want["flags"] == metric.EMPTY | metric.ZERO_DENOMINATOR and want["counted"] == 0 and want["value"] == 0.0 and want["mse"] == 0.0
    black, grey = np.zeros((3, 5, 4), F), np.ones((3, 5, 4), F)
    want, _, _ = _check_compare(cpu, grey, black, params(), "a black reference")
    assert want["flags"] == metric.ZERO_DENOMINATOR and want["value"] == math.inf and want["num"] == 45.0 and want["mse"] == 1.0
    want, _, _ = _check_compare(cpu, black, black, params(), "both black")
    assert want["flags"] == metric.ZERO_DENOMINATOR and want["value"] == 0.0 and want["counted"] == 15
    want, _, _ = _check_estimate(cpu, black, black, params(), "an estimate without samples")
    assert want["flags"] == metric.EMPTY | metric.ZERO_DENOMINATOR and want["skipped"] == 15


def test_value_agrees_with_convergence_rel_l2():
    """Each term carries at most three binary32 roundings (the two divisions' share in d, the subtraction, the square) and sums of
    non-negative terms keep the relative bound, so the ratio under the root is within 2^-22 and `value` within 2^-23 = 1.2e-7 of the
    binary64 figure; 1e-6 is eight times that, to cover the final double roundings.  Ordinary magnitudes: no term underflows."""
    img, ref = seeded_pair(160, 90, seed=21, median=1.0, sigma=2.0, classes=False)
    want, _, _ = metric.reference_compare(img, ref)
    assert want["nonfinite"] == 0 and metric.terms_compare(img, ref)["y"].min() > 2.0 ** -100
    theirs = convergence.rel_l2(convergence.normalised(img), convergence.normalised(ref))
    print(f"value {want['value']!r}, convergence.rel_l2 {theirs!r}, relative difference {abs(want['value'] / theirs - 1):.3e}")
    assert abs(want["value"] / theirs - 1) <= 1e-6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_estimate_predicts_the_actual_error(seed):
    """64 x 64 pixels, 16 iid Gaussian samples each: the sampling standard deviation of estimate / actual is about 2.3 %, 15 % is more than
    five of them"""
    frame, moments, truth = estimate_frame(64, 64, seed)
    est, _, _ = metric.reference_estimate(frame, moments)
    actual = luminance_rel_l2(frame, truth)
    print(f"seed {seed}: estimate {est['value']:.6f}, actual {actual:.6f}, ratio {est['value'] / actual:.4f}")
    assert est["counted"] == 64 * 64 and est["flags"] == 0
    assert abs(est["value"] / actual - 1) <= 0.15


def test_the_estimate_is_aderrors_variance(cpu):
    """x / y per pixel is the square of hr_adaptive.h's adError where its floor does not engage (the same lines up to the square root):
    within a few binary32 roundings"""
    from heatray_amd import adaptive, _ffi as ffi
    frame, moments, _ = estimate_frame(32, 16, seed=4)
    t = metric.terms_estimate(frame, moments)
    err = adaptive.reference_error(frame, moments, ffi.AdaptiveParams(0.02, 1e-30, 2, 0))
    assert np.allclose(np.sqrt(t["x"].astype(np.float64) / t["y"]), np.asarray(err, np.float64).ravel(), rtol=1e-6)
    _check_estimate(cpu, frame, moments, params(), "a clean frame")


def test_default_params():
    p = metric.default_params()
    assert (list(p.window), list(p.reserved)) == ([0] * 4, [0] * 4)
