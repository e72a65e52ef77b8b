"""The convergence metric (include/hrcore_metric.h) restated in numpy, operation for operation — `reference_compare` and
`reference_estimate` give the bits, the counts and the bins the device kernel (heatray_amd/csrc/hr_metric.h) gives.

    r = eng.metric_compare(reference_ptr)                 # the frame against a kept copy of a converged frame: r["value"]
    r = eng.metric_estimate()                             # no reference: what the sample moments predict
    want, num_bins, den_bins = metric.reference_compare(eng.readback(), reference_frame)

The float lines are one binary32 operation each.  A term is never added as a float: its 24-bit mantissa goes into the uint64 bin of its
exponent, so the bins hold the exact sum in any order, and `fold` rounds that sum once, to binary64.
"""
import math

import numpy as np

from . import _ffi as ffi
from .denoise import lum

F = np.float32
BINS = ffi.HR_METRIC_BINS
COMPARE, ESTIMATE = ffi.HR_METRIC_COMPARE, ffi.HR_METRIC_ESTIMATE
EMPTY, ZERO_DENOMINATOR = ffi.HR_METRIC_EMPTY, ffi.HR_METRIC_ZERO_DENOMINATOR


def default_params():
    """hr_metric_default_params: the whole image."""
    return ffi.MetricParams()


def _window(image, params):
    img = np.ascontiguousarray(image, F)
    if params is not None and any(params.window):
        x0, y0, x1, y1 = (int(v) for v in params.window)
        img = img[y0:y1, x0:x1]
    return img.reshape(-1, 4)


def _finite(t):
    return (np.ascontiguousarray(t, F).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def _normalised(px):
    a = px[:, 3:4]
    has = a > 0
    return np.where(has, px[:, :3] / np.where(has, a, F(1)), F(0)).astype(F)


def terms_compare(image, reference, params=None):
    """hr_metric.h's mtCompare over the window of two H x W x 4 accumulation-format images: {"x", "y": N x 3 float32 (every pixel of
    the window, row-major), "counted", "nonfinite", "differing": N bools, "max_abs_bits": N uint32}"""
    I, R = _window(image, params), _window(reference, params)
    with np.errstate(all="ignore"):
        cI, cR = _normalised(I), _normalised(R)
        d = cI - cR
        x, y = d * d, cR * cR
    finite = _finite(x).all(axis=1) & _finite(y).all(axis=1)
    abs_bits = (np.ascontiguousarray(d, F).view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1)
    return {"x": x, "y": y, "counted": finite, "nonfinite": ~finite, "differing": finite & (d != 0).any(axis=1), "max_abs_bits": abs_bits}


def terms_estimate(frame, moments, params=None):
    """hr_metric.h's mtEstimate over the window of the frame and its MOMENTS plane: {"x", "y": N float32, "counted", "nonfinite",
    "skipped": N bools}"""
    Fr, M = _window(frame, params), _window(moments, params)
    n = Fr[:, 3]
    with np.errstate(all="ignore"):
        ok = n >= 2
        c = Fr[:, :3] / n[:, None]
        e = M[:, :3] - (n[:, None] * c) * c
        e = np.where(e > 0, e, F(0)).astype(F)
        vc = (e / (n[:, None] - F(1))) / n[:, None]
        l = lum(c[:, 0], c[:, 1], c[:, 2])
        x, y = np.ascontiguousarray(lum(vc[:, 0], vc[:, 1], vc[:, 2]), F), np.ascontiguousarray(l * l, F)
    finite = _finite(x) & _finite(y)
    return {"x": x, "y": y, "counted": ok & finite, "nonfinite": ok & ~finite, "skipped": ~ok}


def bins(terms):
    """finite non-negative float32 terms -> their 256 uint64 bins: bins[b >> 23] += (b & 0x7fffff) | (b >> 23 ? 0x800000 : 0)"""
    b = np.ascontiguousarray(terms, F).reshape(-1).view(np.uint32)
    e = b >> np.uint32(23)
    assert (e < 255).all(), "a term is finite and has no sign bit"
    m = (b & np.uint32(0x7FFFFF)) | np.where(e != 0, np.uint32(0x800000), np.uint32(0))
    out = np.zeros(BINS, np.uint64)
    np.add.at(out, e, m.astype(np.uint64))
    return out


def fold(b):
    """the exact sum the bins hold, rounded once to binary64: S = sum of bins[e] * 2^(max(e, 1) - 1) in units of 2^-149 (Python integers;
    int / int is correctly rounded)"""
    S = sum(int(v) << (max(e, 1) - 1) for e, v in enumerate(b))
    return S / (1 << 149)


def finish(kind, num_bins, den_bins, counted, differing=0, nonfinite=0, skipped=0, max_abs=0.0, passes=0):
    """the result Engine.metric_compare / metric_estimate return, from the bins and the counts"""
    num, den = fold(num_bins), fold(den_bins)
    flags = 0
    if den == 0.0:
        flags |= ZERO_DENOMINATOR
        value = 0.0 if num == 0.0 else math.inf
    else:
        value = math.sqrt(num / den)
    if counted == 0:
        flags |= EMPTY
        value = mse = 0.0
    else:
        mse = num / float(3 * counted if kind == COMPARE else counted)
    return {"num": num, "den": den, "value": value, "mse": mse, "counted": int(counted), "differing": int(differing), "nonfinite": int(nonfinite),
            "skipped": int(skipped), "max_abs": float(max_abs), "passes": int(passes), "kind": kind, "flags": flags}


def reference_compare(image, reference, params=None, passes=0):
    """What hr_metric_compare answers for these images: (the result as Engine.metric_compare's dict, the bins of num, the bins of den)."""
    t = terms_compare(image, reference, params)
    k = t["counted"]
    nb, db = bins(t["x"][k]), bins(t["y"][k])
    max_bits = np.array([t["max_abs_bits"][k].max() if k.any() else 0], np.uint32)
    return finish(COMPARE, nb, db, k.sum(), differing=t["differing"].sum(), nonfinite=t["nonfinite"].sum(), max_abs=max_bits.view(F)[0], passes=passes), nb, db


def reference_estimate(frame, moments, params=None, passes=0):
    """What hr_metric_estimate answers for this frame and its MOMENTS plane: (the result dict, the bins of num, the bins of den)."""
    t = terms_estimate(frame, moments, params)
    k = t["counted"]
    nb, db = bins(t["x"][k]), bins(t["y"][k])
    return finish(ESTIMATE, nb, db, k.sum(), nonfinite=t["nonfinite"].sum(), skipped=t["skipped"].sum(), passes=passes), nb, db
