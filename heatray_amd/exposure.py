"""Auto-exposure (include/hrcore_exposure.h): the luminance histogram, its percentile-trimmed average and the exposure scale restated
in numpy, operation for operation — `reference` gives the bits and the counts the device kernels (heatray_amd/csrc/hr_exposure.h) give.

    r = eng.exposure_meter()                         # the frame; or image=<device pointer of a W x H float4 image>
    eng.exposure_display(out_ptr, display)           # metered and shown at the metered scale, no host round trip
    want, bins, state = exposure.reference(eng.readback())

The float lines are one binary32 operation each; the histogram's position is integer arithmetic on the luminance's bits (a piecewise-
linear log2, 8 bins per octave from 2^-16 to 2^16), so a power-of-two change of the image moves `position` by 4096 per octave and
nothing else.
"""
import math

import numpy as np

from . import _ffi as ffi
from .denoise import lum

F = np.float32
BINS = ffi.HR_EXPOSURE_BINS
EMPTY, CLAMPED_LOW, CLAMPED_HIGH, ADAPTED = ffi.HR_EXPOSURE_EMPTY, ffi.HR_EXPOSURE_CLAMPED_LOW, ffi.HR_EXPOSURE_CLAMPED_HIGH, ffi.HR_EXPOSURE_ADAPTED


def default_params():
    """hr_exposure_default_params: key 0.18, percentiles 100 .. 950 permille, scale within 1/256 .. 256, adapt 1 (no memory), the
    whole image."""
    return ffi.ExposureParams(0.18, 100, 950, 1.0 / 256.0, 256.0, 1.0)


def adapt_rate(dt, tau):
    """The `adapt` of a caller with a clock: the share of the way to the target covered in dt at time constant tau, 1 - exp(-dt / tau)."""
    return 1.0 if tau <= 0 else 1.0 - math.exp(-dt / tau)


def apply(image, scale):
    """The image the metered display shows: rgb times scale (one binary32 multiply per channel), alpha untouched."""
    out = np.array(image, F)
    out[..., :3] = out[..., :3] * F(scale)
    return out


def classify(image, params=None):
    """(the 256 bins as uint64, {"below", "above", "nonfinite", "invalid"}) of the window of an H x W x 4 accumulation-format image:
    hr_exposure.h's exClass per pixel."""
    p = params if params is not None else default_params()
    img = np.ascontiguousarray(image, F)
    x0, y0, x1, y1 = (int(v) for v in p.window)
    if (x0, y0, x1, y1) != (0, 0, 0, 0):
        img = img[y0:y1, x0:x1]
    a = img[..., 3]
    with np.errstate(all="ignore"):
        valid = a > 0
        c = img[..., :3] / a[..., None]
        L = np.ascontiguousarray(lum(c[..., 0], c[..., 1], c[..., 2]), F)
    b = L.view(np.uint32)
    nonfinite = valid & ((b & np.uint32(0x7F800000)) == np.uint32(0x7F800000))
    rest = valid & ~nonfinite
    negative = rest & ((b >> np.uint32(31)) != 0)
    k = (b >> np.uint32(20)).astype(np.int64) - 888
    binned = rest & ~negative & (k >= 0) & (k <= 255)
    counts = {"below": int((negative | (rest & ~negative & (k < 0))).sum()), "above": int((rest & ~negative & (k > 255)).sum()),
              "nonfinite": int(nonfinite.sum()), "invalid": int((~valid).sum())}
    return np.bincount(k[binned], minlength=BINS).astype(np.uint64), counts


def luminance_at(q):
    """The luminance at position q (1/4096 octave above 2^-16): the inverse of the bins' map."""
    return np.array([(((q >> 12) - 16 + 127) << 23) | ((q & 4095) << 11)], np.uint32).view(F)[0]


def reduce(bins, params=None, state=None):
    """hr_exposure.h's exReduce: the ordered pass over the bins.  state: the adaptation state's scale, None = there is none.  Returns
    ({"scale", "target", "key_luminance", "position", "counted", "used", "flags"}, the state after)."""
    p = params if params is not None else default_params()
    hist = [int(v) for v in bins]
    N = sum(hist)
    if N == 0:
        s = F(state) if state is not None else F(1.0)
        return {"scale": float(s), "target": float(s), "key_luminance": 0.0, "position": 0, "counted": 0, "used": 0, "flags": EMPTY}, state
    lo, hi = N * int(p.low_permille) // 1000, N * int(p.high_permille) // 1000
    if hi <= lo:
        hi = lo + 1
    C = T = 0
    for k, h in enumerate(hist):
        T += max(0, min(C + h, hi) - max(C, lo)) * (2 * k + 1)
        C += h
    U = hi - lo
    q = (T << 8) // U
    lavg = luminance_at(q)
    flags = 0
    with np.errstate(all="ignore"):
        t = F(p.key) / lavg
        floored = F(p.min_scale) if t < F(p.min_scale) else t  # fmax_(t, min_scale)
        target = F(p.max_scale) if F(p.max_scale) < floored else floored  # fmin_(.., max_scale)
        if t < F(p.min_scale):
            flags |= CLAMPED_LOW
        if F(p.max_scale) < floored:
            flags |= CLAMPED_HIGH
        if state is not None and F(p.adapt) < F(1.0):
            prev = F(state)
            scale = F(prev + F(F(target - prev) * F(p.adapt)))
            flags |= ADAPTED
        else:
            scale = target
    return {"scale": float(scale), "target": float(target), "key_luminance": float(lavg), "position": int(q), "counted": N, "used": U, "flags": flags}, F(scale)


def reference(image, params=None, state=None):
    """What hr_exposure_meter answers for this image: (the result as Engine.exposure_meter's dict, the 256 bins as uint64, the
    adaptation state after: a float32 scale or None).  state: the state before (None: none, as after exposure_reset)."""
    bins, counts = classify(image, params)
    res, new_state = reduce(bins, params, state)
    res.update(counts)
    return res, bins, new_state
