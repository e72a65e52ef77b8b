"""Firefly suppression of include/hrcore_despeckle.h restated in numpy float32, operation for operation: `reference(frame, moments,
params)` gives the bits the device kernel (heatray_amd/csrc/hr_despeckle.h) gives, both output planes and the five counters.  It is
the checker of the GPU tests and works without a GPU.

    eng.set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS); ... render ...
    img = eng.despeckle_denoise(spatial=True)                                     # on the device
    ref = despeckle.reference_denoise(eng.readback(), eng.aovs(), spatial=True)   # the same bits, on the host
"""
import numpy as np

from . import _ffi as ffi
from . import denoise, denoise_spatial
from .denoise import F, _fmax, _shift, lum

RADIUS = 2  # the window: 5 x 5 without its centre, 24 taps
NO_TAP = F(-np.inf)  # the luminance of a pixel that is nobody's tap


def default_params():
    """hr_despeckle_default_params: rank 2, min_taps 8, ratio 2, sigmas 3, floor 0."""
    return ffi.DespeckleParams(2, 8, 2.0, 3.0, 0.0)


def _check(p):
    if not 1 <= p.rank <= ffi.HR_DESPECKLE_RANK_HIGHEST:
        raise ValueError(f"rank = {p.rank} is outside 1 .. 4")
    if not p.rank <= p.min_taps <= ffi.HR_DESPECKLE_TAPS:
        raise ValueError(f"min_taps = {p.min_taps} is outside rank .. 24")
    for name, low in (("ratio", 1.0), ("sigmas", 0.0), ("floor", 0.0)):
        v = getattr(p, name)
        if not (np.isfinite(v) and v >= low):
            raise ValueError(f"{name} = {v} must be finite and at least {low}")
    if any(p.reserved):
        raise ValueError("reserved words must be 0")


def classify(frame):
    """-> (valid, nonfinite, l): the masks of the VALID and the NONFINITE pixels, and the luminance of every pixel's mean with NO_TAP
    wherever the pixel is not VALID (hr_despeckle.h's dkClass)"""
    Fr = np.ascontiguousarray(frame, F)
    with np.errstate(all="ignore"):
        n = Fr[..., 3]
        some = n > 0
        c = Fr[..., :3] / n[..., None]
        l = lum(c[..., 0], c[..., 1], c[..., 2]).astype(F)
        finite = (np.abs(l) <= np.finfo(F).max) & (np.abs(n) <= np.finfo(F).max)
    valid = some & finite
    return valid, some & ~finite, np.where(valid, l, NO_TAP).astype(F)


def reference(frame, moments, params=None, with_classes=False):
    """(out, moments_out, result dict) of a frame (Engine.readback) and its MOMENTS plane (Engine.aovs()["moments"]): the bits
    hr_despeckle gives.  with_classes: a fourth value, the masks {"valid", "clamped", "kept", "starved", "nonfinite"}."""
    p = params if params is not None else default_params()
    _check(p)
    Fr, M = np.ascontiguousarray(frame, F), np.ascontiguousarray(moments, F)
    assert Fr.shape == M.shape and Fr.ndim == 3 and Fr.shape[2] == 4
    valid, nonfinite, l = classify(Fr)
    with np.errstate(all="ignore"):
        t = [np.full(l.shape, NO_TAP, F) for _ in range(4)]  # the four largest tap luminances so far, in order
        K = np.zeros(l.shape, np.int32)
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                if dx == 0 and dy == 0:
                    continue
                lq, ok = _shift(l, dy, dx)
                v = np.where(ok, lq, NO_TAP).astype(F)
                K = np.where(v > NO_TAP, K + 1, K)
                for k in range(4):  # v takes the place of the first it is greater than; the displaced one moves down
                    up = v > t[k]
                    t[k], v = np.where(up, v, t[k]).astype(F), np.where(up, t[k], v).astype(F)
        starved = valid & (K < int(p.min_taps))
        R = t[int(p.rank) - 1]
        T = _fmax(F(p.ratio) * R + F(p.floor), F(0.0))
        ex = (l - T).astype(F)
        over = valid & ~starved & (ex > 0)
        n = Fr[..., 3]
        c = Fr[..., :3] / n[..., None]
        e = M[..., :3] - (n[..., None] * c) * c
        e = np.where(e > 0, e, F(0.0)).astype(F)
        vc = (e / (n - F(1.0))[..., None]) / n[..., None]
        v = lum(vc[..., 0], vc[..., 1], vc[..., 2]).astype(F)
        kept = over & (n >= F(2.0)) & (ex * ex > (F(p.sigmas) * F(p.sigmas)) * v)
        clamped = over & ~kept
        s = (T / l).astype(F)
        s2 = (s * s).astype(F)
        out, mout = Fr.copy(), M.copy()  # (every pixel that is not written below: a copy, bit for bit)
        out[clamped, :3] = (Fr[..., :3] * s[..., None]).astype(F)[clamped]
        mout[clamped, :3] = (M[..., :3] * s2[..., None]).astype(F)[clamped]
        out[nonfinite], mout[nonfinite] = F(0.0), F(0.0)
    result = {"valid_pixels": int(valid.sum()), "clamped_pixels": int(clamped.sum()), "kept_pixels": int(kept.sum()), "starved_pixels": int(starved.sum()),
              "nonfinite_pixels": int(nonfinite.sum())}
    if with_classes:
        return out, mout, result, {"valid": valid, "clamped": clamped, "kept": kept, "starved": starved, "nonfinite": nonfinite}
    return out, mout, result


def reference_denoise(frame, planes, params=None, dparams=None, spatial=False, sparams=None, with_result=False):
    """denoise.reference (spatial: denoise_spatial.reference) over the despeckled frame and moments, ALBEDO and NORMAL_DEPTH as they
    are: the bits hr_despeckle_denoise gives.  with_result: (image, the despeckle's result dict)."""
    out, mout, result = reference(frame, planes["moments"], params)
    clean = {"albedo": planes["albedo"], "normal_depth": planes["normal_depth"], "moments": mout}
    img = denoise_spatial.reference(out, clean, dparams, sparams) if spatial else denoise.reference(out, clean, dparams)
    return (img, result) if with_result else img
