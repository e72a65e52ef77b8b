"""Adaptive sampling (include/hrcore_adaptive.h): the error estimate and the sample mask restated in numpy float32, operation for
operation — `reference_error` and `reference_mask` give the bits the device kernels (heatray_amd/csrc/hr_adaptive.h) give — and a small
driver that renders with the mask rebuilt every few batches.

    eng.set_aovs(HR_AOV_MOMENTS); eng.clear()
    out = adaptive.render(eng, scene.options, max_passes=1024)   # stops when no pixel is left to sample
    out["paths"], out["passes"], out["updates"]

The known limit (the header has the figures): the decision is made from the samples it is about to average, so a pixel whose variance
is under-estimated stops early; min_samples and the dilation (keep radius >= 1) are the guards, not a proof.
"""
import numpy as np

from . import _ffi as ffi
from .denoise import _fmax, lum

F = np.float32


def default_params():
    """hr_adaptive_default_params: threshold 0.02 (= convergence.THRESHOLD), floor 0.05, min_samples 16, radius 2."""
    return ffi.AdaptiveParams(0.02, 0.05, 16, 2)


def reference_error(frame, moments, params=None):
    """The error map (H x W float32) of a frame (Engine.readback) and its MOMENTS plane: hr_adaptive.h's adError per pixel."""
    p = params if params is not None else default_params()
    Fr, M = np.ascontiguousarray(frame, F), np.ascontiguousarray(moments, F)
    with np.errstate(all="ignore"):
        n = Fr[..., 3]
        c = Fr[..., :3] / n[..., None]
        e = M[..., :3] - (n[..., None] * c) * c
        e = np.where(e > 0, e, F(0.0)).astype(F)
        vc = (e / (n - F(1.0))[..., None]) / n[..., None]
        v = lum(vc[..., 0], vc[..., 1], vc[..., 2])
        err = np.sqrt(v) / _fmax(lum(c[..., 0], c[..., 1], c[..., 2]), F(p.floor))
        err = np.where(~(n > 0) | (n < F(p.min_samples)), F(np.inf), err)
    return err.astype(F)


def unconverged(error, params=None):
    """error > threshold (a NaN error is not)"""
    p = params if params is not None else default_params()
    with np.errstate(invalid="ignore"):
        return np.asarray(error, F) > F(p.threshold)


def reference_mask(error, params=None):
    """The sample mask (H x W uint8, 0 / 1) built from an error map: an unconverged pixel keeps the (2 radius + 1)^2 pixels around it
    (inside the image) sampled."""
    p = params if params is not None else default_params()
    u = unconverged(error, p)
    H, W = u.shape
    r = int(p.radius)
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = u
    out = np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return out.astype(np.uint8)


def reference_result(error, params=None, passes=0):
    """What hr_adaptive_update reports for that error map: {"unconverged_pixels", "active_pixels", "max_error", "passes"}."""
    p = params if params is not None else default_params()
    err = np.asarray(error, F)
    finite = err[np.isfinite(err)]
    return {"unconverged_pixels": int(unconverged(err, p).sum()), "active_pixels": int(reference_mask(err, p).sum()),
            "max_error": float(finite.max()) if finite.size else 0.0, "passes": int(passes)}


def render(eng, options, max_passes, params=None, every=None, first_pass=0, on_update=None):
    """Render up to max_passes passes of `options` (a scenes.RenderOptions), rebuilding the sample mask every `every` passes, and stop when
    no pixel is left to sample.  `every` defaults to four of the engine's pass batches: an update completes the passes in flight, so it
    should not follow every batch.  The engine needs HR_AOV_MOMENTS enabled before the frame's first pass.  on_update(passes, result),
    when given, is called after every update and may return True to stop.  Returns {"passes": passes requested, "paths": camera paths
    traced (eng.stats().paths), "updates": [(passes so far, AdaptiveResult as a dict)]}."""
    if every is None:
        every = 4 * max(1, eng.pass_batch(options.pass_params(first_pass).max_ray_depth))
    every = max(1, int(every))
    done, updates = 0, []
    while done < max_passes:
        n = min(every, max_passes - done)
        for s in range(done, done + n):
            eng.render_pass(options.pass_params(first_pass + s))
        done += n
        r = eng.adaptive_update(params, install=True).as_dict()
        updates.append((done, r))
        stop = on_update(done, r) if on_update is not None else False
        if r["active_pixels"] == 0 or stop:
            break
    return {"passes": done, "paths": int(eng.stats().paths), "updates": updates}
