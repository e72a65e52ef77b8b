"""AOV sums (include/hrcore_aov.h, Engine.aovs()) -> per-pixel means and the variance of the frame's mean.

The planes hold sums over passes: the first visible surface's albedo, shading normal and camera-space depth, summed over the passes
that recorded a surface (the count is ALBEDO.a), and the sum of the squared samples with the number of samples (MOMENTS.a).  Pixels
without a surface or with too few samples get 0 instead of a division by zero.
"""
import numpy as np


def _div(num, den):
    den = np.asarray(den, dtype=np.float64)
    safe = np.where(den > 0, den, 1.0)
    return np.where(den > 0, num / safe, 0.0)


def resolve(aovs, frame=None):
    """aovs: the dict Engine.aovs() returns; frame: the accumulation buffer read back with the planes (needed for the variance).

    Returns a dict of float32 arrays (H x W [x 3]), each present when its planes are:
      hits      passes that recorded a first visible surface
      coverage  hits / passes (the fraction of passes whose camera path met a surface)
      albedo    mean base colour of the surface (0 where hits == 0)
      normal    mean shading normal, renormalised (0 where hits == 0 or the mean vanishes)
      depth     mean camera-space depth (0 where hits == 0)
      samples   samples summed into the frame (MOMENTS.a)
      variance  per channel, the variance of the frame's mean estimate: s^2 / n with the unbiased sample variance
                s^2 = (sum s^2 - n mean^2) / (n - 1), clamped at 0 (0 where n < 2)
    Means are formed in float64 and returned as float32.
    """
    out = {}
    if "albedo" in aovs:
        alb = aovs["albedo"].astype(np.float64)
        nd = aovs["normal_depth"].astype(np.float64)
        hits = alb[..., 3]
        out["hits"] = hits.astype(np.float32)
        out["coverage"] = _div(hits, aovs.get("passes", 0)).astype(np.float32)
        out["albedo"] = _div(alb[..., :3], hits[..., None]).astype(np.float32)
        n = _div(nd[..., :3], hits[..., None])
        out["normal"] = _div(n, np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        out["depth"] = _div(nd[..., 3], hits).astype(np.float32)
    if "moments" in aovs:
        mom = aovs["moments"].astype(np.float64)
        n = mom[..., 3]
        out["samples"] = n.astype(np.float32)
        if frame is not None:
            mean = _div(np.asarray(frame, dtype=np.float64)[..., :3], n[..., None])
            nn = n[..., None]
            s2 = _div(np.maximum(mom[..., :3] - nn * mean * mean, 0.0), nn - 1.0)
            out["variance"] = np.where(nn >= 2, _div(s2, nn), 0.0).astype(np.float32)
    return out
