"""The denoiser of include/hrcore_denoise.h restated in numpy float32, operation for operation: `reference(frame, planes, params)`
gives the bits the device kernels (heatray_amd/csrc/hr_denoise.h) give.  It is the checker of the GPU tests and a denoiser for anyone
without a GPU (slow: a 1080p frame takes tens of seconds).

    eng.set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS); ... render ...
    img = eng.denoise()                                       # on the device
    ref = denoise.reference(eng.readback(), eng.aovs())       # the same bits, on the host
"""
import numpy as np

from . import _ffi as ffi

F = np.float32
_K = (F(0.375), F(0.25), F(0.0625))  # the B3 spline, by |offset|
_G = (F(0.5), F(0.25))               # the 3 x 3 Gaussian, by |offset|


def default_params():
    """hr_denoise_default_params: 5 iterations, normal power 7, sigma_l 4, sigma_z 4, kernel chosen by the library."""
    return ffi.DenoiseParams(5, 7, 4.0, 4.0, ffi.HR_DENOISE_KERNEL_AUTO)


def exp_(xx):
    """hr_math.h's exp_ (Cephes expf in plain float32 operations) on an array."""
    xx = np.asarray(xx, F)
    with np.errstate(all="ignore"):
        x = xx
        z = np.floor(F(1.44269504088896341) * x + F(0.5))
        x = x - z * F(0.693359375)
        x = x - z * F(-2.12194440e-4)
        n = np.clip(np.where(np.isfinite(z), z, 0), -200, 200).astype(np.int32)
        z = x * x
        z = (((((F(1.9875691500e-4) * x + F(1.3981999507e-3)) * x + F(8.3334519073e-3)) * x + F(4.1665795894e-2)) * x
              + F(1.6666665459e-1)) * x + F(5.0000001201e-1)) * z + x + F(1.0)
        scale = ((n + 127).astype(np.uint32) << np.uint32(23)).view(F)
        r = (z * scale).astype(F)
        r = np.where(xx > F(88.0), F(np.inf), r)
        r = np.where(~(xx >= F(-87.0)), np.where(np.isnan(xx), xx, F(0.0)), r)
    return r.astype(F)


def _fmax(x, y):
    """hr_math.h's fmax_: (x < y) ? y : x"""
    return np.where(x < y, y, x).astype(F)


def lum(r, g, b):
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def _facing(nd, cov, ndq, covq):
    """hr_denoise.h's dnFacing: both pixels without a surface, or normals less than a right angle apart"""
    return ((cov == 0) & (covq == 0)) | ((nd[..., 0] * ndq[..., 0] + nd[..., 1] * ndq[..., 1]) + nd[..., 2] * ndq[..., 2] > 0)


def _shift(a, dy, dx):
    """(a[y + dy, x + dx] where that is inside the image, else 0; the mask of those pixels)"""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def prepare(frame, albedo, normal_depth, moments):
    """-> cv (demodulated colour, variance), nd (unit normal, depth), ac (effective albedo, coverage; -1 = invalid), grad"""
    Fr, A, G, M = (np.ascontiguousarray(p, F) for p in (frame, albedo, normal_depth, moments))
    with np.errstate(all="ignore"):
        n = Fr[..., 3]
        valid = n > 0
        hits = A[..., 3]
        miss = n - hits
        c = Fr[..., :3] / n[..., None]
        a = _fmax((A[..., :3] + miss[..., None]) / n[..., None], F(0.01))
        e = M[..., :3] - (n[..., None] * c) * c
        e = np.where(e > 0, e, F(0.0)).astype(F)
        vc = ((e / (n - F(1.0))[..., None]) / n[..., None]) / (a * a)
        v = np.where(n >= F(2.0), lum(vc[..., 0], vc[..., 1], vc[..., 2]), F(0.0)).astype(F)
        d = c / a
        l2 = (G[..., 0] * G[..., 0] + G[..., 1] * G[..., 1]) + G[..., 2] * G[..., 2]
        surf = hits > 0
        N = np.where((surf & (l2 > 0))[..., None], G[..., :3] / np.sqrt(l2)[..., None], F(0.0)).astype(F)
        z = np.where(surf, G[..., 3] / hits, F(0.0)).astype(F)
        cov = hits / n
    cv = np.where(valid[..., None], np.concatenate([d, v[..., None]], -1), F(0.0)).astype(F)
    nd = np.where(valid[..., None], np.concatenate([N, z[..., None]], -1), F(0.0)).astype(F)
    ac = np.concatenate([np.where(valid[..., None], a, F(0.0)), np.where(valid, cov, F(-1.0))[..., None]], -1).astype(F)
    # depth gradient: the largest difference to a direct neighbour with a surface facing the same way
    g = np.zeros(n.shape, F)
    has = ac[..., 3] > 0
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        ndq, ok = _shift(nd, dy, dx)
        cq, _ = _shift(ac[..., 3], dy, dx)
        t = np.abs(nd[..., 3] - ndq[..., 3])
        with np.errstate(all="ignore"):
            g = np.where(ok & (cq > 0) & _facing(nd, F(1.0), ndq, cq), _fmax(g, t), g).astype(F)
    g = np.where(has, g, F(0.0)).astype(F)
    return cv, nd, ac, g


def iterate(cv, nd, ac, grad, step, params):
    """One a-trous iteration at `step`: the new cv."""
    sigma_l, sigma_z, power = F(params.sigma_l), F(params.sigma_z), int(params.normal_power)
    cov = ac[..., 3]
    valid = ~(cov < 0)
    with np.errstate(all="ignore"):
        gv = np.zeros(cov.shape, F)
        gs = np.zeros(cov.shape, F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, ok = _shift(cv[..., 3], dy, dx)
                cq, _ = _shift(cov, dy, dx)
                m = ok & ~(cq < 0)
                if dx or dy:
                    m &= _facing(nd, cov, _shift(nd, dy, dx)[0], cq)
                g = _G[abs(dy)] * _G[abs(dx)]
                gv = np.where(m, gv + g * vq, gv).astype(F)
                gs = np.where(m, gs + g, gs).astype(F)
        sl = sigma_l * np.sqrt(gv / gs) + F(1e-6)
        zs = (sigma_z * (grad * F(step)) + F(1e-3) * np.abs(nd[..., 3])) + F(1e-30)
        lp = lum(cv[..., 0], cv[..., 1], cv[..., 2])
        S = np.zeros(cv.shape[:2] + (3,), F)
        V = np.zeros(cov.shape, F)
        Wt = np.zeros(cov.shape, F)
        for j in range(-2, 3):
            for i in range(-2, 3):
                cvq, ok = _shift(cv, j * step, i * step)
                if not ok.any():
                    continue
                covq, _ = _shift(cov, j * step, i * step)
                k = _K[abs(j)] * _K[abs(i)]
                if i == 0 and j == 0:
                    w = np.full(cov.shape, k, F)
                else:
                    ndq, _ = _shift(nd, j * step, i * step)
                    wn = _fmax((nd[..., 0] * ndq[..., 0] + nd[..., 1] * ndq[..., 1]) + nd[..., 2] * ndq[..., 2], F(0.0))
                    for _ in range(power):
                        wn = wn * wn
                    wn = np.where((cov == 0) & (covq == 0), F(1.0), wn).astype(F)
                    wc = _fmax(F(1.0) - F(4.0) * np.abs(cov - covq), F(0.0))
                    we = exp_(-(np.abs(nd[..., 3] - ndq[..., 3]) / zs + np.abs(lp - lum(cvq[..., 0], cvq[..., 1], cvq[..., 2])) / sl))
                    w = ((k * wn) * wc) * we
                m = ok & ~(covq < 0) & (w > 0)
                S = np.where(m[..., None], S + w[..., None] * cvq[..., :3], S).astype(F)
                V = np.where(m, V + (w * w) * cvq[..., 3], V).astype(F)
                Wt = np.where(m, Wt + w, Wt).astype(F)
        out = np.concatenate([S / Wt[..., None], (V / (Wt * Wt))[..., None]], -1)
    return np.where(valid[..., None], out, F(0.0)).astype(F)


def reference(frame, planes, params=None):
    """The denoised image (H x W x 4 float32: rgb = mean colour, a = 1; pixels without samples 0) of a frame (Engine.readback) and its
    planes (Engine.aovs: "albedo", "normal_depth", "moments"), the bits hr_denoise gives."""
    params = params if params is not None else default_params()
    cv, nd, ac, grad = prepare(frame, planes["albedo"], planes["normal_depth"], planes["moments"])
    for it in range(int(params.iterations)):
        cv = iterate(cv, nd, ac, grad, 1 << it, params)
    valid = ~(ac[..., 3] < 0)
    out = np.concatenate([cv[..., :3] * ac[..., :3], np.ones(valid.shape + (1,), F)], -1)
    return np.where(valid[..., None], out, F(0.0)).astype(F)


def relative_mse(image, truth):
    """mean(|x - ref|^2 / (|ref|^2 + 0.01)) over the pixels, rgb"""
    a, r = np.asarray(image, np.float64)[..., :3], np.asarray(truth, np.float64)[..., :3]
    return float(np.mean(((a - r) ** 2).sum(-1) / ((r ** 2).sum(-1) + 1e-2)))
