"""History reprojection (include/hrcore_history.h): capture and merge restated in numpy float32, operation for operation —
`reference_capture` and `reference_merge` give the bits the device kernels (heatray_amd/csrc/hr_history.h) give — and a small driver
that makes the sequence a viewer makes when its camera moves.

    eng.set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS); eng.clear()
    ... render with options.view_matrix = old ...
    r = history.move_camera(eng, options, new_view_matrix, first_passes=1)   # capture, clear, render, merge
    r["reused_pixels"], r["history_samples"]

The limits (the header has them in full): the history's samples belong to another view, so a merged frame is biased, bounded by
max_history and by nothing else; view-dependent shading is taken over as if it were diffuse; first-surface guides only; pixels the new
view has not sampled take nothing over; context groups and tile shards are refused.
"""
import numpy as np

from . import _ffi as ffi

F = np.float32
PLANES = ("albedo", "normal_depth", "moments")


def default_params():
    """hr_history_default_params: max_history 32, normal_cos 0.9, plane_tol 0.02, min_weight 0.25."""
    return ffi.HistoryParams(32, 0.9, 0.02, 0.25)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _finite(v):
    return np.abs(v) < F(np.inf)


def _ray_x(x, Wf, aspect, fov):
    return ((F(2.0) * ((x.astype(F) + F(0.5)) / Wf) - F(1.0)) * aspect) * fov


def _ray_y(y, Hf, fov):
    return (F(2.0) * ((y.astype(F) + F(0.5)) / Hf) - F(1.0)) * fov


def _camera(pp):
    """(view matrix as 16 float32, column-major; aspect; fov_tan) of a PassParams"""
    return np.array(list(pp.view_matrix), F), F(pp.aspect_ratio), F(pp.fov_tan)


def cameras(old_pass_params, new_pass_params):
    """hsCameras: R = Rold^T Rnew (3 x 3), O = Rold^T, t = Rold^T (eye_new - eye_old), in float32 in the header's order."""
    vo, ao, fo = _camera(old_pass_params)
    vn, an, fn = _camera(new_pass_params)
    e = (vn[12:15] - vo[12:15]).astype(F)
    R, O, t = np.zeros((3, 3), F), np.zeros((3, 3), F), np.zeros(3, F)
    for i in range(3):
        o = vo[4 * i:4 * i + 3]
        for j in range(3):
            n = vn[4 * j:4 * j + 3]
            R[i, j] = _dot(o[0], o[1], o[2], n[0], n[1], n[2])
        O[i] = o
        t[i] = _dot(o[0], o[1], o[2], e[0], e[1], e[2])
    return {"R": R, "O": O, "t": t, "aspect_new": an, "fov_new": fn, "aspect_old": ao, "fov_old": fo, "ax_old": F(ao * fo)}


def reference_capture(frame, planes):
    """The history (3 x H x W x 4 float32: H0, H1, H2) of a frame (Engine.readback) and its planes (Engine.aovs): hr_history.h's hsCapture
    per pixel."""
    Fr = np.ascontiguousarray(frame, F)
    A, G, M = (np.ascontiguousarray(planes[k], F) for k in PLANES)
    with np.errstate(all="ignore"):
        n = Fr[..., 3]
        have = n > 0
        cov = A[..., 3] / n
        surf = have & (cov >= F(0.5))
        H0 = np.concatenate([Fr[..., :3] / n[..., None], n[..., None]], -1)
        H1 = np.concatenate([M[..., :3] / n[..., None], cov[..., None]], -1)
        l2 = _dot(G[..., 0], G[..., 1], G[..., 2], G[..., 0], G[..., 1], G[..., 2])
        l = np.sqrt(l2)
        N = np.where((l2 > 0)[..., None], G[..., :3] / l[..., None], F(0.0))
        H2 = np.concatenate([np.where(surf[..., None], N, F(0.0)), np.where(surf, G[..., 3] / A[..., 3], F(np.inf))[..., None]], -1)
        out = np.stack([H0, H1, H2]).astype(F)
        out[:, ~have] = F(0.0)
    return out


def reference_merge(history, old_pass_params, frame, planes, new_pass_params, params=None):
    """What hr_history_merge leaves: (frame, {"albedo", "normal_depth", "moments"}, result) from the history captured with
    old_pass_params' camera and the frame and planes of the view rendered with new_pass_params': hr_history.h's hsMerge per pixel.
    result = {"reused_pixels", "rejected_pixels", "history_samples"} plus "nh", the H x W float32 map of the samples each pixel took
    over (0 where none)."""
    p = params if params is not None else default_params()
    cam = cameras(old_pass_params, new_pass_params)
    Hs = np.ascontiguousarray(history, F)
    Fr = np.ascontiguousarray(frame, F).copy()
    A, G, M = (np.ascontiguousarray(planes[k], F).copy() for k in PLANES)
    H, W = Fr.shape[:2]
    Wf, Hf = F(W), F(H)
    R, O, t = cam["R"], cam["O"], cam["t"]
    max_h, ncos, ptol, minw = F(p.max_history), F(p.normal_cos), F(p.plane_tol), F(p.min_weight)
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        n = Fr[..., 3].copy()
        sampled = n > 0
        ok = sampled.copy()
        surf = sampled & (A[..., 3] / n >= F(0.5))
        cx, cy, cz = _ray_x(x, Wf, cam["aspect_new"], cam["fov_new"]), _ray_y(y, Hf, cam["fov_new"]), F(-1.0)
        rc = [(R[i, 0] * cx + R[i, 1] * cy) + R[i, 2] * cz for i in range(3)]
        d = G[..., 3] / A[..., 3]
        l2 = _dot(G[..., 0], G[..., 1], G[..., 2], G[..., 0], G[..., 1], G[..., 2])
        l = np.sqrt(l2)
        N = [np.where(surf & (l2 > 0), G[..., k] / l, F(0.0)).astype(F) for k in range(3)]
        q = [np.where(surf, d * rc[i] + t[i], rc[i]).astype(F) for i in range(3)]
        Nq = [np.where(surf, _dot(O[i, 0], O[i, 1], O[i, 2], N[0], N[1], N[2]), F(0.0)).astype(F) for i in range(3)]
        z = -q[2]
        ok &= z > 0
        sx = (((q[0] / z) / cam["ax_old"] + F(1.0)) * F(0.5)) * Wf
        sy = (((q[1] / z) / cam["fov_old"] + F(1.0)) * F(0.5)) * Hf
        ok &= (sx >= F(-1.0)) & (sx <= Wf + F(1.0)) & (sy >= F(-1.0)) & (sy <= Hf + F(1.0))
        fx = np.where(ok, sx - F(0.5), F(0.0)).astype(F)
        fy = np.where(ok, sy - F(0.5), F(0.0)).astype(F)
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = ptol * z
        wsum, ns = np.zeros((H, W), F), np.zeros((H, W), F)
        hs, ms = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
        for k in range(4):
            tx, ty = x0 + (k & 1), y0 + (k >> 1)
            w = (wx if k & 1 else F(1.0) - wx) * (wy if k >> 1 else F(1.0) - wy)
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            ux, uy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            h0, h1, h2 = Hs[0, uy, ux], Hs[1, uy, ux], Hs[2, uy, ux]
            use = ok & inside & (h0[..., 3] > 0) & (_finite(h2[..., 3]) == surf)
            nd = _dot(N[0], N[1], N[2], h2[..., 0], h2[..., 1], h2[..., 2])
            px = h2[..., 3] * _ray_x(ux, Wf, cam["aspect_old"], cam["fov_old"])
            py = h2[..., 3] * _ray_y(uy, Hf, cam["fov_old"])
            pz = h2[..., 3] * F(-1.0)
            pd = np.abs(_dot(Nq[0], Nq[1], Nq[2], px - q[0], py - q[1], pz - q[2]))
            use &= ~surf | ((nd >= ncos) & (pd <= tol))
            wsum = np.where(use, wsum + w, wsum).astype(F)
            hs = np.where(use[..., None], hs + w[..., None] * h0[..., :3], hs).astype(F)
            ms = np.where(use[..., None], ms + w[..., None] * h1[..., :3], ms).astype(F)
            ns = np.where(use, ns + w * h0[..., 3], ns).astype(F)
        ok &= ~(wsum < minw)
        nh = np.floor(np.where(max_h < ns / wsum, max_h, ns / wsum)).astype(F)  # fmin_(ns / wsum, max_history): (y < x) ? y : x
        h, m2 = hs / wsum[..., None], ms / wsum[..., None]
        k3 = ok[..., None]
        nh3 = nh[..., None]
        Fr[..., :3] = np.where(k3, Fr[..., :3] + h * nh3, Fr[..., :3])
        Fr[..., 3] = np.where(ok, Fr[..., 3] + nh, Fr[..., 3])
        M[..., :3] = np.where(k3, M[..., :3] + m2 * nh3, M[..., :3])
        M[..., 3] = np.where(ok, M[..., 3] + nh, M[..., 3])
        n3 = n[..., None]
        A[...] = np.where(k3, A + (A / n3) * nh3, A)
        G[...] = np.where(k3, G + (G / n3) * nh3, G)
        count = np.where(ok & (nh >= 0), nh, F(0.0)).astype(np.uint64)
    result = {"reused_pixels": int(ok.sum()), "rejected_pixels": int((sampled & ~ok).sum()), "history_samples": int(count.sum()),
              "nh": np.where(ok, nh, F(0.0)).astype(F)}
    return Fr, {"albedo": A, "normal_depth": G, "moments": M}, result


def move_camera(eng, options, new_view_matrix, first_passes, params=None, first_pass=0):
    """The sequence a viewer makes when its camera moves: capture the frame rendered so far with `options` (a scenes.RenderOptions) as
    it stands, clear, set options.view_matrix = new_view_matrix (m[row, col], as host.orbit_view_matrix returns it), render
    `first_passes` (>= 1) passes of the new view, merge.  The engine needs HR_AOV_SURFACE | HR_AOV_MOMENTS enabled before the captured
    frame's first pass.  Returns the merge's result dict."""
    if first_passes < 1:
        raise ValueError("move_camera: the new view needs at least one pass before the merge (its planes are the guides)")
    eng.history_capture(options.pass_params(0))
    eng.clear()
    options.view_matrix = np.asarray(new_view_matrix, dtype=F)
    for s in range(first_passes):
        eng.render_pass(options.pass_params(first_pass + s))
    return eng.history_merge(options.pass_params(first_pass), params)
