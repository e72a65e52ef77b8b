"""Motion reprojection (include/hrcore_motion.h): the trace's resolve, the merge and the motion vectors restated in numpy float32,
operation for operation — `reference_trace`, `reference_merge` and `reference_vectors` give the bits the device kernels
(heatray_amd/csrc/hr_motion.h) give — `camera_rays`, the pixel-centre rays the trace walks, and a small driver that makes the sequence a
viewer makes when its scene moves.

    eng.set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS); eng.clear()
    ... render ...
    r = motion.move_scene(eng, scene, lambda eng: eng.set_transform(gid, new_world), passes=2)   # capture, snapshot, edit, commit, clear, render, merge
    r["reused_pixels"], r["unmatched_pixels"]
    mv = eng.motion_vectors()                                                                    # H x W x 4: dx, dy, old depth, class

The hits come into `reference_trace` as data (Engine.query of `camera_rays` returns exactly the hits the trace finds): the references
work without a GPU.  The limits (the header has them in full): a pinhole at the lens centre; first surface only; view-dependent shading
and lighting that changed with the motion are taken over, bounded by max_history; material and light edits still need history_drop;
context groups and tile shards are refused.
"""
import numpy as np

from . import _ffi as ffi
from . import history
from .deform import direction, point
from .history import PLANES, _dot, _finite, _ray_x, _ray_y
from .meshprep import F, cross, dot, normalize, triangles, valid

_INF = F(np.inf)


def default_params():
    """hr_motion_default_params: history's defaults with normal_cos 0.8 (a geometric normal against an interpolated one)."""
    return ffi.HistoryParams(32, 0.8, 0.02, 0.25)


def _view(pass_params):
    """the view matrix as numpy holds a matrix (m[row][col]), float32"""
    return np.array(pass_params.view_matrix[:], F).reshape(4, 4).T


def camera_rays(pass_params, W, H):
    """The ray through the centre of every pixel of a W x H frame, in the frame's memory order (row 0 = bottom) -> (W * H) x 6 float32
    (o, d): o = eye(V), d = normalize(dir(V, ray(x, y; aspect, fov)))."""
    V = _view(pass_params)
    aspect, fov = F(pass_params.aspect_ratio), F(pass_params.fov_tan)
    y, x = np.mgrid[0:H, 0:W]
    n = W * H
    with np.errstate(all="ignore"):
        c = np.stack([_ray_x(x, F(W), aspect, fov), _ray_y(y, F(H), fov), np.full((H, W), -1.0, F)], axis=-1).astype(F).reshape(n, 3)
        d = normalize(direction(np.tile(V[None], (n, 1, 1)), c))
    o = np.tile(V[:3, 3][None], (n, 1))
    return np.concatenate([o, d], axis=1).astype(F)


def _unit_or_zero(x):
    with np.errstate(all="ignore"):
        ok = valid(dot(x, x))
        return np.where(ok[:, None], normalize(x), F(0.0)).astype(F)


def world_triangles(mesh):
    """(p0, e1, e2) of a mesh's triangles as the commit stores them, T x 3 each: p_k = point(world, positions[i_k]), e1 = p1 - p0,
    e2 = p2 - p0 (the triangles query.reference_surface makes)."""
    tri = triangles(mesh.indices, mesh.mode)
    m = np.eye(4, dtype=F) if mesh.world is None else np.ascontiguousarray(mesh.world, F).reshape(4, 4)
    M = np.tile(m[None], (len(tri), 1, 1))
    pos = np.ascontiguousarray(mesh.positions, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p0, p1, p2 = (point(M, pos[tri[:, k]]) for k in range(3))
        return p0.astype(F), (p1 - p0).astype(F), (p2 - p0).astype(F)


def reference_snapshot(meshes):
    """What hr_motion_snapshot stores for the committed meshes (in the order they were added): T x 12 float32."""
    parts = [np.concatenate([*world_triangles(m), np.zeros((len(triangles(m.indices, m.mode)), 3), F)], axis=1) for m in meshes]
    return np.concatenate(parts).astype(F) if parts else np.zeros((0, 12), F)


def reference_trace(hits, rays, current_meshes, snapshot_meshes, pass_params):
    """The motion planes from the hits of `rays` (camera_rays of `pass_params`; hits as Engine.query returns them, prim < 0: a miss).
    current_meshes / snapshot_meshes: [(hr_geom_id, mesh)] of the committed scene now and when the snapshot was taken, in the order
    they were added (objects with positions, indices, mode, world, like scenes.MeshData; a mesh without a triangle is skipped as the
    commit skips it).  -> (2 x n x 4 float32: Mv0, Mv1; {"surface_pixels", "sky_pixels", "unmatched_pixels"})."""
    r = np.ascontiguousarray(rays, F).reshape(-1, 6)
    o, d = r[:, :3], r[:, 3:]
    n = len(hits)
    n2 = _view(pass_params)[:3, 2]
    prim = hits["prim"].astype(np.int64)
    hit = prim >= 0
    mv = np.zeros((2, n, 4), F)
    with np.errstate(all="ignore"):
        Pw = o + d * hits["t"][:, None]
        depth = -dot(n2, Pw - o)
    mv[0, :, :3], mv[0, :, 3] = np.where(hit[:, None], Pw, F(0.0)), np.where(hit, F(-1.0), F(0.0))
    mv[1, :, 3] = np.where(hit, depth, _INF)
    snap = {gid: m for gid, m in snapshot_meshes}
    first = 0
    for gid, mesh in current_meshes:
        T = len(triangles(mesh.indices, mesh.mode))
        if T == 0:
            continue
        sel = np.nonzero((prim >= first) & (prim < first + T))[0]
        lt = prim[sel] - first
        first += T
        old = snap.get(gid)
        if sel.size == 0 or old is None or len(triangles(old.indices, old.mode)) != T:
            continue
        p0, e1, e2 = (a[lt] for a in world_triangles(old))
        u, v = hits["u"][sel][:, None], hits["v"][sel][:, None]
        with np.errstate(all="ignore"):
            Q = (p0 + e1 * u) + e2 * v
            Ng = _unit_or_zero(cross(e1, e2).astype(F))
        mv[0, sel, :3], mv[0, sel, 3] = Q, F(1.0)
        mv[1, sel, :3] = Ng
    w = mv[0, :, 3]
    return mv, {"surface_pixels": int((w == 1).sum()), "sky_pixels": int((w == 0).sum()), "unmatched_pixels": int((w == -1).sum())}


def _cameras(old_pass_params, new_pass_params):
    cam = history.cameras(old_pass_params, new_pass_params)
    cam["eye_old"] = np.array(old_pass_params.view_matrix[12:15], F)
    return cam


def _old_space(cam, Mv0, x, y, Wf, Hf):
    """mvOldSpace: the surface point (Mv0.w == 1) or the pixel's direction (otherwise) in the old camera's space"""
    R, O = cam["R"], cam["O"]
    r = [Mv0[..., k] - cam["eye_old"][k] for k in range(3)]
    cx, cy, cz = _ray_x(x, Wf, cam["aspect_new"], cam["fov_new"]), _ray_y(y, Hf, cam["fov_new"]), F(-1.0)
    known = Mv0[..., 3] == F(1.0)
    return [np.where(known, _dot(O[i, 0], O[i, 1], O[i, 2], r[0], r[1], r[2]), (R[i, 0] * cx + R[i, 1] * cy) + R[i, 2] * cz).astype(F) for i in range(3)]


def reference_merge(hist, old_pass_params, planes_mv, frame, planes, new_pass_params, params=None):
    """What hr_motion_merge leaves: (frame, {"albedo", "normal_depth", "moments"}, result) from the history captured with
    old_pass_params' camera, the motion planes (2 x H x W x 4) and the frame and planes of the view rendered with new_pass_params':
    hr_motion.h's mvMerge per pixel.  result = {"reused_pixels", "rejected_pixels", "history_samples"} plus "nh", the H x W float32 map
    of the samples each pixel took over (0 where none)."""
    p = params if params is not None else default_params()
    cam = _cameras(old_pass_params, new_pass_params)
    Hs = np.ascontiguousarray(hist, F)
    Fr = np.ascontiguousarray(frame, F).copy()
    A, G, M = (np.ascontiguousarray(planes[k], F).copy() for k in PLANES)
    H, W = Fr.shape[:2]
    mv = np.ascontiguousarray(planes_mv, F).reshape(2, H, W, 4)
    Mv0, Mv1 = mv[0], mv[1]
    Wf, Hf = F(W), F(H)
    O = cam["O"]
    max_h, ncos, ptol, minw = F(p.max_history), F(p.normal_cos), F(p.plane_tol), F(p.min_weight)
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        n = Fr[..., 3].copy()
        sampled = n > 0
        cov = A[..., 3] / n
        surf = sampled & (Mv0[..., 3] == F(1.0)) & (cov >= F(0.5))
        sky = sampled & (Mv0[..., 3] == F(0.0)) & (cov < F(0.5))
        ok = surf | sky
        q = _old_space(cam, Mv0, x, y, Wf, Hf)
        Ng = [Mv1[..., k] for k in range(3)]
        dmean = G[..., 3] / A[..., 3]
        ok &= ~surf | (np.abs(Mv1[..., 3] - dmean) <= ptol * dmean)
        Nq = [np.where(surf, _dot(O[i, 0], O[i, 1], O[i, 2], Ng[0], Ng[1], Ng[2]), F(0.0)).astype(F) for i in range(3)]
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
            nd = np.abs(_dot(Ng[0], Ng[1], Ng[2], h2[..., 0], h2[..., 1], h2[..., 2]))
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


def reference_vectors(planes_mv, old_pass_params, new_pass_params, W, H):
    """What hr_motion_vectors writes: H x W x 4 float32 (dx, dy, depth in the old camera, Mv0.w) from the motion planes of a trace with
    new_pass_params' camera; 0 0 0 Mv0.w where Mv0.w == -1 or the point is not in front of the old camera."""
    cam = _cameras(old_pass_params, new_pass_params)
    Mv0 = np.ascontiguousarray(planes_mv, F).reshape(2, H, W, 4)[0]
    Wf, Hf = F(W), F(H)
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        q = _old_space(cam, Mv0, x, y, Wf, Hf)
        z = -q[2]
        sx = (((q[0] / z) / cam["ax_old"] + F(1.0)) * F(0.5)) * Wf
        sy = (((q[1] / z) / cam["fov_old"] + F(1.0)) * F(0.5)) * Hf
        none = (Mv0[..., 3] == F(-1.0)) | ~(z > 0)
        out = np.stack([sx - (x.astype(F) + F(0.5)), sy - (y.astype(F) + F(0.5)), z, Mv0[..., 3]], axis=-1).astype(F)
    out[none, :3] = F(0.0)
    return out


def move_scene(eng, sc, edit, passes, params=None, first_pass=0):
    """The sequence a viewer makes when its scene moves: capture the frame rendered so far with sc.options (a scenes.Scene's) as it
    stands, snapshot the committed pose, run `edit(eng)` (set_transform, update_mesh, deform_pose, add_mesh, remove_mesh; it may change
    sc.options' camera too), commit, clear, render `passes` (>= 1) passes, merge.  The engine needs HR_AOV_SURFACE | HR_AOV_MOMENTS
    enabled before the captured frame's first pass.  Returns the merge's result dict."""
    if passes < 1:
        raise ValueError("move_scene: the new pose needs at least one pass before the merge (its planes are the guides)")
    eng.history_capture(sc.options.pass_params(0))
    eng.motion_snapshot()
    edit(eng)
    eng.commit()
    eng.clear()
    for s in range(passes):
        eng.render_pass(sc.options.pass_params(first_pass + s))
    return eng.motion_merge(sc.options.pass_params(first_pass), params)
