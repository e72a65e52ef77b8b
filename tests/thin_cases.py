"""Thin triangles in one plane, rays aimed at them from a distance, float64 truth, and the hit rule of DESIGN.md §4 restated in numpy
float32 (tests/test_hit_truth.py without a GPU and on one, tools/hit_truth_table.py).

A cell is one plane with 64 thin triangles of one aspect in it (long edge 0.2 to 1.0, none overlapping another) plus two small anchor
triangles in opposite corners of [-1, 1]^3, so that every cell has the same scene diagonal; rays are aimed at interior points of the
thin triangles from D scene diagonals away.  Truth is float64 Möller–Trumbore on the same float32 inputs."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_phantoms import cross, dot, moller_trumbore  # noqa: E402  (float32, the contract's operation order)

F = np.float32
ASPECTS = (10, 100, 1000, 10000)
DISTANCES = (0.2, 1.5, 5.0)
PLANES = ("x", "y", "z", "tilt1e-4", "tilt1e-2", "free")
N_TRIS, N_RAYS = 64, 2000
RETRY_S2 = F(9e-10)  # hr_trace.h: kRetryS2 (s = 3e-5, squared)


# ------------------------------------------------------------------------------------------------ scenes
def _frame(plane, rng):
    """orthonormal (a, b, n), float64: the plane's two directions and its normal"""
    e = np.eye(3)
    if plane in ("x", "y", "z"):
        k = "xyz".index(plane)
        return e[(k + 1) % 3], e[(k + 2) % 3], e[k]
    if plane == "free":
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        return q[:, 0], q[:, 1], np.cross(q[:, 0], q[:, 1])
    ang = float(plane[4:])           # the plane z = const turned by `ang` about a direction inside it
    phi = rng.uniform(0, 2 * np.pi)
    ax = np.array([np.cos(phi), np.sin(phi), 0.0])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    return R @ e[0], R @ e[1], R @ e[2]


@functools.lru_cache(maxsize=None)
def make_cell(aspect, plane, seed=0):
    """(66, 3, 3) float32 vertex positions: 64 triangles of width = long edge / aspect in one plane, then the two anchors"""
    rng = np.random.default_rng([seed, aspect, PLANES.index(plane)])
    a, b, n = _frame(plane, rng)
    # No two of them overlap, so that no robust ray can be shadowed: each triangle has a lane of its own, 0.022 wide, across the
    # cell's in-plane direction (one random rotation per cell); its width stays below 0.018 (at 1:10 the long edge is 0.1 to 0.18)
    L = rng.uniform(0.2, 1.0, N_TRIS) if aspect >= 100 else rng.uniform(0.1, 0.18, N_TRIS)
    s = rng.uniform(0.3, 0.7, N_TRIS)
    x0, y0 = rng.uniform(-0.1, 0.1, N_TRIS), (np.arange(N_TRIS) - (N_TRIS - 1) / 2) * 0.022
    flip = rng.integers(0, 2, N_TRIS) * 2 - 1   # (either winding)
    c0 = rng.uniform(-0.3, 0.3)
    loc = np.stack([np.stack([x0 - flip * L / 2, y0], 1), np.stack([x0 + flip * L / 2, y0], 1), np.stack([x0 + (s - 0.5) * L, y0 + L / aspect], 1)], 1)  # (64, 3, 2)
    th = rng.uniform(0, 2 * np.pi)
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    loc = loc @ rot.T
    tris = c0 * n + loc[..., 0:1] * a + loc[..., 1:2] * b
    anchors = np.array([[[-1, -1, -1], [-0.99, -1, -1], [-1, -0.99, -1]], [[1, 1, 1], [0.99, 1, 1], [1, 0.99, 1]]], dtype=np.float64)
    out = np.concatenate([tris, anchors]).astype(F)
    out.setflags(write=False)
    return out


def diagonal(tris):
    p = tris.reshape(-1, 3).astype(np.float64)
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


@functools.lru_cache(maxsize=None)
def make_rays(aspect, plane, D, n=N_RAYS, seed=0):
    """(origins, directions, aimed-at triangle) float32: from D diagonals away at interior points (u, v > 0.12, u + v < 0.88) of the
    thin triangles, at an angle to the plane's normal whose |cosine| is above 0.35"""
    tris = make_cell(aspect, plane, seed).astype(np.float64)
    rng = np.random.default_rng([seed, aspect, PLANES.index(plane), int(D * 10), 1])
    k = rng.integers(0, N_TRIS, n)
    uv = rng.uniform(0, 1, (n, 2))
    uv = np.where((uv.sum(axis=1) > 1)[:, None], 1 - uv, uv)
    uv = 0.12 + 0.64 * uv
    v0, e1, e2 = tris[k, 0], tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0]
    p = v0 + uv[:, 0:1] * e1 + uv[:, 1:2] * e2
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    w = rng.normal(size=(4 * n + 64, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    w = w[np.abs(w @ nrm[0]) > 0.35][:n]   # (the cell's triangles share one plane up to rounding and a sign)
    assert w.shape[0] == n
    o = (p - D * diagonal(tris) * w).astype(F)
    d = p - o.astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    for arr in (o, d, k):
        arr.setflags(write=False)
    return o, d, k


def scene(tris, name="thin"):
    """tris (n, 3, 3) float32 as a scene: identity transform, the engines form v0, e1 = p1 - p0, e2 = p2 - p0 from them"""
    from heatray_amd import host, scenes
    sc = scenes.Scene(name, width=32, height=32)
    pos = np.ascontiguousarray(tris, dtype=F).reshape(-1, 3)
    nrm = np.tile(np.array([0, 0, 1], F), (pos.shape[0], 1))
    sc.materials = scenes._material_palette(scenes.SplitMix64(1), 2)
    sc.meshes.append(scenes.MeshData(pos, nrm, np.arange(pos.shape[0], dtype=np.uint32), material_id=0))
    sc.lights.add_directional(color=(1, 1, 1), illuminance=10.0, phi=0.3, theta=0.5)
    scenes._camera_for(sc, np.array([-1, -1, -1], F), np.array([1, 1, 1], F))
    sc.options.max_ray_depth, sc.options.max_render_passes = 1, 8
    sc.options.fstop = host.FSTOP_DISABLED
    return sc


# ------------------------------------------------------------------------------------------------ float64 truth
def truth(tris, o, d, k, eps, D):
    """Float64 Möller–Trumbore of every ray against every triangle, on the float32 inputs.  Returns
    robust: the ray is a robust true hit of the triangle k it was aimed at (u, v > 0.1, u + v < 0.9, t > 10 eps, |d.n| > 0.3),
    alone:  ... and no other triangle can be reported in its place: none that the ray's line meets inside or NEAR its outline (below)
            lies in front of, or less than 1e-3 diagonals behind, that hit,
    t:      the float64 distance to triangle k."""
    T = tris.astype(np.float64)
    o, d = o.astype(np.float64)[:, None, :], d.astype(np.float64)[:, None, :]
    v0, e1, e2 = T[None, :, 0], (T[:, 1] - T[:, 0])[None], (T[:, 2] - T[:, 0])[None]
    diag = diagonal(tris)
    with np.errstate(all="ignore"):
        pvec = np.cross(d, e2)
        det = (e1 * pvec).sum(-1)
        tvec = o - v0
        u = (tvec * pvec).sum(-1) / det
        qvec = np.cross(tvec, e1)
        v = (d * qvec).sum(-1) / det
        t = (e2 * qvec).sum(-1) / det
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    cosn = np.abs((d * n).sum(-1)) / np.linalg.norm(d, axis=-1)
    r = np.arange(o.shape[0])
    robust = (u[r, k] > 0.1) & (v[r, k] > 0.1) & (u[r, k] + v[r, k] < 0.9) & (t[r, k] > 10 * eps) & (cosn[r, k] > 0.3)
    # NEAR the outline of another triangle j: within what float32 could mistake for inside.  The coordinates of a ray from D diagonals
    # away carry an absolute error of a few 2^-24 (|o| + t) <= 2^-24 * 4 (D + 1) diag; in barycentric units of j that is this error over
    # j's width.  40 times that, and never less than 0.05.
    width = np.linalg.norm(np.cross(e1, e2), axis=-1) / np.maximum(np.linalg.norm(e1, axis=-1), np.linalg.norm(e2, axis=-1))
    m = 0.05 + 40 * 2.0 ** -24 * 4 * (D + 1) * diag / width
    with np.errstate(all="ignore"):
        near = (u > -m) & (v > -m) & (u + v < 1 + m) & (t > 0) & (t < t[r, k][:, None] + 1e-3 * diag)
    near[r, k] = False
    return robust, robust & ~near.any(axis=1), t[r, k]


# ------------------------------------------------------------------------------------------------ the hit rule, float32
def in_tri_box(p0, e1, e2, o, d, t, h):
    """hr_trace.h::hitInTriBox: seven operations per axis"""
    p1, p2 = p0 + e1, p0 + e2
    lo, hi = np.minimum(np.minimum(p0, p1), p2), np.maximum(np.maximum(p0, p1), p2)
    P = o + t[:, None] * d
    return ((P >= lo - h) & (P <= hi + h)).all(axis=1)


def hit_rule(p0, p1, p2, o, d, tmin, tmax, h, retry=True):
    """Row by row: does ray (o, d, tmin, tmax) hit triangle (p0, p1, p2)?  (hit, t, u, v, retried), float32 in the operation order of
    hr_trace.h / oracle_bvh.cpp.  retry=False: conditions 1-3 only (the rule before the plane retry)."""
    tmin, tmax, h = F(tmin), F(tmax), F(h)
    e1, e2 = p1 - p0, p2 - p0
    ok, t, u, v = moller_trumbore(p0, p1, p2, o, d)
    with np.errstate(all="ignore"):
        cand = ok & (t > tmin) & (t < tmax)
        box = in_tri_box(p0, e1, e2, o, d, t, h)
        hit = cand & box
        if not retry:
            return hit, t, u, v, np.zeros_like(hit)
        n = cross(e1, e2)
        guard = dot(n, n) >= RETRY_S2 * dot(e1, e1) * dot(e2, e2)
        den = dot(n, d)
        tp = dot(n, p0 - o) * (F(1.0) / den)
        again = cand & ~box & guard & (den != 0) & (tp > tmin) & (tp < tmax) & in_tri_box(p0, e1, e2, o, d, tp, h)
    return hit | again, np.where(again, tp, t), u, v, again


def closest(tris, o, d, eps, h, retry=True, chunk=512):
    """The brute-force closest hit of every ray, restated: (prim, t, u, v, retried) with prim = -1 for a miss"""
    R, T = o.shape[0], tris.shape[0]
    out = [np.full(R, -1, np.int32), np.zeros(R, F), np.zeros(R, F), np.zeros(R, F), np.zeros(R, bool)]
    for a in range(0, R, chunk):
        oo, dd = o[a:a + chunk], d[a:a + chunk]
        r = oo.shape[0]
        rep = lambda x: np.repeat(x, T, axis=0)
        til = lambda x: np.tile(x, (r, 1))
        hit, t, u, v, again = hit_rule(til(tris[:, 0]), til(tris[:, 1]), til(tris[:, 2]), rep(oo), rep(dd), eps, np.inf, h, retry)
        hit, t, u, v, again = (x.reshape(r, T) for x in (hit, t, u, v, again))
        tt = np.where(hit, t, np.inf)
        j = tt.argmin(axis=1)                     # (the first of equal distances: the lower id)
        rr = np.arange(r)
        got = hit[rr, j]
        out[0][a:a + chunk] = np.where(got, j, -1)
        for dst, src in zip(out[1:], (t, u, v, again)):
            dst[a:a + chunk] = np.where(got, src[rr, j], 0)
    return out


def scene_constants(info):
    """(eps, h, diagonal) float32 of a committed scene from its scene_info(), as oracle_scene.cpp / hr_scene.inl form them"""
    lo, hi = np.array(info.aabb_min, F), np.array(info.aabb_max, F)
    e = hi - lo
    length = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return F(1e-4) * length, F(0.5) * (F(1e-5) * length), length
