"""Synthetic frames, planes and cameras for the CPU reference tests (tests/test_*_ref.py): what a renderer would leave behind, made with
numpy from a seed; the bit-exact comparison of two arrays; and the matrices that the camera moves of device_support.py use too."""
import ctypes as C
import math

import numpy as np

from heatray_amd import _ffi as ffi
from heatray_amd import denoise, history, scenes

F = np.float32


def camera(view=None, fov=0.24, aspect=None, W=1, H=1):
    """A PassParams that holds a camera: view = camera -> world as m[row, col]"""
    p = ffi.PassParams()
    m = np.eye(4) if view is None else np.asarray(view, np.float64)
    p.view_matrix = (C.c_float * 16)(*m.astype(F).T.reshape(-1))
    p.fov_tan = fov
    p.aspect_ratio = aspect if aspect is not None else W / H
    return p


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


MOVES = {
    "none": lambda: (np.eye(4), 0.24),
    "yaw": lambda: (rot_y(0.05), 0.24),
    "orbit": lambda: (translate(0, 0, -6) @ rot_y(0.3) @ translate(0, 0, 6), 0.24),
    "pitch_shift": lambda: (translate(0.3, -0.2, 0.1) @ rot_x(-0.07), 0.24),
    "dolly": lambda: (translate(0, 0, -0.6), 0.24),
    "zoom": lambda: (np.eye(4), 0.31),
}


def uniform(rng, shape):
    """SplitMix64 content -> float32 in [0, 1)"""
    n = int(np.prod(shape))
    return ((rng.u64(n) >> np.uint64(40)).astype(np.float64) / float(1 << 24)).astype(F).reshape(shape)


def plane_view(W, H, cam, seed, depth=6.0, max_n=40, holes=True, sky=True, noise=True):
    """A frame and its planes as a renderer would leave them in front of the world plane z = -depth (normal 0 0 1), seen with `cam`:
    per-pixel sample counts (some 0), coverage between 0 and 1 (sky patches, half-covered pixels), normals and depths disturbed at some
    pixels (what the tap tests must reject), colours and moments from SplitMix64."""
    rng = scenes.SplitMix64(seed)
    v = np.array(list(cam.view_matrix), np.float64).reshape(4, 4).T
    y, x = np.mgrid[0:H, 0:W]
    cx = (2 * (x + 0.5) / W - 1) * cam.aspect_ratio * cam.fov_tan
    cy = (2 * (y + 0.5) / H - 1) * cam.fov_tan
    d = cx[..., None] * v[:3, 0] + cy[..., None] * v[:3, 1] - v[:3, 2]
    with np.errstate(all="ignore"):
        s = (-depth - v[2, 3]) / d[..., 2]
    hit = np.isfinite(s) & (s > 0)
    u = uniform(rng, (8, H, W))
    n = np.floor(u[0] * (max_n + 1)) if holes else np.full((H, W), float(max_n))
    if holes:
        n[u[1] < 0.05] = 0
    cov = np.where(hit, 1.0, 0.0)
    if sky:
        blocks = uniform(rng, ((H + 7) // 8, (W + 7) // 8))[y // 8, x // 8]
        cov = np.where(blocks < 0.2, 0.0, cov)                         # sky patches
        cov = np.where((u[2] < 0.1) & hit, np.round(u[3] * 4) / 4, cov)  # partly covered pixels: 0, 1/4 .. 1
    hits = np.floor(n * cov)
    normal = np.zeros((H, W, 3))
    normal[..., 2] = 1.0
    dep = np.where(hit, s, 0.0)
    if noise:
        turn = u[4] < 0.1
        ang = u[5] * 1.2
        normal[turn] = np.stack([np.sin(ang), np.zeros_like(ang), np.cos(ang)], -1)[turn]
        dep = np.where(u[6] < 0.1, dep * (1 + 0.2 * (u[7] - 0.5)), dep)
    col = uniform(rng, (H, W, 3)) * F(1.5) + F(0.02)
    frame, planes = np.zeros((H, W, 4), F), {k: np.zeros((H, W, 4), F) for k in history.PLANES}
    frame[..., :3], frame[..., 3] = col * n[..., None], n
    planes["moments"][..., :3], planes["moments"][..., 3] = (col * col * F(1.3)) * n[..., None], n
    planes["albedo"][..., :3], planes["albedo"][..., 3] = uniform(rng, (H, W, 3)) * hits[..., None], hits
    planes["normal_depth"][..., :3], planes["normal_depth"][..., 3] = normal * hits[..., None], dep * hits
    return frame, planes


def flat(W, H, n, colour=(0.5, 0.25, 0.125), depth=6.0, cov=1.0, normal=(0.0, 0.0, 1.0)):
    """n samples of one colour everywhere on a surface of one depth and normal (cov = 0: sky)"""
    frame, planes = np.zeros((H, W, 4), F), {k: np.zeros((H, W, 4), F) for k in history.PLANES}
    c = np.asarray(colour, F)
    frame[..., :3], frame[..., 3] = c * F(n), n
    planes["moments"][..., :3], planes["moments"][..., 3] = (c * c) * F(n), n
    hits = F(n * cov)
    planes["albedo"][..., :3], planes["albedo"][..., 3] = F(0.5) * hits, hits
    planes["normal_depth"][..., :3], planes["normal_depth"][..., 3] = np.asarray(normal, F) * hits, F(depth) * hits
    return frame, planes


def merge_input(old, old_cam, new, new_cam, p):
    """what tests/host/history_cpu.cpp and reproject_cpu.cpp read first: int32 W, H, max_history, 0; float normal_cos, plane_tol, min_weight,
    0; both cameras (view matrix, aspect, fov_tan); the old (frame, planes), then the new"""
    H, W = old[0].shape[:2]
    cam_floats = lambda pp: np.array(list(pp.view_matrix) + [pp.aspect_ratio, pp.fov_tan], F)
    data = [np.array([W, H, p.max_history, 0], np.int32), np.array([p.normal_cos, p.plane_tol, p.min_weight, 0], F), cam_floats(old_cam), cam_floats(new_cam)]
    for frame, planes in (old, new):
        data += [np.ascontiguousarray(frame, F)] + [np.ascontiguousarray(planes[k], F) for k in history.PLANES]
    return b"".join(a.tobytes() for a in data)


def filter_params(iterations=5, normal_power=7, sigma_l=4.0, sigma_z=4.0):
    p = denoise.default_params()
    p.iterations, p.normal_power, p.sigma_l, p.sigma_z = iterations, normal_power, sigma_l, sigma_z
    return p


def synthetic(W, H, n_passes, seed, hits="partial", holes=False):
    """A frame and its planes as n_passes of a noisy renderer would leave them: two surfaces split by a slanted edge, a background
    strip, per-pass samples around a smooth mean."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    side = (x + F(0.5) * y) > F(0.55) * F(W)
    frame, alb, nd, mom = (np.zeros((H, W, 4), F) for _ in range(4))
    for _ in range(n_passes):
        if hits == "none":
            hit = np.zeros((H, W), bool)
        elif hits == "all":
            hit = np.ones((H, W), bool)
        else:
            hit = (rng.random((H, W)) < np.where(y < F(0.15) * F(H), 0.0, np.where(np.abs(x - F(0.3) * F(W)) < 2, 0.5, 1.0)))
        base = np.where(side[..., None], F([0.8, 0.3, 0.2]), F([0.2, 0.5, 0.9])).astype(F) * (F(0.6) + F(0.4) * rng.random((H, W, 1)).astype(F))
        light = (F(0.5) + x / F(max(W, 2))) [..., None] * rng.gamma(2.0, 0.5, (H, W, 3)).astype(F)
        s = np.where(hit[..., None], base * light, F(0.7)).astype(F)
        frame[..., :3] += s
        frame[..., 3] += F(1)
        mom[..., :3] += s * s
        mom[..., 3] += F(1)
        nrm = np.where(side[..., None], F([0.0, 0.6, 0.8]), F([0.6, 0.0, 0.8])).astype(F) + F(0.05) * rng.standard_normal((H, W, 3)).astype(F)
        nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(F)
        depth = (F(3.0) + F(0.02) * x + np.where(side, F(1.5), F(0.0)) + F(0.01) * rng.random((H, W)).astype(F)).astype(F)
        alb[..., :3] += np.where(hit[..., None], base, F(0))
        alb[..., 3] += hit
        nd[..., :3] += np.where(hit[..., None], nrm, F(0))
        nd[..., 3] += np.where(hit, depth, F(0))
    if holes:
        dead = rng.random((H, W)) < 0.3
        for p in (frame, alb, nd, mom):
            p[dead] = 0
    return frame, {"albedo": alb, "normal_depth": nd, "moments": mom}


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, what
    if g.tobytes() != w.tobytes():
        bad = np.argwhere(g.view(np.uint32 if g.dtype == F else g.dtype) != w.view(np.uint32 if w.dtype == F else w.dtype))
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} against {w[tuple(bad[0])]}")
