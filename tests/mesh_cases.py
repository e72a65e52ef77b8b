"""Meshes the mesh-preparation tests share (tests/test_mesh_ref.py without a GPU, tests/test_gpu_mesh.py on one), and the comparison of
a result with heatray_amd.meshprep.reference: every array byte for byte, every counter equal."""
import numpy as np

from device_support import same
from heatray_amd import _ffi as ffi
from heatray_amd import meshprep

F = np.float32
WEIGHTS = (ffi.HR_MESH_WEIGHT_ANGLE, ffi.HR_MESH_WEIGHT_AREA, ffi.HR_MESH_WEIGHT_UNIFORM)
BOTH = ffi.HR_MESH_WANT_NORMALS | ffi.HR_MESH_WANT_TANGENTS


def grid(nx, ny, seed=1, strip=False):
    """(positions, uvs, indices, mode) of nx x ny quads over a bumpy height field: (nx + 1)(ny + 1) vertices, 2 nx ny triangles as a
    list, or one strip with repeated indices between its rows (whose zero-area triangles are counted degenerate)"""
    rng = np.random.default_rng(seed)
    X, Z = np.meshgrid(np.linspace(-1, 1, nx + 1), np.linspace(-1, 1, ny + 1))
    Y = 0.2 * np.sin(3 * X) * np.cos(2 * Z) + 0.02 * rng.uniform(-1, 1, X.shape)
    pos = np.stack([X, Y, Z], axis=-1).astype(F).reshape(-1, 3)
    uv = np.stack([(X + 1) / 2, (Z + 1) / 2], axis=-1).astype(F).reshape(-1, 2)
    i = np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]
    if not strip:
        a, b, c, d = i, i + 1, i + nx + 2, i + nx + 1
        return pos, uv, np.stack([a, d, c, a, c, b], axis=-1).reshape(-1).astype(np.uint32), ffi.HR_TRIANGLES
    idx = []
    for r in range(ny):
        row = []
        for x in range(nx + 1):
            row += [r * (nx + 1) + x, (r + 1) * (nx + 1) + x]
        if r:  # two repeated indices join the rows and keep the winding's parity
            idx += [idx[-1], row[0]]
        idx += row
    return pos, uv, np.array(idx, np.uint32), ffi.HR_TRIANGLE_STRIP


def cube24():
    """a unit cube with 4 vertices per face (24), CCW seen from outside: (positions, uvs, indices)"""
    pos, uv, idx = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            corners = [(-1, -1), (1, -1), (1, 1), (-1, 1)] if sign > 0 else [(-1, -1), (-1, 1), (1, 1), (1, -1)]
            base = len(pos)
            for ca, cb in corners:
                p = [0.0, 0.0, 0.0]
                p[axis], p[a], p[b] = sign, ca, cb
                pos.append(p)
                uv.append([(ca + 1) / 2, (cb + 1) / 2])
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(pos, F), np.array(uv, F), np.array(idx, np.uint32)


def fan(n):
    """n triangles round vertex 0 (a cone, so that the centre's normal is no face's)"""
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([np.cos(ang), np.full(n, -0.3), -np.sin(ang)], axis=-1)
    pos = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(F)
    uv = np.concatenate([[[0.5, 0.5]], 0.5 + 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=-1)]).astype(F)
    k = np.arange(n)
    idx = np.stack([np.zeros(n, int), 1 + k, 1 + (k + 1) % n], axis=-1).reshape(-1).astype(np.uint32)
    return pos, uv, idx


def fin():
    """two triangles over the same three points with opposite windings: their normals cancel in every vertex"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    uv = np.array([[0, 0], [1, 0], [0, 1]], F)
    return pos, uv, np.array([0, 1, 2, 0, 2, 1], np.uint32)


def given_normals(pos, seed=3):
    """some caller's normals: unnormalised, with a zero and a huge one among them"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=pos.shape).astype(F)
    n[0] = 0
    if len(n) > 1:
        n[1] = (1e30, 1e30, 0)  # its squared length overflows: no N
    return n


def check(got, pos, idx, uvs=None, normals=None, mode=ffi.HR_TRIANGLES, params=None, what=""):
    """got = (normals, tangents, bitangents, result dict) against the reference, exactly; returns the reference's tuple"""
    want = meshprep.reference(pos, idx, uvs=uvs, normals=normals, mode=mode, params=params)
    for name, g, w in zip(("normals", "tangents", "bitangents"), got[:3], want[:3]):
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            same(np.ascontiguousarray(g, F).reshape(-1, 1, 3), w.reshape(-1, 1, 3), f"{what}: {name}")
    assert got[3] == want[3], (what, got[3], want[3])
    return want
