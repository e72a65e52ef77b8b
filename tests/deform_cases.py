"""Rest poses, rigs and poses the deformable-mesh tests share (tests/test_deform_ref.py without a GPU, tests/test_gpu_deform.py on one)."""
import numpy as np

from heatray_amd import meshprep

F = np.float32
U32 = np.uint32


def make_rest(V, frames, seed):
    """{"positions", "normals"[, "tangents", "bitangents"]}: random positions, unit directions"""
    rng = np.random.default_rng(seed)
    rest = {"positions": rng.normal(size=(V, 3)).astype(F), "normals": meshprep.normalize(rng.normal(size=(V, 3)).astype(F))}
    if frames:
        rest["tangents"] = meshprep.normalize(rng.normal(size=(V, 3)).astype(F))
        rest["bitangents"] = meshprep.normalize(rng.normal(size=(V, 3)).astype(F))
    return rest


def make_rig(V, K, J, morph_normals, seed):
    """K morphs (deltas of a tenth of the mesh's size) and J joints: four influences per vertex with weights that sum to 1, a fifth of
    the vertices with one or two of them at 0 or -0"""
    rng = np.random.default_rng(seed)
    rig = {"morph_positions": None, "morph_normals": None, "joints": None, "weights": None}
    if K:
        rig["morph_positions"] = (0.1 * rng.normal(size=(K, V, 3))).astype(F)
        if morph_normals:
            rig["morph_normals"] = (0.1 * rng.normal(size=(K, V, 3))).astype(F)
    if J:
        rig["joints"] = rng.integers(0, J, (V, 4)).astype(U32)
        w = rng.uniform(0.05, 1, (V, 4))
        w[rng.integers(0, 5, V) == 0, 3] = 0
        w[rng.integers(0, 5, V) == 0, 1] = 0
        w = (w / w.sum(axis=1, keepdims=True)).astype(F)
        w[::11, 3][w[::11, 3] == 0] = -0.0
        rig["weights"] = w
    return rig


def rigid(rng, n, spread=0.3):
    """n rigid 4 x 4 matrices (m[row][col]): a rotation about a random axis and a small translation"""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-1, 1, n)
    Kx = np.zeros((n, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3)[None] + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
    M = np.tile(np.eye(4), (n, 1, 1))
    M[:, :3, :3] = R
    M[:, :3, 3] = spread * rng.normal(size=(n, 3))
    return M.astype(F)


def pose_inputs(K, J, seed):
    """(morph weights or None, joint matrices J x 4 x 4 or None)"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, K).astype(F) if K else None), (rigid(rng, J) if J else None)
