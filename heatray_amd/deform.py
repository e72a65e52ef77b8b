"""Deformable meshes of include/hrcore_deform.h restated in numpy float32, operation for operation: `reference_pose` gives the bits
k_deform_pose (heatray_amd/csrc/hr_deform.h) gives, `reference` adds the regeneration through heatray_amd.meshprep.reference and says what
the mesh block must hold afterwards.  It is the checker of the GPU tests and works without a GPU.

    eng.deform_bind(gid, joints=joints, weights=weights)
    eng.deform_pose(gid, joint_matrices=mats, params=deform.params(regenerate=3)); eng.commit()              # on the device
    block, result = deform.reference(rest, rig, None, mats, indices=idx, uvs=uvs, params=deform.params(regenerate=3))   # the same bits
"""
import numpy as np

from . import _ffi as ffi
from . import meshprep
from .meshprep import F, dot, normalize, valid

LARGEST = F(3.0e37)  # "finite": |x| <= this


def default_params():
    """hr_deform_default_params: regenerate 0, weight ANGLE, weld 1."""
    return ffi.DeformParams(0, ffi.HR_MESH_WEIGHT_ANGLE, 1)


def params(regenerate=0, weight=ffi.HR_MESH_WEIGHT_ANGLE, weld=1):
    return ffi.DeformParams(regenerate, weight, weld)


def _check(p):
    if p.regenerate & ~(ffi.HR_DEFORM_NORMALS | ffi.HR_DEFORM_TANGENTS):
        raise ValueError(f"unknown regenerate {p.regenerate}")
    if p.regenerate & ffi.HR_DEFORM_TANGENTS and not p.regenerate & ffi.HR_DEFORM_NORMALS:
        raise ValueError("regenerate TANGENTS needs NORMALS")
    if p.weight not in (ffi.HR_MESH_WEIGHT_ANGLE, ffi.HR_MESH_WEIGHT_AREA, ffi.HR_MESH_WEIGHT_UNIFORM):
        raise ValueError(f"unknown weight {p.weight}")
    if p.weld not in (0, 1):
        raise ValueError(f"weld = {p.weld} is neither 0 nor 1")
    if any(p.reserved):
        raise ValueError("reserved words must be 0")


def point(M, p):
    """M: n x 4 x 4 as numpy holds a matrix (m[row][col]), p: n x 3 -> M p with w = 1, in the header's order of operations"""
    return np.stack([((M[:, r, 0] * p[:, 0] + M[:, r, 1] * p[:, 1]) + M[:, r, 2] * p[:, 2]) + M[:, r, 3] for r in range(3)], axis=-1)


def direction(M, d):
    return np.stack([(M[:, r, 0] * d[:, 0] + M[:, r, 1] * d[:, 1]) + M[:, r, 2] * d[:, 2] for r in range(3)], axis=-1)


def _finish_direction(d, rest):
    """(normalize(d) where its squared length is valid, else the rest direction; how many kept the rest one)"""
    with np.errstate(all="ignore"):
        ok = valid(dot(d, d))
        out = np.where(ok[:, None], normalize(d), rest).astype(F)
    return out, int((~ok).sum())


def reference_pose(rest, rig, morph_weights=None, joint_matrices=None):
    """rest: {"positions", "normals"[, "tangents", "bitangents"]}, V x 3 each; rig: {"morph_positions", "morph_normals": K x V x 3,
    "joints": V x 4, "weights": V x 4}, each optional; morph_weights: K; joint_matrices: J x 4 x 4 (m[row][col]).
    -> (positions, normals, tangents, bitangents, rejected_vertices, kept_directions); an array the pose does not write is None."""
    restP, restN = (np.ascontiguousarray(rest[k], F).reshape(-1, 3) for k in ("positions", "normals"))
    frames = rest.get("tangents") is not None and rest.get("bitangents") is not None
    restT, restB = (np.ascontiguousarray(rest[k], F).reshape(-1, 3) for k in ("tangents", "bitangents")) if frames else (None, None)
    V = len(restP)
    dP, dN, joints, weights = (rig.get(k) for k in ("morph_positions", "morph_normals", "joints", "weights"))
    K = 0 if dP is None else np.asarray(dP).reshape(-1, V, 3).shape[0]
    skinned = joints is not None
    p, n = restP.copy(), restN.copy()
    t, b = (restT.copy(), restB.copy()) if frames else (None, None)
    with np.errstate(all="ignore"):
        if K:
            dP = np.ascontiguousarray(dP, F).reshape(K, V, 3)
            dN = None if dN is None else np.ascontiguousarray(dN, F).reshape(K, V, 3)
            mw = np.ascontiguousarray(morph_weights, F).reshape(-1)
            for k in range(K):
                p = p + dP[k] * mw[k]
                if dN is not None:
                    n = n + dN[k] * mw[k]
        if skinned:
            joints = np.ascontiguousarray(joints, np.uint32).reshape(V, 4)
            weights = np.ascontiguousarray(weights, F).reshape(V, 4)
            mats = np.ascontiguousarray(joint_matrices, F).reshape(-1, 4, 4)
            P, N = np.zeros((V, 3), F), np.zeros((V, 3), F)
            T, B = (np.zeros((V, 3), F), np.zeros((V, 3), F)) if frames else (None, None)
            for i in range(4):
                w = weights[:, i]
                use = (w != F(0.0))[:, None]  # (-0 == 0: skipped too)
                M = mats[joints[:, i]]
                P = np.where(use, P + point(M, p) * w[:, None], P).astype(F)
                N = np.where(use, N + direction(M, n) * w[:, None], N).astype(F)
                if frames:
                    T = np.where(use, T + direction(M, t) * w[:, None], T).astype(F)
                    B = np.where(use, B + direction(M, b) * w[:, None], B).astype(F)
            p, n, t, b = P, N, T, B
        fine = (np.abs(p) <= LARGEST).all(axis=1)  # (a NaN compares false)
    positions = np.where(fine[:, None], p, restP).astype(F)
    kept = 0
    normals = tangents = bitangents = None
    if (K and dN is not None) or skinned:
        normals, k = _finish_direction(n, restN)
        kept += k
    if frames and skinned:
        tangents, k = _finish_direction(t, restT)
        kept += k
        bitangents, k = _finish_direction(b, restB)
        kept += k
    return positions, normals, tangents, bitangents, int((~fine).sum()), kept


def reference(rest, rig, morph_weights=None, joint_matrices=None, indices=None, mode=ffi.HR_TRIANGLES, uvs=None, params=None):
    """hr_deform_pose as a whole: the pose, then params.regenerate on the posed positions (indices, mode and uvs: the mesh's own).
    -> ({attribute name: the array the block must hold, for every attribute the call writes}, the hr_deform_result as a dict)."""
    p = params if params is not None else default_params()
    _check(p)
    pos, nrm, tan, bit, rejected, kept = reference_pose(rest, rig, morph_weights, joint_matrices)
    block = {"positions": pos}
    for name, a in (("normals", nrm), ("tangents", tan), ("bitangents", bit)):
        if a is not None:
            block[name] = a
    tri = meshprep.triangles(indices, mode) if indices is not None else np.zeros((0, 3), np.uint32)
    result = {"vertices": len(pos), "triangles": len(tri), "rejected_vertices": rejected, "kept_directions": kept, "regenerated": p.regenerate, "posed": 1,
              "mesh": dict.fromkeys(meshprep.RESULT_KEYS, 0)}
    result["mesh"].update(regenerate(block, indices, mode=mode, uvs=uvs, params=p))
    return block, result


def regenerate(block, indices, mode=ffi.HR_TRIANGLES, uvs=None, params=None):
    """params.regenerate on block["positions"] (hr_geom_update's and hr_deform_pose's): the regenerated arrays replace the block's;
    returns the hr_mesh_result's counters ({} without a regeneration)."""
    p = params if params is not None else default_params()
    _check(p)
    if not p.regenerate:
        return {}
    n, t, b, res = meshprep.reference(block["positions"], indices, uvs=uvs, mode=mode, params=meshprep.params(p.weight, p.weld, p.regenerate))
    block["normals"] = n
    if p.regenerate & ffi.HR_DEFORM_TANGENTS:
        block["tangents"], block["bitangents"] = t, b
    return res
