"""The arithmetic of hr_deform_pose without a GPU: heatray_amd/csrc/hr_deform.h compiled for the CPU (tests/host/deform_cpu.cpp, plain
and once more under AddressSanitizer + UBSan) against its numpy restatement heatray_amd.deform.reference_pose, byte for byte, and
properties of the reference alone on poses whose answers are known (include/hrcore_deform.h is the contract).  tests/test_gpu_deform.py
holds the device to the same reference."""
import numpy as np
import pytest

import cpu_header
from deform_cases import F, U32, make_rest, make_rig, pose_inputs
from heatray_amd import deform, meshprep
from mesh_cases import cube24


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cpu(request, tmp_path_factory):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    exe = cpu_header.build("deform", tmp_path_factory.mktemp("deform_" + request.param), flags=flags)

    def run(rest, rig, mw, mats):
        """dfPose over the whole rig -> (V x 12 floats: p, n, t, b; rejected; kept)"""
        V = len(rest["positions"])
        K = 0 if rig.get("morph_positions") is None else len(rig["morph_positions"])
        J = 0 if mats is None else len(mats)
        frames = "tangents" in rest
        parts = [np.array([V, K, J, (rig.get("morph_normals") is not None) * 1 + frames * 2], np.int32).tobytes()]
        parts += [np.ascontiguousarray(rest[k], F).tobytes() for k in ("positions", "normals", "tangents", "bitangents") if k in rest]
        parts += [np.ascontiguousarray(rig[k], F).tobytes() for k in ("morph_positions", "morph_normals") if rig.get(k) is not None]
        if J:
            parts += [np.ascontiguousarray(rig["joints"], U32).tobytes(), np.ascontiguousarray(rig["weights"], F).tobytes()]
        w8 = np.zeros(8, F)
        w8[:K] = mw if K else 0
        parts.append(w8.tobytes())
        if J:
            parts.append(np.ascontiguousarray(np.transpose(mats, (0, 2, 1)), F).tobytes())  # column-major, as the ABI holds them
        raw = cpu_header.run(exe, b"".join(parts))
        words = np.frombuffer(raw, F)
        return words[:-2].reshape(V, 12), int(words[-2:].view(U32)[0]), int(words[-2:].view(U32)[1])
    return run


def _against_reference(cpu, rest, rig, mw, mats, what):
    got, rejected, kept = cpu(rest, rig, mw, mats)
    p, n, t, b, wr, wk = deform.reference_pose(rest, rig, mw, mats)
    zero = np.zeros_like(p)
    # what the pose does not write stays the rest value in dfPose's result (0 for the frames of a mesh without them)
    want = [p, n if n is not None else rest["normals"], t if t is not None else rest.get("tangents", zero), b if b is not None else rest.get("bitangents", zero)]
    for k, (name, w) in enumerate(zip(("positions", "normals", "tangents", "bitangents"), want)):
        g = np.ascontiguousarray(got[:, 3 * k:3 * k + 3])
        bad = np.nonzero((g.view(U32) != np.ascontiguousarray(w, F).view(U32)).any(axis=1))[0]
        assert not len(bad), f"{what}: {name}: {len(bad)} vertices differ, first {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}"
    assert (rejected, kept) == (wr, wk), (what, rejected, kept, wr, wk)
    return wr, wk


@pytest.mark.parametrize("K, J", [(k, j) for k in (0, 1, 8) for j in (0, 1, 37) if k or j])  # (a rig needs morphs or joints)
@pytest.mark.parametrize("frames", [False, True])
def test_pose_equals_the_numpy_reference_byte_for_byte(cpu, K, J, frames):
    V = 300
    rest = make_rest(V, frames=frames, seed=K * 100 + J)
    for morph_normals in ((False, True) if K else (False,)):
        rig = make_rig(V, K, J, morph_normals=morph_normals, seed=K * 100 + J + 7)
        mw, mats = pose_inputs(K, J, seed=K + J)
        _against_reference(cpu, rest, rig, mw, mats, f"K={K} J={J} frames={frames} morph_normals={morph_normals}")


def test_zero_weights_are_skipped_collapsed_directions_kept_and_overflowing_positions_rejected(cpu):
    V, J = 256, 6
    rest = make_rest(V, frames=True, seed=3)
    rig = make_rig(V, 2, J, morph_normals=True, seed=4)
    mw, mats = pose_inputs(2, J, seed=5)
    mats[4] = 0.0
    mats[4, 3, 3] = 1.0           # collapses every direction (and position) to 0
    mats[5] = np.diag([1e30, 1e30, 1e30, 1]).astype(F)  # finite, but a position of more than 3e7 overflows the bound
    rest["positions"][200:] = (np.abs(rest["positions"][200:]) + F(1.0)) * F(1e9)
    rig["joints"][:40] = [4, 0, 0, 0]
    rig["weights"][:40] = [1, 0, -0.0, 0]      # joint 4 alone: 0 and -0 are skipped
    rig["joints"][200:] = [5, 1, 2, 3]
    rig["weights"][200:] = [1, 0, 0, -0.0]
    assert np.signbit(rig["weights"]).any()
    rejected, kept = _against_reference(cpu, rest, rig, mw, mats, "edge cases")
    assert rejected == 56 and kept >= 3 * 40
    p, n, t, b, _, _ = deform.reference_pose(rest, rig, mw, mats)
    assert (p[200:] == rest["positions"][200:]).all() and np.isfinite(p).all()
    for a, name in ((n, "normals"), (t, "tangents"), (b, "bitangents")):
        assert (a[:40] == rest[name][:40]).all(), name  # kept
    # a skipped joint's matrix is never read: NaNs there change nothing
    poisoned = mats.copy()
    poisoned[0] = np.nan
    rig2 = {k: (v.copy() if v is not None else None) for k, v in rig.items()}
    rig2["joints"][:] = [1, 0, 0, 0]
    rig2["weights"][:] = [0.5, 0.0, -0.0, 0.0]
    a = deform.reference_pose(rest, rig2, mw, mats)
    c = deform.reference_pose(rest, rig2, mw, poisoned)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], c[:4])) and np.isfinite(c[0]).all()
    _against_reference(cpu, rest, rig2, mw, poisoned, "NaN in a skipped joint")


# ---- properties of the reference alone
def test_identity_joints_return_the_rest_positions_bit_for_bit():
    V = 200
    rest = make_rest(V, frames=True, seed=1)
    rest["positions"][0] = [0.0, -0.0, 1e-40]  # a signed zero and a denormal among them
    rig = {"joints": np.zeros((V, 4), U32), "weights": np.tile(np.array([1, 0, 0, 0], F), (V, 1))}
    p, n, t, b, rejected, kept = deform.reference_pose(rest, rig, None, np.eye(4, dtype=F)[None])
    assert (p == rest["positions"]).all() and p[1:].tobytes() == rest["positions"][1:].tobytes()  # (x + 0 is x, except that -0 + 0 is +0)
    assert (rejected, kept) == (0, 0)
    for a, name in ((n, "normals"), (t, "tangents"), (b, "bitangents")):
        assert np.abs(a - meshprep.normalize(rest[name])).max() == 0, name


def test_an_exact_quarter_turn_rotates_exactly():
    pos, _, idx = cube24()
    nrm, _, _, _ = meshprep.reference(pos, idx, params=meshprep.params(weld=0))  # the faces' axes: entries 0 and +-1
    turn = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)  # x -> y, y -> -x
    rig = {"joints": np.zeros((24, 4), U32), "weights": np.tile(np.array([1, 0, 0, 0], F), (24, 1))}
    p, n, _, _, rejected, kept = deform.reference_pose({"positions": pos, "normals": nrm}, rig, None, turn[None])
    assert (p == np.stack([-pos[:, 1], pos[:, 0], pos[:, 2]], axis=-1)).all()
    assert (n == np.stack([-nrm[:, 1], nrm[:, 0], nrm[:, 2]], axis=-1)).all() and (rejected, kept) == (0, 0)


def test_a_morph_weight_of_one_gives_rest_plus_delta():
    V = 100
    rest = make_rest(V, frames=False, seed=2)
    rig = make_rig(V, 1, 0, morph_normals=False, seed=3)
    p, n, t, b, _, _ = deform.reference_pose(rest, rig, np.ones(1, F), None)
    assert p.tobytes() == (rest["positions"] + rig["morph_positions"][0]).astype(F).tobytes()
    assert n is None and t is None and b is None  # nothing but the positions is written


def test_default_params_and_the_parameter_check():
    p = deform.default_params()
    assert (p.regenerate, p.weight, p.weld, list(p.reserved)) == (0, 0, 1, [0] * 5)
    r = deform.default_params()
    r.reserved[1] = 1
    for q in (deform.params(regenerate=4), deform.params(regenerate=2), deform.params(weight=3), deform.params(weld=2), r):
        with pytest.raises(ValueError):
            deform.regenerate({"positions": np.zeros((3, 3), F)}, np.arange(3, dtype=U32), params=q)
