"""tools/deform_time.py [calls=7] — GPU box: what moving a resident mesh's vertices costs (include/hrcore_deform.h) against removing and
adding the mesh again.

For scenes.terrain(1000, 500) (1 M triangles, 501,501 vertices) and scenes.terrain(256, 256) (66,049 vertices) prints lines starting
DEFORM_TIME with wall milliseconds (one warm-up, then the median of `calls`; every timed sequence ends in hr_scene_commit, which waits for
the device) of
  the status quo: prepare_mesh(normals + tangents) + remove_mesh + add_mesh + commit, on the library HRCORE_PARENT names (an earlier
      build, e.g. build_variants/libhrcore_parent.so from tools/build_variant.sh in a checkout of the parent commit), in a child process
      of this one; "not measured" without it;
  update_mesh + commit;  update_mesh(regenerate = 3) + commit;
  deform_pose + commit with regenerate = 0 and 3 (a rig of 2 morphs with normals and 64 joints);
and the bytes one pose moves (what k_deform_pose reads and writes once, computed from the shapes).

tools/deform_time.py --pose-only N: N poses of each mesh and nothing else, to be run under `rocprofv3 --kernel-trace`;
tools/deform_time.py --trace FILE_kernel_trace.csv: that trace's kernels by name, mean microseconds, and k_deform_pose's bytes per second."""
import csv
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from heatray_amd import _ffi as ffi
from heatray_amd import core, meshprep, scenes

F = np.float32
BOTH = ffi.HR_MESH_WANT_NORMALS | ffi.HR_MESH_WANT_TANGENTS
K, J = 2, 64
MESHES = (("terrain(1000, 500)", 1000, 500), ("terrain(256, 256)", 256, 256))


def wall(fn, n):
    fn()  # warm: scratch, staging ring, code objects
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def mesh_of(nx, ny):
    m = scenes.terrain(nx, ny, width=64, height=36).meshes[0]
    rng = np.random.default_rng(1)
    moved = (m.positions + rng.normal(size=m.positions.shape) * 0.002).astype(F)
    return m, moved


def rig_of(V):
    """2 morphs with normals, 64 joints laid out along x so that neighbouring vertices name the same joints"""
    rng = np.random.default_rng(2)
    dP, dN = (0.01 * rng.normal(size=(K, V, 3))).astype(F), (0.01 * rng.normal(size=(K, V, 3))).astype(F)
    col = (np.arange(V) * J // V).astype(np.uint32)
    joints = np.stack([col, np.minimum(col + 1, J - 1), col, col], axis=1).astype(np.uint32)
    weights = np.tile(np.array([0.6, 0.4, 0.0, 0.0], F), (V, 1))
    mats = np.tile(np.eye(4, dtype=F), (J, 1, 1))
    mats[:, :3, 3] = 0.001 * rng.normal(size=(J, 3))
    return dict(morph_positions=dP, morph_normals=dN, joints=joints, weights=weights), rng.uniform(0, 1, K).astype(F), mats


def pose_bytes(V, frames=True):
    """what one k_deform_pose reads and writes once: rest arrays, deltas, joints and weights, outputs (the matrices are cache traffic)"""
    arrays = 4 if frames else 2
    return V * (12 * arrays + K * 24 + 32 + 12 * arrays)


def status_quo(calls):
    for name, nx, ny in MESHES:
        m, moved = mesh_of(nx, ny)
        eng = core.create_engine()
        p = meshprep.params(want=BOTH)
        n, t, b = eng.prepare_mesh(m.positions, m.indices, uvs=m.uvs, params=p)
        state = {"gid": eng.add_mesh(m.positions, n, m.indices, uvs=m.uvs, tangents=t, bitangents=b)}
        eng.commit()

        def again():
            n, t, b = eng.prepare_mesh(moved, m.indices, uvs=m.uvs, params=p)
            eng.remove_mesh(state["gid"])
            state["gid"] = eng.add_mesh(moved, n, m.indices, uvs=m.uvs, tangents=t, bitangents=b)
            eng.commit()
        print(f"STATUS_QUO {name}: {wall(again, calls):.3f}")
        eng.close()


def bound_engine(m):
    eng = core.create_engine()
    z = np.zeros_like(m.positions)
    gid = eng.add_mesh(m.positions, m.normals, m.indices, uvs=m.uvs, tangents=z, bitangents=z)
    eng.update_mesh(gid, m.positions, params=ffi.DeformParams(3, 0, 1))  # the frames the poses start from
    eng.commit()
    rig, mw, mats = rig_of(len(m.positions))
    eng.deform_bind(gid, n_joints=J, **rig)
    return eng, gid, mw, mats


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        rows = list(csv.DictReader(open(sys.argv[2])))
        by = {}
        for r in rows:
            by.setdefault(r["Kernel_Name"].split("(")[0].replace("void ", "").replace("hr::", ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for k in sorted(by, key=lambda k: -sum(by[k])):
            if k.startswith(("k_deform", "k_mesh")):
                print(f"DEFORM_TRACE {k}: {len(by[k])} launches, mean {statistics.mean(by[k]):.1f} us, median {statistics.median(by[k]):.1f} us")
        # every regeneration in the trace (k_mesh_face .. k_mesh_finish, in launch order) and the corner sort's part of it (the launches
        # between k_mesh_face and k_mesh_ranges): what caching the sorted corners per mesh would save, the sort depending on the indices alone
        ordered = sorted(rows, key=lambda r: int(r["Start_Timestamp"]))
        names = [r["Kernel_Name"].split("(")[0].replace("void ", "").replace("hr::", "") for r in ordered]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in ordered]
        faces = [i for i, k in enumerate(names) if k == "k_mesh_face"]
        for (name, _, _), i in zip(MESHES, faces):
            j, e = names.index("k_mesh_ranges", i), names.index("k_mesh_finish", i)
            total, sort = sum(t for k, t in zip(names[i:e + 1], us[i:e + 1]) if k.startswith("k_mesh")), sum(t for k, t in zip(names[i + 1:j], us[i + 1:j]) if k.startswith("k_mesh"))
            print(f"DEFORM_TRACE regeneration of {name}: its kernels {total:.1f} us, of which the corner sort {sort:.1f} us = {100 * sort / total:.0f} %")
        # the launches alternate between the two meshes' sizes: the larger half is the 1 M-triangle terrain's
        pose = sorted(by.get("k_deform_pose", []))
        if pose:
            for (name, nx, ny), us in zip(MESHES, (pose[len(pose) // 2:], pose[:len(pose) // 2])):
                V = (nx + 1) * (ny + 1)
                t = statistics.median(us)
                print(f"DEFORM_TRACE k_deform_pose on {name}: median {t:.1f} us for {pose_bytes(V) / 1e6:.1f} MB = {pose_bytes(V) / t / 1e6:.2f} TB/s")
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--pose-only":
        for name, nx, ny in MESHES:
            m, _ = mesh_of(nx, ny)
            eng, gid, mw, mats = bound_engine(m)
            for _ in range(int(sys.argv[2])):
                eng.deform_pose(gid, morph_weights=mw, joint_matrices=mats)
            eng.close()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--status-quo":
        status_quo(int(sys.argv[2]))
        return
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    quo = {}
    parent = os.environ.get("HRCORE_PARENT")
    if parent and os.path.exists(parent):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--status-quo", str(calls)], env={**os.environ, "HRCORE_LIB": os.path.abspath(parent)},
                             capture_output=True, text=True, timeout=300)
        for line in out.stdout.splitlines():
            if line.startswith("STATUS_QUO "):
                quo[line[len("STATUS_QUO "):].rsplit(": ", 1)[0]] = float(line.rsplit(": ", 1)[1])
        if not quo:
            print("status quo child failed:", out.stderr[-500:])
    for name, nx, ny in MESHES:
        m, moved = mesh_of(nx, ny)
        V = len(m.positions)
        eng, gid, mw, mats = bound_engine(m)
        both = [moved, m.positions]
        turn = {"i": 0}

        def update(regen):
            turn["i"] ^= 1
            eng.update_mesh(gid, both[turn["i"]], params=ffi.DeformParams(regen, 0, 1))
            eng.commit()

        def pose(regen):
            turn["i"] ^= 1
            eng.deform_pose(gid, morph_weights=mw * F(0.5 + turn["i"]), joint_matrices=mats, params=ffi.DeformParams(regen, 0, 1))
            eng.commit()
        t = {"update": wall(lambda: update(0), calls), "update3": wall(lambda: update(3), calls), "pose": wall(lambda: pose(0), calls), "pose3": wall(lambda: pose(3), calls)}
        refit = eng.scene_info()
        q = f"{quo[name]:.2f} ms" if name in quo else "not measured"
        print(f"DEFORM_TIME {name}: {V} vertices, {m.indices.size // 3} triangles; status quo (prepare + remove + add + commit, parent library) {q}; "
              f"update_mesh + commit {t['update']:.2f} ms; update_mesh(regenerate=3) + commit {t['update3']:.2f} ms; deform_pose + commit {t['pose']:.2f} ms; "
              f"deform_pose(regenerate=3) + commit {t['pose3']:.2f} ms (wall, median of {calls}); last commit refitted = {refit.refitted}, build_ms {refit.build_ms:.2f}; "
              f"one pose moves {pose_bytes(V) / 1e6:.1f} MB ({K} morphs with normals, {J} joints, tangent frames)")
        eng.close()


main()
