"""tools/meshprep_time.py [calls=5] — GPU box: what mesh preparation (include/hrcore_mesh.h) costs and what it saves.

For scenes.terrain(1000, 500) (1 M triangles over 501,501 shared vertices) and triangle_soup(1_000_000) (3 M unshared vertices, the
weld's worst case for sorting) prints lines starting MESHPREP_BUYS:
  the wall time of Engine.prepare_mesh for want = NORMALS and for NORMALS | TANGENTS (one warm-up call, then the median of `calls`),
  upload and download inside it, since the caller pays for them;
  heatray_amd.meshprep.reference's wall time on this machine's CPUs (numpy), the host-side pass a caller would write instead;
  scene_info().build_ms of the same mesh, for scale.
(Per-kernel times are not printed: the context's kernel timers cover the render stages only; a kernel trace of this script gives them.)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from heatray_amd import _ffi as ffi
from heatray_amd import core, meshprep, scenes

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BOTH = ffi.HR_MESH_WANT_NORMALS | ffi.HR_MESH_WANT_TANGENTS


def wall(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


for name, sc in (("terrain(1000, 500)", scenes.terrain(1000, 500, width=64, height=36)), ("triangle_soup(1_000_000)", scenes.triangle_soup(1_000_000, width=64, height=36))):
    # the scene's meshes as one (the soup comes as one mesh per material)
    base = np.cumsum([0] + [len(me.positions) for me in sc.meshes[:-1]])
    m = scenes.MeshData(np.concatenate([me.positions for me in sc.meshes]), None, np.concatenate([me.indices + np.uint32(b) for me, b in zip(sc.meshes, base)]),
                        uvs=np.concatenate([me.uvs for me in sc.meshes]) if all(me.uvs is not None for me in sc.meshes) else None)
    uvs = m.uvs if m.uvs is not None else np.random.default_rng(1).uniform(0, 1, (len(m.positions), 2)).astype(np.float32)
    eng = core.create_engine()
    times = {}
    for label, want in (("normals", ffi.HR_MESH_WANT_NORMALS), ("normals + tangents", BOTH)):
        p = meshprep.params(want=want)
        call = lambda: eng.prepare_mesh(m.positions, m.indices, uvs=uvs if want & 2 else None, params=p)
        call()  # warm: the scratch and the staging ring are made
        times[label] = wall(call, calls)
    result = eng.mesh_last()
    t0 = time.perf_counter()
    ref = meshprep.reference(m.positions, m.indices, uvs=uvs, params=meshprep.params(want=BOTH))
    ref_ms = (time.perf_counter() - t0) * 1e3
    got = eng.prepare_mesh(m.positions, m.indices, uvs=uvs, params=meshprep.params(want=BOTH))
    exact = all(a.tobytes() == b.tobytes() for a, b in zip(got, ref[:3])) and result == ref[3]
    eng.add_mesh(m.positions, got[0], m.indices, uvs=uvs, tangents=got[1], bitangents=got[2])
    eng.commit()
    build_ms = eng.scene_info().build_ms
    print(f"MESHPREP_BUYS {name}: {len(m.positions)} vertices, {result['triangles']} triangles, {result['weld_groups']} groups, max valence {result['max_valence']}; "
          f"prepare_mesh normals {times['normals']:.2f} ms, normals + tangents {times['normals + tangents']:.2f} ms (wall, median of {calls}, upload and download inside); "
          f"meshprep.reference (numpy, normals + tangents) {ref_ms:.0f} ms = {ref_ms / times['normals + tangents']:.0f} x; tree build {build_ms:.2f} ms; "
          f"device == reference: {exact}")
    eng.close()
