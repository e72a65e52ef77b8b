"""Deformable meshes on the device (include/hrcore_deform.h): an update writes what it is given, into any block layout; a regeneration
is hr_mesh_prepare's, byte for byte; a pose is heatray_amd.deform.reference's; a frame does not know how its mesh got there (update, pose
or a fresh add_mesh, on the device and on the CPU oracle); commits refit and rebuild when the guard says so; every call is deterministic
across contexts and context groups; bindings die with their meshes; and every refusal names its cause and changes nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from deform_cases import F, U32, make_rig, pose_inputs, rigid
from device_support import host_tables, same
from heatray_amd import _ffi as ffi
from heatray_amd import core, deform, meshprep, scenes
from mesh_cases import BOTH, WEIGHTS, cube24, fan, given_normals, grid
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

NAMES = ("positions", "normals", "uvs", "tangents", "bitangents", "colors")
BOUNDARY = (1, 63, 64, 65, 255, 256, 257)  # vertex counts round a wave and round the kernels' 256-lane workgroups


@pytest.fixture(scope="module")
def eng():
    e = core.create_engine()
    yield e
    e.close()


def same3(got, want, what):
    same(np.ascontiguousarray(got, F).reshape(len(got), 1, -1), np.ascontiguousarray(want, F).reshape(len(want), 1, -1), what)


def block(e, gid, names=NAMES[:5]):
    """the mesh block's attributes as the device holds them"""
    return {n: e.mesh_attribute(gid, NAMES.index(n)) for n in names}


def full_mesh(pos, uv, idx, mode=ffi.HR_TRIANGLES, seed=0):
    """every attribute a mesh can have: prepared normals and frames, random colours"""
    n, t, b, _ = meshprep.reference(pos, idx, uvs=uv, mode=mode, params=meshprep.params(want=BOTH))
    col = np.random.default_rng(seed).uniform(0, 1, pos.shape).astype(F)
    return {"positions": pos, "normals": n, "uvs": uv, "tangents": t, "bitangents": b, "colors": col}


def add(e, m, idx, mode=ffi.HR_TRIANGLES, names=NAMES):
    kw = {n: m[n] for n in names if n not in ("positions", "normals")}
    return e.add_mesh(m["positions"], m["normals"], idx, mode=mode, **kw)


def small_meshes():
    p, _, uv, idx = scenes.plane_strip(15, 15)
    return [("grid(13, 7)",) + grid(13, 7), ("fan(70)",) + fan(70) + (ffi.HR_TRIANGLES,), ("cube24",) + cube24() + (ffi.HR_TRIANGLES,),
            ("plane_strip",) + (p, uv, idx, ffi.HR_TRIANGLE_STRIP)]


def random_mesh(V, seed):
    """V vertices, about 2 V triangles with random indices (V = 1: one degenerate triangle), some coincident positions to weld"""
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(V, 3)).astype(F)
    pos[rng.integers(0, V, V // 8)] = pos[rng.integers(0, V, V // 8)]
    return pos, rng.uniform(0, 1, (V, 2)).astype(F), rng.integers(0, V, 3 * max(1, 2 * V)).astype(U32)


def odd(a, stride):
    """a copy of `a` whose rows lie `stride` bytes apart (no multiple of four)"""
    raw = np.zeros(len(a) * stride + 16, np.uint8)
    view = np.ndarray(a.shape, F, buffer=raw.data, strides=(stride, 4))
    view[...] = a
    return view


def add_raw(e, m, idx, mode=ffi.HR_TRIANGLES):
    """hr_geom_add with the arrays' own strides (add_mesh packs them)"""
    arrays = [ffi._strided(m.get(n), 2 if n == "uvs" else 3) for n in NAMES]
    d = ffi.MeshDesc()
    d.positions, d.normals, d.uvs, d.tangents, d.bitangents, d.colors = (ffi._ptr(a) for a, _ in arrays)
    d.position_stride, d.normal_stride, d.uv_stride, d.tangent_stride, d.bitangent_stride, d.color_stride = (s for _, s in arrays)
    idx = np.ascontiguousarray(idx, U32)
    d.n_vertices, d.indices, d.n_indices, d.mode = len(m["positions"]), ffi._ptr(idx, ffi.u32p), idx.size, mode
    d.world_from_entity = (C.c_float * 16)(*np.eye(4, dtype=F).reshape(-1))
    d.is_occluder = 1
    gid = C.c_int32(-1)
    e._call("geom_add", C.byref(d), C.byref(gid))
    e.__dict__.setdefault("_mesh_vertices", {})[gid.value] = d.n_vertices  # (what add_mesh notes for mesh_attribute)
    return gid.value


# ---- 1. update writes what it is given
def test_update_writes_what_it_is_given_into_every_layout(eng):
    eng.clear_scene()
    pos, uv, idx, _ = grid(13, 7)
    m = full_mesh(pos, uv, idx)
    V = len(pos)
    tight = add(eng, m, idx)
    buf = np.zeros((V, 9), F)  # one interleaved vertex buffer: positions, a gap, normals, uvs
    buf[:, 0:3], buf[:, 4:7], buf[:, 7:9] = pos, m["normals"], uv
    inter = eng.add_mesh_strided(buf, 0, 4, 7, 9, idx)
    strided = add_raw(eng, {"positions": odd(pos, 13), "normals": odd(m["normals"], 17), "uvs": odd(uv, 11)}, idx)
    rng = np.random.default_rng(5)
    for gid, names in ((tight, NAMES), (inter, NAMES[:3]), (strided, NAMES[:3])):
        before = block(eng, gid, names)
        for n in names:
            same3(before[n], m[n], f"mesh {gid} as added: {n}")
        new_p = (pos + rng.normal(size=pos.shape) * 0.01).astype(F)
        new_n = (m["normals"] + rng.normal(size=pos.shape) * 0.1).astype(F)
        r = eng.update_mesh(gid, new_p, normals=new_n, with_result=True)
        assert r == dict(vertices=V, triangles=idx.size // 3, rejected_vertices=0, kept_directions=0, regenerated=0, posed=0, mesh=dict.fromkeys(meshprep.RESULT_KEYS, 0))
        assert eng.deform_last() == r
        after = block(eng, gid, names)
        same3(after["positions"], new_p, f"mesh {gid}: positions"), same3(after["normals"], new_n, f"mesh {gid}: normals")
        for n in names[2:]:
            same3(after[n], m[n], f"mesh {gid}: {n} was not sent")
        # an update that is itself interleaved, and one with strides that are no multiple of four
        ib = np.zeros((V, 7), F)
        ib[:, 0:3], ib[:, 3:5], ib[:, 5:7] = pos * F(1.5), uv * F(0.5), 0.25
        eng.update_mesh(gid, ib[:, 0:3], uvs=ib[:, 3:5])
        assert ib[:, 0:3].strides == (28, 4)
        after = block(eng, gid, names)
        same3(after["positions"], pos * F(1.5), f"mesh {gid}: interleaved update"), same3(after["uvs"], uv * F(0.5), f"mesh {gid}: interleaved update, uvs")
        same3(after["normals"], new_n, f"mesh {gid}: normals stay")
        eng.update_mesh(gid, odd(pos, 13), normals=odd(m["normals"], 19), uvs=odd(uv, 9))
        after = block(eng, gid, names)
        for n in names[:3]:
            same3(after[n], m[n], f"mesh {gid}: oddly strided update: {n}")
    # all six attributes in one call (two launches of the scatter)
    eng.update_mesh(tight, *(np.ascontiguousarray(m[n][::-1]) for n in ("positions", "normals", "uvs", "tangents", "bitangents", "colors")))
    for n, a in block(eng, tight, NAMES).items():
        same3(a, m[n][::-1], f"six attributes: {n}")


# ---- 2. regeneration is hr_mesh_prepare's
@pytest.fixture(scope="module")
def terrain256():
    m = scenes.terrain(256, 256, width=64, height=36).meshes[0]
    rng = np.random.default_rng(7)
    new_p = (m.positions + rng.normal(size=m.positions.shape) * 0.002).astype(F)
    return m, new_p, meshprep.reference(new_p, m.indices, uvs=m.uvs, params=meshprep.params(want=BOTH))


def test_regeneration_is_mesh_prepares(eng, terrain256):
    eng.clear_scene()
    pos0, uv0, idx0, _ = grid(3, 2)
    prepared = eng.prepare_mesh(pos0, idx0, with_result=True)[3]
    rng = np.random.default_rng(11)
    for what, pos, uv, idx, mode in small_meshes():
        m = full_mesh(pos, uv, idx, mode)
        gid = add(eng, m, idx, mode)
        for weight in WEIGHTS:
            for weld in (1, 0):
                for regen in (1, 3):
                    new_p = (pos + rng.normal(size=pos.shape) * 0.02).astype(F)
                    r = eng.update_mesh(gid, new_p, params=deform.params(regen, weight, weld), with_result=True)
                    n, t, b, res = meshprep.reference(new_p, idx, uvs=uv, mode=mode, params=meshprep.params(weight, weld, regen))
                    tag = f"{what} weight={weight} weld={weld} regenerate={regen}"
                    got = block(eng, gid)
                    same3(got["positions"], new_p, tag), same3(got["normals"], n, tag + ": normals")
                    if regen == 3:
                        same3(got["tangents"], t, tag + ": tangents"), same3(got["bitangents"], b, tag + ": bitangents")
                    assert r["mesh"] == res and r["regenerated"] == regen, (tag, r["mesh"], res)
    m, new_p, (n, t, b, res) = terrain256
    mm = {"positions": m.positions, "normals": m.normals, "uvs": m.uvs, "tangents": np.zeros_like(m.positions), "bitangents": np.zeros_like(m.positions)}
    gid = add(eng, mm, m.indices, names=NAMES[:5])
    r = eng.update_mesh(gid, new_p, params=deform.params(3), with_result=True)
    got = block(eng, gid)
    same3(got["normals"], n, "terrain(256, 256): normals"), same3(got["tangents"], t, "terrain: tangents"), same3(got["bitangents"], b, "terrain: bitangents")
    assert r["mesh"] == res and res["max_valence"] == 6
    assert eng.mesh_last() == prepared  # (hr_mesh_last is hr_mesh_prepare's alone)


# ---- 3. pose is the reference's
def posed_against_reference(e, gid, rest, rig, mw, mats, idx, uv, mode=ffi.HR_TRIANGLES, params=None, what=""):
    """deform_pose on the bound mesh, held to deform.reference: the written attributes byte for byte, the others untouched, the result equal"""
    before = block(e, gid, [n for n in NAMES[:5] if n in rest or n == "uvs"])
    r = e.deform_pose(gid, morph_weights=mw, joint_matrices=mats, params=params, with_result=True)
    want, res = deform.reference(rest, rig, mw, mats, indices=idx, mode=mode, uvs=uv, params=params)
    after = block(e, gid, list(before))
    for n in before:
        same3(after[n], want.get(n, before[n]), f"{what}: {n}" + ("" if n in want else " (not written)"))
    assert r == res == e.deform_last(), (what, r, res)
    return want, res


@pytest.mark.parametrize("V", BOUNDARY)
def test_pose_at_the_lane_boundaries(eng, V):
    eng.clear_scene()
    pos, uv, idx = random_mesh(V, seed=V)
    for frames in (False, True):
        m = full_mesh(pos, uv, idx)
        m["normals"] = given_normals(pos, seed=V)  # unnormalised, a zero and a huge one among them
        names = NAMES[:5] if frames else NAMES[:3]
        gid = add(eng, m, idx, names=names)
        rest = {n: m[n] for n in names if n != "uvs"}
        for K, J, morph_normals in ((2, 5, True), (0, 300, False), (8, 0, True)):
            rig = make_rig(V, K, J, morph_normals, seed=V + K + J)
            mw, mats = pose_inputs(K, J, seed=V * 3 + K)
            eng.deform_bind(gid, n_joints=J, **rig)
            for regen in (0, 1) + ((3,) if frames else ()):
                posed_against_reference(eng, gid, rest, rig, mw, mats, idx, uv, params=deform.params(regen), what=f"V={V} frames={frames} K={K} J={J} regenerate={regen}")
            eng.update_mesh(gid, *(m[n] for n in names))  # back to the rest pose for the next bind


@pytest.mark.parametrize("K, J", [(k, j) for k in (0, 1, 8) for j in (0, 1, 300) if k or j])
def test_pose_with_every_kind_of_rig(eng, K, J):
    eng.clear_scene()
    for what, pos, uv, idx, mode in small_meshes():
        m = full_mesh(pos, uv, idx, mode)
        for frames in (True, False):
            names = NAMES[:5] if frames else NAMES[:3]
            gid = add(eng, m, idx, mode, names=names)
            rest = {n: m[n] for n in names if n != "uvs"}
            for morph_normals in ((False, True) if K else (False,)):
                rig = make_rig(len(pos), K, J, morph_normals, seed=K * 7 + J)
                mw, mats = pose_inputs(K, J, seed=K + J)
                eng.deform_bind(gid, n_joints=J, **rig)
                posed_against_reference(eng, gid, rest, rig, mw, mats, idx, uv, mode, what=f"{what} frames={frames} K={K} J={J} morph_normals={morph_normals}")
                eng.update_mesh(gid, *(m[n] for n in names))  # (the next bind's rest pose is the mesh as it stands)


def test_rejected_positions_and_kept_directions_through_finite_inputs(eng):
    eng.clear_scene()
    pos, uv, idx, _ = grid(13, 7)
    m = full_mesh(pos, uv, idx)
    V = len(pos)
    gid = add(eng, m, idx, names=NAMES[:5])
    rest = {n: m[n] for n in NAMES[:5] if n != "uvs"}
    rig = make_rig(V, 1, 4, True, seed=2)
    mw, mats = pose_inputs(1, 4, seed=3)
    mats[2] = 0.0
    mats[2, 3, 3] = 1.0                                    # a collapsing joint: every direction through it alone has length 0
    mats[3] = np.diag([1e30, 1e30, 1e30, 1]).astype(F)     # finite, and times a finite position past 3e37
    rig["joints"][:10], rig["weights"][:10] = [2, 0, 0, 0], [1, 0, -0.0, 0]
    rig["joints"][20:27], rig["weights"][20:27] = [3, 0, 0, 0], [1, 0, 0, 0]
    big = {**m, "positions": pos.copy()}
    big["positions"][20:27] = 1e9
    eng.update_mesh(gid, big["positions"])
    rest["positions"] = big["positions"]
    eng.deform_bind(gid, n_joints=4, **rig)
    want, res = posed_against_reference(eng, gid, rest, rig, mw, mats, idx, uv, what="edge cases")
    assert res["rejected_vertices"] == 7 and res["kept_directions"] >= 30
    assert (want["positions"][20:27] == 1e9).all() and (want["normals"][:10] == m["normals"][:10]).all() and np.isfinite(want["positions"]).all()


# ---- 4. the frame does not know how the mesh got there
def _normal_mapped_scene():
    sc = scenes.multi_material(width=64, height=36, passes=2, textured=True)
    rng = np.random.default_rng(9)
    bumps = np.concatenate([rng.uniform(0.2, 0.8, (16, 16, 2)), np.ones((16, 16, 1))], axis=-1).astype(F)
    sc.textures.append((bumps, ffi.HR_WRAP_REPEAT, ffi.HR_FILTER_LINEAR))
    for mid in (0, 1, 3):
        sc.materials[mid].normalmap = len(sc.textures) - 1
        sc.materials[mid].flags |= ffi.HR_MF_HAS_NORMALMAP
    for m in sc.meshes:
        m.normals, m.tangents, m.bitangents, _ = meshprep.reference(m.positions, m.indices, uvs=m.uvs, mode=m.mode, params=meshprep.params(want=BOTH))
    return sc


def test_the_frame_does_not_know_how_the_mesh_got_there(golden):
    sc = _normal_mapped_scene()
    which = 1  # the rough-metal sphere
    m = sc.meshes[which]
    V = len(m.positions)
    bump = (1.0 + 0.04 * np.sin(7 * m.positions[:, 0]) * np.cos(5 * m.positions[:, 1]))[:, None]
    moved = (m.positions + m.normals * (bump - 1.0)).astype(F)  # a few percent along the normals
    a = core.create_engine()
    sc.apply(a, lut=golden["multiscatter_lut"], tables=host_tables(sc))
    rng = np.random.default_rng(4)
    org = rng.uniform(-3, 3, (3000, 3)).astype(F)
    d = rng.normal(size=(3000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)

    def frame(e):
        e.clear()
        for s in range(2):
            e.render_pass(sc.options.pass_params(s))
        return e.readback(), e.debug_trace(org, d)

    first = frame(a)[0]
    turn = rigid(np.random.default_rng(1), 1, spread=0.05)
    rig = {"morph_positions": (moved - m.positions)[None], "morph_normals": None, "joints": np.zeros((V, 4), U32), "weights": np.tile(np.array([1, 0, 0, 0], F), (V, 1))}
    steps = [("update_mesh", lambda: a.update_mesh(which, moved, normals=m.normals)),
             ("deform_pose", lambda: (a.deform_bind(which, **rig), a.deform_pose(which, morph_weights=[0.5], joint_matrices=turn))),
             ("deform_pose with regenerate=3", lambda: a.deform_pose(which, morph_weights=[1.0], joint_matrices=turn, params=deform.params(3)))]
    for what, step in steps:
        step()
        a.commit()
        assert a.scene_info().refitted == 1, what
        fa, ha = frame(a)
        assert (fa != first).any(), what
        got = block(a, which)
        fresh = _normal_mapped_scene()
        fm = fresh.meshes[which]
        fm.positions, fm.normals, fm.tangents, fm.bitangents = got["positions"], got["normals"], got["tangents"], got["bitangents"]
        same3(got["uvs"], m.uvs, what + ": uvs")
        b, o = core.create_engine(), oracle_lib.engine()
        for e in (b, o):
            fresh.apply(e, lut=golden["multiscatter_lut"], tables=host_tables(fresh))
        (fb, hb), (fo, ho) = frame(b), frame(o)
        same(fa, fb, what + ": the deformed engine against a fresh one")
        assert_parity(fa, fo, what + ": against the oracle")
        assert ha.tobytes() == hb.tobytes() == ho.tobytes(), what
        b.close(), o.close()
        if what == "update_mesh":  # back to the rest pose: the bind that follows snapshots it
            a.update_mesh(which, m.positions, normals=m.normals)
    a.close()


# ---- 5. refit, and rebuild when the guard says so
def test_a_walk_of_deformations_refits_and_rebuilds():
    rng = np.random.default_rng(2027)
    sc = scenes.triangle_soup(6000, width=48, height=32, bounces=3, passes=8, n_materials=6)
    g = core.create_engine()
    sc.apply(g)
    cur = [m.positions.copy() for m in sc.meshes]
    refits = rebuilds = 0
    for step in range(30):
        gid = int(rng.integers(0, len(cur)))
        p = cur[gid]
        extent = float((p.max(0) - p.min(0)).max())
        if step % 7 == 3:  # every triangle of one mesh flung, rigidly, somewhere in a box many times the mesh's size
            cur[gid] = (p.reshape(-1, 3, 3) + rng.uniform(-8 * extent, 8 * extent, (len(p) // 3, 1, 3))).reshape(-1, 3).astype(F)
            kind = "scatter"
        else:              # per-vertex jitter of 1 % of the mesh's extent
            cur[gid] = (p + rng.uniform(-0.01 * extent, 0.01 * extent, p.shape)).astype(F)
            kind = "jitter"
        g.update_mesh(gid, cur[gid])
        g.commit()
        gi = g.scene_info()
        refits += int(gi.refitted)
        rebuilds += int(not gi.refitted)
        print(f"step {step} ({kind}, mesh {gid}): refitted {gi.refitted}, box_area_ratio {gi.box_area_ratio:.4f}")
        assert (abs(gi.box_area_ratio - 1.0) < 1e-3) if not gi.refitted else (0.0 < gi.box_area_ratio <= 1.25 * 1.001), (step, kind, gi.refitted, gi.box_area_ratio)
        fresh = core.create_engine()
        for m, p in zip(sc.meshes, cur):
            fresh.add_mesh(p, m.normals, m.indices, uvs=m.uvs, material_id=m.material_id, is_occluder=m.is_occluder)
        fresh.commit()
        fi = fresh.scene_info()
        assert list(gi.aabb_min) == list(fi.aabb_min) and list(gi.aabb_max) == list(fi.aabb_max) and gi.n_triangles == fi.n_triangles
        lo, hi = np.array(gi.aabb_min), np.array(gi.aabb_max)
        org = rng.uniform(lo - 0.2, hi + 0.2, (3000, 3)).astype(F)
        d = rng.uniform(lo, hi, (3000, 3)) - org
        d = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-20)).astype(F)
        hg, hf = g.debug_trace(org, d), fresh.debug_trace(org, d)
        assert hg.tobytes() == hf.tobytes(), f"step {step} ({kind}): {(hg != hf).sum()} of 3000 hits differ"
        fresh.close()
    g.close()
    assert refits >= 1 and rebuilds >= 1, (refits, rebuilds)


# ---- 6. determinism
def test_the_same_bytes_in_every_context_and_group(golden):
    pos, uv, idx, _ = grid(13, 7)
    m = full_mesh(pos, uv, idx)
    V = len(pos)
    rig = make_rig(V, 2, 9, True, seed=1)
    mw, mats = pose_inputs(2, 9, seed=2)
    new_p = (pos * F(1.1)).astype(F)
    sc = _normal_mapped_scene()
    sv = len(sc.meshes[1].positions)
    srig = make_rig(sv, 1, 3, False, seed=3)
    smw, smats = pose_inputs(1, 3, seed=4)
    srig["morph_positions"] *= F(0.3)
    results = []
    engines = [core.create_engine(), core.create_engine(), core.create_group(device_ids=[0, 0]), core.create_group(device_ids=[0, 0, 0])]
    for e in engines:
        sc.apply(e, lut=golden["multiscatter_lut"], tables=host_tables(sc))
        gid = add(e, m, idx, names=NAMES[:5])
        out = []
        r = e.update_mesh(gid, new_p, normals=m["normals"][::-1].copy(), with_result=True)
        out.append((block(e, gid), r))
        r = e.update_mesh(gid, new_p, params=deform.params(3), with_result=True)
        out.append((block(e, gid), r))
        e.update_mesh(gid, *(m[n] for n in NAMES[:5]))
        e.deform_bind(gid, n_joints=9, **rig)
        r = e.deform_pose(gid, morph_weights=mw, joint_matrices=mats, params=deform.params(1), with_result=True)
        out.append((block(e, gid), r))
        assert r == e.deform_last()
        # and a frame after a pose of the scene's sphere
        e.deform_bind(1, n_joints=3, **srig)
        e.deform_pose(1, morph_weights=smw, joint_matrices=smats)
        e.commit()
        e.clear()
        for s in range(2):
            e.render_pass(sc.options.pass_params(s))
        results.append((out, e.readback()))
    want, res = deform.reference({n: m[n] for n in NAMES[:5] if n != "uvs"}, rig, mw, mats, indices=idx, uvs=uv, params=deform.params(1))
    for k, (out, fr) in enumerate(results):
        for (blk, r), (blk0, r0) in zip(out, results[0][0]):
            assert r == r0, k
            for n in blk:
                assert blk[n].tobytes() == blk0[n].tobytes(), (k, n)
        for n in want:
            assert out[2][0][n].tobytes() == want[n].tobytes(), (k, n)
        assert out[2][1] == res
        same(fr, results[0][1], f"engine {k}: the frame after a pose")
    for e in engines:
        e.close()


# ---- 7. lifetimes
def test_lifetimes_of_bindings_and_the_commit_rule(eng):
    eng.clear_scene()
    pos, uv, idx, _ = grid(13, 7)
    m = full_mesh(pos, uv, idx)
    V = len(pos)
    rig = make_rig(V, 1, 2, False, seed=1)
    mw, mats = pose_inputs(1, 2, seed=2)
    fresh = core.create_engine()
    with pytest.raises(ffi.EngineError, match="no mesh has been updated or posed"):
        fresh.deform_last()
    fresh.close()
    gid = add(eng, m, idx, names=NAMES[:5])
    with pytest.raises(ffi.EngineError, match="the mesh is not bound"):
        eng.deform_pose(gid, morph_weights=mw, joint_matrices=mats)
    with pytest.raises(ffi.EngineError, match="the mesh is not bound"):
        eng.deform_unbind(gid)
    eng.deform_bind(gid, n_joints=2, **rig)
    eng.deform_unbind(gid)
    with pytest.raises(ffi.EngineError, match="the mesh is not bound"):
        eng.deform_pose(gid, morph_weights=mw, joint_matrices=mats)
    # bind, update, pose: the pose starts from the rest pose, not from the update
    eng.deform_bind(gid, n_joints=2, **rig)
    eng.deform_bind(gid, n_joints=2, **rig)  # (a second bind replaces the first)
    eng.update_mesh(gid, (pos * F(3.0)).astype(F), normals=-m["normals"])
    rest = {n: m[n] for n in NAMES[:5] if n != "uvs"}
    posed_against_reference(eng, gid, rest, rig, mw, mats, idx, uv, what="bind, update, pose")
    # remove_mesh of a bound mesh, then an add_mesh that reuses nothing of it
    eng.remove_mesh(gid)
    with pytest.raises(ffi.EngineError, match="bad geom id"):
        eng.deform_pose(gid, morph_weights=mw, joint_matrices=mats)
    p2, uv2, i2 = fan(70)
    m2 = full_mesh(p2, uv2, i2)
    g2 = add(eng, m2, i2, names=NAMES[:5])
    with pytest.raises(ffi.EngineError, match="the mesh is not bound"):
        eng.deform_pose(g2, morph_weights=mw, joint_matrices=mats)
    for n, a in block(eng, g2).items():
        same3(a, m2[n], "the mesh added after a removal: " + n)
    # clear_scene drops bindings
    eng.deform_bind(g2, morph_positions=np.zeros((1, len(p2), 3), F))
    eng.clear_scene()
    g3 = add(eng, m2, i2, names=NAMES[:5])
    with pytest.raises(ffi.EngineError, match="the mesh is not bound"):
        eng.deform_pose(g3, morph_weights=[1.0])
    # after an update and before a commit there is no scene to render, as after set_transform
    sc = scenes.multi_material(width=64, height=36, passes=2)
    e = core.create_engine()
    sc.apply(e)
    e.render_pass(sc.options.pass_params(0))
    e.set_transform(1, scenes._translate(0, 0.1, 0))
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        e.render_pass(sc.options.pass_params(1))
    e.commit()
    e.render_pass(sc.options.pass_params(1))
    e.update_mesh(1, sc.meshes[1].positions * F(1.05))
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        e.render_pass(sc.options.pass_params(2))
    e.commit()
    assert e.scene_info().refitted == 1
    e.render_pass(sc.options.pass_params(2))
    e.deform_bind(1, morph_positions=np.full((1, len(sc.meshes[1].positions), 3), 0.01, F))
    e.deform_pose(1, morph_weights=[1.0])
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        e.render_pass(sc.options.pass_params(3))
    e.commit()
    e.render_pass(sc.options.pass_params(3))
    assert np.isfinite(e.readback()).all()
    e.close()  # (with a live binding: hr_ctx_destroy frees it)


# ---- 8. refusals
def test_every_refusal_names_its_cause_and_changes_nothing(eng):
    eng.clear_scene()
    pos, uv, idx, _ = grid(3, 2)
    m = full_mesh(pos, uv, idx)
    V = len(pos)
    gid = add(eng, m, idx, names=NAMES[:5])                   # everything but colours
    bare = add(eng, m, idx, names=NAMES[:2])                  # positions and normals only
    rig = make_rig(V, 2, 3, True, seed=1)
    mw, mats = pose_inputs(2, 3, seed=2)
    eng.deform_bind(gid, n_joints=3, **rig)
    last = eng.update_mesh(gid, pos, with_result=True)
    held = block(eng, gid)

    def unchanged():
        for n, a in block(eng, gid).items():
            assert a.tobytes() == held[n].tobytes(), n
        assert eng.deform_last() == last

    def desc(**arrays):
        d = ffi.MeshDesc()
        keep = [np.ascontiguousarray(a, F) for a in arrays.values()]
        for n, a in zip(arrays, keep):
            setattr(d, n, ffi._ptr(a))
        d.n_vertices = V
        return d, keep

    def update_refused(match, g=gid, params=None, null_desc=False, **fields):
        d, keep = desc(positions=pos)
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep.append(np.ascontiguousarray(v, F))
                v = ffi._ptr(keep[-1])
            setattr(d, k, v)
        with pytest.raises(ffi.EngineError, match=match):
            eng._feature_call("deform", "geom_update", C.c_int32(g), None if null_desc else C.byref(d), C.byref(params) if params is not None else None, None)
        unchanged()

    update_refused("bad geom id", g=99)
    update_refused("bad geom id", g=-1)
    update_refused("null desc", null_desc=True)
    update_refused("null positions", positions=ffi.f32p())
    update_refused("n_vertices = 11 but the mesh has 12", n_vertices=V - 1)
    update_refused("the mesh has no colors", colors=pos)
    update_refused("the mesh has no tangents", g=bare, tangents=pos)
    update_refused("the mesh has no uvs", g=bare, uvs=uv)
    update_refused("attribute stride smaller than the attribute", position_stride=8)
    update_refused("attribute stride smaller than the attribute", uvs=uv, uv_stride=4)
    update_refused("attribute stride smaller than the attribute", normals=pos, normal_stride=-12)
    for bad in (np.nan, np.inf, 3.2e37):
        q = pos.copy()
        q[5, 1] = bad
        update_refused("vertex positions must be finite", positions=q)
    update_refused("unknown regenerate 4", params=deform.params(4))
    update_refused("regenerate TANGENTS needs NORMALS", params=deform.params(2))
    update_refused("unknown weight 3", params=deform.params(1, weight=3))
    update_refused("weld = 2 is neither 0 nor 1", params=deform.params(1, weld=2))
    r = deform.default_params()
    r.reserved[3] = 1
    update_refused(r"reserved\[3\] must be 0", params=r)
    update_refused("normals are both given and regenerated", params=deform.params(1), normals=pos)
    update_refused("tangents are both given and regenerated", params=deform.params(3), tangents=pos)
    update_refused("tangents are both given and regenerated", params=deform.params(3), bitangents=pos)
    update_refused("regenerate TANGENTS needs a mesh with uvs, tangents and bitangents", g=bare, params=deform.params(3))

    def attribute_refused(match, g, attribute, null_out=False):
        out = np.empty((V, 3), F)
        with pytest.raises(ffi.EngineError, match=match):
            eng._feature_call("deform", "geom_get_attribute", C.c_int32(g), C.c_int32(attribute), ffi.f32p() if null_out else ffi._ptr(out))
        unchanged()

    attribute_refused("bad geom id", 99, 0)
    attribute_refused("unknown attribute 6", gid, 6)
    attribute_refused("unknown attribute -1", gid, -1)
    attribute_refused("the mesh has no colors", gid, ffi.HR_GEOM_COLORS)
    attribute_refused("null output", gid, 0, null_out=True)

    def bind_refused(match, g=bare, null_rig=False, **fields):
        keep = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in rig.items()}
        b = ffi.DeformRig()
        b.morph_positions, b.morph_normals, b.weights = (ffi._ptr(keep[k]) for k in ("morph_positions", "morph_normals", "weights"))
        b.joints, b.n_morph, b.n_joints = ffi._ptr(keep["joints"], ffi.u32p), 2, 3
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                keep[k + "_new"] = v
                v = ffi._ptr(v, ffi.u32p if v.dtype == U32 else ffi.f32p)
            if k == "reserved":
                b.reserved[v] = 1
            else:
                setattr(b, k, v)
        with pytest.raises(ffi.EngineError, match=match):
            eng._feature_call("deform", "deform_bind", C.c_int32(g), None if null_rig else C.byref(b))
        unchanged()
        with pytest.raises(ffi.EngineError, match="the mesh is not bound"):  # (the refused bind bound nothing)
            eng.deform_unbind(bare)

    bind_refused("bad geom id", g=99)
    bind_refused("null rig", null_rig=True)
    bind_refused("n_morph = 9 is outside", n_morph=9)
    bind_refused("n_morph = -1 is outside", n_morph=-1)
    bind_refused("n_joints = 1025 is outside", n_joints=1025)
    bind_refused("a rig needs morphs or joints", n_morph=0, n_joints=0, morph_positions=ffi.f32p(), morph_normals=ffi.f32p(), joints=ffi.u32p(), weights=ffi.f32p())
    bind_refused("null morph_positions", morph_positions=ffi.f32p())
    bind_refused("morph_positions without morphs", n_morph=0)
    bind_refused("morph_normals without morphs", n_morph=0, morph_positions=ffi.f32p())
    bind_refused("null joints", joints=ffi.u32p())
    bind_refused("null weights", weights=ffi.f32p())
    bind_refused("joints or weights without joints", n_joints=0)
    bad_j = rig["joints"].copy()
    bad_j[7, 2] = 3
    bind_refused("joint index out of range", joints=bad_j)
    for field, text in (("weights", "weights must be finite"), ("morph_positions", "morph deltas must be finite"), ("morph_normals", "morph deltas must be finite")):
        for bad in (np.nan, -np.inf, 3.2e37):
            q = rig[field].copy()
            q.reshape(-1)[5] = bad
            bind_refused(text, **{field: q})
    bind_refused(r"reserved\[2\] must be 0", reserved=2)

    def pose_refused(match, g=gid, params=None, w=mw, j=mats):
        jm = None if j is None else np.ascontiguousarray(np.transpose(j, (0, 2, 1)), F)
        wm = None if w is None else np.ascontiguousarray(w, F)
        with pytest.raises(ffi.EngineError, match=match):
            eng._feature_call("deform", "deform_pose", C.c_int32(g), ffi._ptr(wm), ffi._ptr(jm), C.byref(params) if params is not None else None, None)
        unchanged()

    pose_refused("bad geom id", g=99)
    pose_refused("the mesh is not bound", g=bare)
    pose_refused("null morph_weights", w=None)
    pose_refused("null joint_matrices", j=None)
    for bad in (np.nan, np.inf, -3.2e37):
        q = mw.copy()
        q[1] = bad
        pose_refused("morph weights must be finite", w=q)
        q = mats.copy()
        q[2, 1, 3] = bad
        pose_refused("joint matrices must be finite", j=q)
    pose_refused("unknown regenerate 8", params=deform.params(8))
    pose_refused("regenerate TANGENTS needs NORMALS", params=deform.params(2))
    pose_refused("unknown weight -1", params=deform.params(1, weight=-1))
    pose_refused("weld = -1 is neither 0 nor 1", params=deform.params(1, weld=-1))
    pose_refused(r"reserved\[3\] must be 0", params=r)
    eng.deform_bind(bare, n_joints=3, **rig)
    pose_refused("regenerate TANGENTS needs a mesh with uvs, tangents and bitangents", g=bare, params=deform.params(3))
    # the context is still usable: the pose the refusals left alone now runs
    rest = {n: m[n] for n in NAMES[:5] if n != "uvs"}
    posed_against_reference(eng, gid, rest, rig, mw, mats, idx, uv, params=deform.params(3), what="after the refusals")
