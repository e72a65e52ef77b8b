"""Motion reprojection (include/hrcore_motion.h) on the GPU.  Every comparison with the reference is exact: no tolerance, no pixel left out.

1. the stages: the snapshot against motion.reference_snapshot; the motion planes against motion.reference_trace fed the hits Engine.query
   returns for motion.camera_rays of the same camera (so the (prim, t, u, v) behind the planes are the query's); the merged frame, the
   three AOV planes, the vectors and every counter against motion.reference_merge / reference_vectors (tests/test_motion_ref.py ties those
   to the per-pixel header the kernels compile), over seven edits at two frame sizes
2. the sky branch is hr_history_merge's: a second engine fed the same frames
3. nothing moved: every surface pixel's vector is shorter than 0.01 pixel
4. what it buys: the error against a long render of the new pose, on the mover's footprints and over the frame
5. life, order and every refusal; a hundred create, snapshot, merge, destroy cycles."""
import copy

import numpy as np
import pytest

import deform_cases
from device_support import BOTH, F, device_engine, orbit, render_passes, same, truth
from heatray_amd import _ffi as ffi
from heatray_amd import core, history, motion, scenes
from synthetic_frames import translate

pytestmark = pytest.mark.gpu

SIZES = {"160x90": (160, 90), "67x41": (67, 41)}  # whole and partial 8 x 8 blocks; a strip mesh, indexed meshes, glass
OLD_PASSES, NEW_PASSES = 24, 2
SPHERE, SMALL = 1, 3  # hr_geom_ids of scenes.multi_material: 0 the ground strip, 1 the metal sphere, 2 the glass sphere, 3 the small one


def params(normal_cos=0.8):
    p = motion.default_params()
    p.normal_cos = normal_cos  # (set explicitly: a geometric against an interpolated normal on a 24-slice sphere)
    return p


def scene(size):
    return scenes.multi_material(*SIZES[size], textured=True)


def mesh_list(sc):
    return [(gid, copy.copy(m)) for gid, m in enumerate(sc.meshes)]


# ---- the edits: each changes the engine's scene (and perhaps sc.options' camera) and returns the mesh list of the new pose
def edit_nothing(eng, sc, meshes):
    return meshes


def edit_orbit(eng, sc, meshes):
    sc.options.view_matrix = orbit(sc.options, 0.05)
    return meshes


def edit_transform(eng, sc, meshes):
    out = [(g, copy.copy(m)) for g, m in meshes]
    m = out[SPHERE][1]
    m.world = (translate(1.0 / 3.0, 0.0, 0.0) @ np.asarray(m.world, np.float64)).astype(F)  # a third of its radius
    eng.set_transform(SPHERE, m.world)
    return out


def edit_update(eng, sc, meshes):
    out = [(g, copy.copy(m)) for g, m in meshes]
    m = out[SMALL][1]
    m.positions = (np.asarray(m.positions, F) * np.array([1.0, 0.8, 1.0], F)).astype(F)
    eng.update_mesh(SMALL, m.positions)
    return out


def edit_pose(eng, sc, meshes):
    out = [(g, copy.copy(m)) for g, m in meshes]
    m = out[SPHERE][1]
    V = len(m.positions)
    rig = deform_cases.make_rig(V, 2, 0, False, seed=5)
    eng.deform_bind(SPHERE, morph_positions=rig["morph_positions"])
    weights, _ = deform_cases.pose_inputs(2, 0, seed=6)
    eng.deform_pose(SPHERE, morph_weights=weights)
    m.positions = eng.mesh_attribute(SPHERE, ffi.HR_GEOM_POSITIONS)  # (the posed vertices as the device block holds them)
    assert m.positions.shape == (V, 3) and not np.array_equal(m.positions, meshes[SPHERE][1].positions)
    return out


def edit_transform_and_orbit(eng, sc, meshes):
    return edit_orbit(eng, sc, edit_transform(eng, sc, meshes))


def edit_swap(eng, sc, meshes):
    """the small sphere goes, a coarser one comes: whatever id it gets, the snapshot holds no mesh of that id and size"""
    eng.remove_mesh(SMALL)
    p, n, uv, i = scenes.uv_sphere(12, 12, 0.45)
    new = scenes.MeshData(p, n, i, uvs=uv, world=translate(-0.3, -1.05, 2.0).astype(F), material_id=3)
    gid = eng.add_mesh(new.positions, new.normals, new.indices, uvs=new.uvs, world=new.world, material_id=new.material_id)
    out = [(g, m) for g, m in meshes if g != SMALL] + [(gid, new)]
    return sorted(out, key=lambda e: e[0])


EDITS = {"a_nothing": edit_nothing, "b_orbit": edit_orbit, "c_transform": edit_transform, "d_update": edit_update, "e_pose": edit_pose,
         "f_transform_orbit": edit_transform_and_orbit, "g_swap": edit_swap}


def drive(golden, size, edit, merge, new_passes=NEW_PASSES, check=False):
    """Render the old pose, capture, snapshot, edit, commit, clear, render the new pose, merge (`merge`: "motion", "history" or None).
    Returns what the comparisons need; with `check`, holds every stage of a motion merge to the reference on the way."""
    sc = scene(size)
    W, H = sc.width, sc.height
    eng = device_engine(sc, golden)
    old_cam = sc.options.pass_params(0)
    render_passes(eng, sc, range(OLD_PASSES))
    eng.history_capture(old_cam)
    hist = eng.history()
    before = mesh_list(sc)
    eng.motion_snapshot()
    if check:
        same(eng.motion_snapshot_triangles()[None], motion.reference_snapshot([m for _, m in before])[None], "the snapshot")
        assert eng.motion_info() == {"snapshot": True, "traced": False, "triangles": sc.n_triangles, "meshes": 4, "bytes": eng.motion_info()["bytes"]}
    after = EDITS[edit](eng, sc, before)
    eng.commit()
    eng.clear()
    new_cam = sc.options.pass_params(0)
    render_passes(eng, sc, range(new_passes))
    frame_b, planes_b = eng.readback(), eng.aovs()
    out = {"W": W, "H": H, "old_cam": old_cam, "new_cam": new_cam, "hist": hist, "frame_b": frame_b, "planes_b": planes_b, "before": before, "after": after}
    p = params()
    if merge == "motion":
        out["res"] = eng.motion_merge(new_cam, p)
        out["mv"] = eng.motion_planes()
        out["vec"] = eng.motion_vectors()
    elif merge == "history":
        out["res"] = eng.history_merge(new_cam, p)
    out["frame"], out["planes"] = eng.readback(), eng.aovs()
    if check:
        what = f"{size}, {edit}"
        rays = motion.camera_rays(new_cam, W, H)
        hits = eng.query(rays[:, :3], rays[:, 3:], tmin=0.0)
        mv, tr = motion.reference_trace(hits, rays, after, before, new_cam)
        mv = mv.reshape(2, H, W, 4)
        same(out["mv"][0], mv[0], what + ": Mv0")
        same(out["mv"][1], mv[1], what + ": Mv1")
        frame, planes, want = motion.reference_merge(hist, old_cam, mv, frame_b, planes_b, new_cam, p)
        same(out["frame"], frame, what + ": merged frame")
        for k in history.PLANES:
            same(out["planes"][k], planes[k], f"{what}: merged {k}")
        assert out["res"] == {"reused_pixels": want["reused_pixels"], "rejected_pixels": want["rejected_pixels"], "history_samples": want["history_samples"],
                              "history_passes": OLD_PASSES, "passes": new_passes, **tr}, (what, out["res"], tr, {k: v for k, v in want.items() if k != "nh"})
        same(out["vec"], motion.reference_vectors(mv, old_cam, new_cam, W, H), what + ": vectors")
        same(eng.motion_vectors(old_cam), out["vec"], what + ": vectors with the old camera named")
        assert eng.motion_trace(new_cam) == tr                                          # the trace alone writes the same planes
        same(eng.motion_planes().reshape(2 * H, W, 4), mv.reshape(2 * H, W, 4), what + ": planes of hr_motion_trace")
        same(out["frame"][..., 3], out["planes"]["moments"][..., 3], what + ": F.a against M.a")
        assert (out["frame"][..., 3] == np.floor(out["frame"][..., 3])).all()
        out["nh"] = want["nh"]
        with pytest.raises(ffi.EngineError, match="already been merged"):               # one merge per hr_clear, of whatever kind
            eng.motion_merge(new_cam, p)
        with pytest.raises(ffi.EngineError, match="already been merged"):
            eng.history_merge(new_cam, p)
        with pytest.raises(ffi.EngineError, match="already merged"):
            eng.reproject_merge(new_cam, p)
    eng.close()
    return out


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("edit", sorted(EDITS))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_every_stage_equals_the_reference(golden, size, edit):
    r = drive(golden, size, edit, "motion", check=True)
    res, n = r["res"], r["W"] * r["H"]
    assert res["surface_pixels"] + res["sky_pixels"] + res["unmatched_pixels"] == n
    assert res["reused_pixels"] + res["rejected_pixels"] == int((r["frame_b"][..., 3] > 0).sum()) == n
    assert res["surface_pixels"] > 0.3 * n and res["sky_pixels"] > 0 and res["reused_pixels"] > 0.3 * n, res  # (sanity: the ground and the sky fill the frame)
    if edit == "g_swap":
        unmatched = r["mv"][0, ..., 3] == -1
        assert res["unmatched_pixels"] == int(unmatched.sum()) > 0
        same(r["frame"][unmatched], r["frame_b"][unmatched], "no pixel with Mv0.w == -1 gains a sample")
        assert not r["nh"][unmatched].any() and not r["vec"][unmatched][:, :3].any()
    else:
        assert res["unmatched_pixels"] == 0


def test_the_driver_makes_the_same_sequence(golden):
    """motion.move_scene is capture, snapshot, edit, commit, clear, render, merge: what `drive` does by hand"""
    want = drive(golden, "67x41", "c_transform", "motion")
    sc = scene("67x41")
    eng = device_engine(sc, golden)
    render_passes(eng, sc, range(OLD_PASSES))
    res = motion.move_scene(eng, sc, lambda e: edit_transform(e, sc, mesh_list(sc)), NEW_PASSES, params())
    assert res == want["res"]
    same(eng.readback(), want["frame"], "move_scene: the merged frame")
    with pytest.raises(ValueError, match="at least one pass"):
        motion.move_scene(eng, sc, lambda e: None, 0)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("edit", sorted(EDITS))
def test_the_sky_branch_is_the_history_merges(golden, edit):
    a = drive(golden, "160x90", edit, "motion")
    b = drive(golden, "160x90", edit, "history")
    same(a["frame_b"], b["frame_b"], "both engines were fed the same frames")
    same(a["hist"].reshape(3 * a["H"], a["W"], 4), b["hist"].reshape(3 * a["H"], a["W"], 4), "... and the same history")
    with np.errstate(all="ignore"):
        sky = (a["mv"][0, ..., 3] == 0) & (a["planes_b"]["albedo"][..., 3] / a["frame_b"][..., 3] < F(0.5))
    assert sky.sum() > 100
    same(a["frame"][sky][None], b["frame"][sky][None], f"{edit}: sky pixels of the frame")
    for k in history.PLANES:
        same(a["planes"][k][sky][None], b["planes"][k][sky][None], f"{edit}: sky pixels of {k}")
    assert (a["frame"][sky][:, 3] > a["frame_b"][sky][:, 3]).any()  # (and the sky did take history over)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("size", sorted(SIZES))
def test_nothing_moved_means_no_motion(golden, size):
    """Q is interpolated over the triangle, the hit point is o + d t: they differ by rounding, about 1e-6 scene units against a pixel
    footprint of about 0.03 at this camera, so 0.01 pixel leaves more than two orders of margin."""
    r = drive(golden, size, "a_nothing", "motion")
    surface = r["mv"][0, ..., 3] == 1
    v = r["vec"][surface]
    length = np.hypot(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64))
    print(f"nothing moved, {size}: longest vector {length.max():.3g} pixel over {int(surface.sum())} surface pixels")
    assert surface.sum() > 0.3 * r["W"] * r["H"] and length.max() < 0.01
    sky = r["mv"][0, ..., 3] == 0
    assert np.abs(r["vec"][sky][:, :2]).max() < 0.01


# ------------------------------------------------------------------------------------------------ 4
def rel_l2(frame, want, mask):
    mean = frame[..., :3].astype(np.float64) / frame[..., 3:4].astype(np.float64)
    d = (mean - want.astype(np.float64))[mask]
    return float(np.sqrt((d * d).sum() / (want.astype(np.float64)[mask] ** 2).sum()))


def test_what_it_buys(golden):
    """Edit (c) at 3 new passes against a long render of the new pose, on the pixels of the mover's new and old footprints (which mesh a
    pixel's centre ray hits, before and after) and over the whole frame: comparisons, no fitted numbers."""
    size = "160x90"
    runs = {kind: drive(golden, size, "c_transform", kind, new_passes=3) for kind in ("motion", "history", None)}

    def moved():
        sc = scene(size)
        m = sc.meshes[SPHERE]
        m.world = (translate(1.0 / 3.0, 0.0, 0.0) @ np.asarray(m.world, np.float64)).astype(F)
        return sc
    want = truth(moved)
    r = runs["motion"]
    W, H = r["W"], r["H"]
    footprint = np.zeros((H, W), bool)
    for sc in (scene(size), moved()):  # the old pose, then the new one
        eng = core.create_engine()
        sc.apply(eng)
        rays = motion.camera_rays(sc.options.pass_params(0), W, H)
        _, surf = eng.query(rays[:, :3], rays[:, 3:], surface=True, tmin=0.0)
        footprint |= (surf["geom"] == SPHERE).reshape(H, W)
        eng.close()
    everything = np.ones((H, W), bool)
    err = {kind: (rel_l2(run["frame"], want, footprint), rel_l2(run["frame"], want, everything)) for kind, run in runs.items()}
    print(f"what it buys, {int(footprint.sum())} footprint pixels, rel_l2 (footprint, frame): motion merge {err['motion']}, "
          f"history merge as if nothing had moved {err['history']}, no merge {err[None]}")
    assert 200 < footprint.sum() < 0.3 * W * H
    assert err["motion"][0] < err[None][0]
    assert err["motion"][0] < err["history"][0]
    assert err["motion"][1] < err[None][1]


# ------------------------------------------------------------------------------------------------ 5
def test_life_order_and_every_refusal(golden):
    sc = scene("67x41")
    W, H = sc.width, sc.height
    eng = core.create_engine()
    cam = sc.options.pass_params(0)
    p = params()
    bad = sc.options.pass_params(0)
    bad.fov_tan = float("nan")
    # ---- before there is a frame, a scene, a snapshot
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        eng.motion_snapshot()
    with pytest.raises(ffi.EngineError, match="no frame"):
        eng.motion_trace(cam)
    with pytest.raises(ffi.EngineError, match="no snapshot"):
        eng.motion_snapshot_triangles()
    assert eng.motion_info() == {"snapshot": False, "traced": False, "triangles": 0, "meshes": 0, "bytes": 0}
    eng.motion_drop()  # (no error when there is nothing)
    eng.close()
    eng = device_engine(sc, golden, aovs=0)
    with pytest.raises(ffi.EngineError, match="motion trace: no snapshot"):
        eng.motion_trace(cam)
    with pytest.raises(ffi.EngineError, match="not finite"):
        eng.motion_trace(bad)
    with pytest.raises(ffi.EngineError, match="no trace at this frame size"):
        eng.motion_planes()
    with pytest.raises(ffi.EngineError, match="no trace at this frame size"):
        eng.motion_vectors(cam)
    with pytest.raises(ffi.EngineError, match="needs the AOV planes"):
        eng.motion_merge(cam, p)
    eng.set_aovs(BOTH)
    eng.clear()
    with pytest.raises(ffi.EngineError, match="the frame is empty"):
        eng.motion_merge(cam, p)
    render_passes(eng, sc, range(2))
    with pytest.raises(ffi.EngineError, match="motion merge: no snapshot"):
        eng.motion_merge(cam, p)
    eng.motion_snapshot()
    with pytest.raises(ffi.EngineError, match="motion merge: no captured history"):
        eng.motion_merge(cam, p)
    with pytest.raises(ffi.EngineError, match="not finite"):
        eng.motion_merge(bad, p)
    for field, value in (("max_history", 0), ("normal_cos", float("nan")), ("plane_tol", 0.0), ("min_weight", float("inf"))):
        q = params()
        setattr(q, field, value)
        with pytest.raises(ffi.EngineError, match="history: " + field):
            eng.motion_merge(cam, q)
    # ---- the snapshot is ordered behind the commit it reads, and the next commit waits for it
    first = motion.reference_snapshot(sc.meshes)
    moved = copy.copy(sc.meshes[SPHERE])
    moved.world = (translate(0.0, 0.4, 0.0) @ np.asarray(moved.world, np.float64)).astype(F)
    eng.set_transform(SPHERE, moved.world)
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        eng.motion_snapshot()
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        eng.motion_trace(cam)
    eng.commit()  # (issued right behind the snapshot: it rewrites the triangles the snapshot read)
    same(eng.motion_snapshot_triangles()[None], first[None], "the snapshot after the next commit")
    # ---- a trace; the vectors want an old camera or a captured history
    tr = eng.motion_trace(cam)
    assert tr["unmatched_pixels"] == 0 and tr["surface_pixels"] > 0 and eng.motion_info()["traced"]
    planes = eng.motion_planes()
    with pytest.raises(ffi.EngineError, match="no old camera and no captured history"):
        eng.motion_vectors()
    with pytest.raises(ffi.EngineError, match="not finite"):
        eng.motion_vectors(bad)
    vec = eng.motion_vectors(cam)
    same(vec, motion.reference_vectors(planes, cam, cam, W, H), "vectors with the old camera named")
    up = vec[planes[0, ..., 3] == 1][:, 1]
    assert (up < -1.0).sum() > 20 and (np.abs(up) < 0.01).sum() > 100  # the sphere went up, so its pixels' points come from below; the ground stood still
    with pytest.raises(ffi.EngineError, match="null output"):
        eng.motion_vectors_to_device(0, cam)
    with pytest.raises(ffi.EngineError, match="16-byte aligned"):
        eng.motion_vectors_to_device(8, cam)
    import torch
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    eng.motion_vectors_to_device(t.data_ptr(), cam)  # the ctx stream
    eng.synchronize()
    torch.cuda.synchronize()
    same(t.cpu().numpy(), vec, "hr_motion_vectors on the ctx stream")
    s = torch.cuda.Stream()
    t2 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    eng.motion_vectors_to_device(t2.data_ptr(), cam, stream=s.cuda_stream)
    s.synchronize()
    same(t2.cpu().numpy(), vec, "hr_motion_vectors on a foreign stream")
    # ---- the snapshot survives hr_clear, a commit and a resize; the planes do not survive a resize
    eng.clear()
    same(eng.motion_planes().reshape(2 * H, W, 4), planes.reshape(2 * H, W, 4), "the planes after hr_clear")
    eng.resize(48, 32)
    info = eng.motion_info()
    assert info["snapshot"] and not info["traced"] and info["triangles"] == sc.n_triangles and info["meshes"] == 4
    same(eng.motion_snapshot_triangles()[None], first[None], "the snapshot after a resize")
    with pytest.raises(ffi.EngineError, match="no trace at this frame size"):
        eng.motion_planes()
    assert eng.motion_trace(cam)["surface_pixels"] > 0 and eng.motion_planes().shape == (2, 32, 48, 4)
    # ---- a second snapshot replaces the first; a drop frees both
    eng.motion_snapshot()
    same(eng.motion_snapshot_triangles()[None], motion.reference_snapshot([m if g != SPHERE else moved for g, m in enumerate(sc.meshes)])[None], "a second snapshot")
    eng.motion_drop()
    assert eng.motion_info() == {"snapshot": False, "traced": False, "triangles": 0, "meshes": 0, "bytes": 0}
    with pytest.raises(ffi.EngineError, match="no snapshot"):
        eng.motion_trace(cam)
    with pytest.raises(ffi.EngineError, match="no trace at this frame size"):
        eng.motion_planes()
    # ---- the merges exclude each other in both directions
    eng.resize(W, H)
    eng.clear()
    render_passes(eng, sc, range(2))
    eng.history_capture(cam)
    eng.motion_snapshot()
    for first_merge in (eng.history_merge, eng.reproject_merge):
        eng.clear()
        render_passes(eng, sc, range(1))
        first_merge(cam, p)
        with pytest.raises(ffi.EngineError, match="motion merge: a history has already been merged"):
            eng.motion_merge(cam, p)
    eng.clear()
    render_passes(eng, sc, range(1))
    assert eng.motion_merge(cam, p)["reused_pixels"] > 0
    eng.close()
    # ---- a context group and a tile shard, as history refuses them
    grp = core.create_group([0, 0])
    sc.apply(grp)
    for call in (grp.motion_snapshot, lambda: grp.motion_trace(cam)):
        with pytest.raises(ffi.EngineError, match="a context group is not supported"):
            call()
    grp.close()
    shard = core.create_engine(rank=0, world=2)
    sc.apply(shard)
    for call in (shard.motion_snapshot, lambda: shard.motion_trace(cam), lambda: shard.motion_merge(cam, p)):
        with pytest.raises(ffi.EngineError, match="tile-sharded"):
            call()
    shard.close()


CYCLES = 100


def test_a_hundred_lives_give_the_first_ones_bytes():
    """create, snapshot, merge, destroy: everything the feature holds goes with the context (hr_features.h: MotionState), a handle freed
    twice or while still in use shows as a fault or as other bytes, and what the feature holds is 0 bytes after a drop.  (Nothing is
    asserted about free device memory: that number belongs to everybody on the device.)"""
    sc = scenes.cornell_box(width=40, height=24, bounces=2)
    cam = sc.options.pass_params(0)
    first = None
    for k in range(CYCLES):
        eng = core.create_engine()
        sc.apply(eng)
        eng.set_aovs(BOTH)
        eng.clear()
        eng.render_pass(cam)
        eng.history_capture(cam)
        eng.motion_snapshot()
        eng.clear()
        eng.render_pass(cam)
        res = eng.motion_merge(cam)
        got = (eng.readback(), eng.motion_planes().reshape(2 * 24, 40, 4), eng.motion_vectors())
        assert eng.motion_info()["bytes"] > 0
        if k % 2:
            eng.motion_drop()
            assert eng.motion_info()["bytes"] == 0
        eng.close()
        assert res["reused_pixels"] > 0
        if first is None:
            first = got
        for a, b, what in zip(got, first, ("frame", "planes", "vectors")):
            same(a, b, f"cycle {k}: {what}")
