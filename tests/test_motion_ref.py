"""The arithmetic of motion reprojection without a GPU: heatray_amd/csrc/hr_motion.h compiled for the CPU (tests/host/motion_cpu.cpp)
against its numpy restatement heatray_amd.motion.reference_trace / reference_merge / reference_vectors, bit for bit, every pixel, on
synthetic planes and cameras and hits constructed analytically; and properties of the reference itself on constructed inputs whose
answers are known (include/hrcore_motion.h is the contract).  tests/test_gpu_motion.py holds the device to the same reference."""
import numpy as np
import pytest

import cpu_header
import synthetic_frames
from heatray_amd import _ffi as ffi
from heatray_amd import history, motion, scenes
from heatray_amd.meshprep import triangles
from synthetic_frames import F, camera, flat, plane_view, rot_x, rot_y, same_bits, translate, uniform

SIZES = [(67, 41), (64, 40)]


def params(max_history=32, normal_cos=0.8, plane_tol=0.02, min_weight=0.25):
    p = motion.default_params()
    p.max_history, p.normal_cos, p.plane_tol, p.min_weight = max_history, normal_cos, plane_tol, min_weight
    return p


def quad(half_w, half_h, z, world=None, strip=False):
    """a rectangle in the plane z (normal +z) as two triangles, or as one four-index strip"""
    p = np.array([[-half_w, -half_h, z], [half_w, -half_h, z], [half_w, half_h, z], [-half_w, half_h, z]], F)
    n = np.tile(np.array([0, 0, 1], F), (4, 1))
    if strip:
        return scenes.MeshData(p, n, np.array([0, 1, 3, 2], np.uint32), mode=ffi.HR_TRIANGLE_STRIP, world=world)
    return scenes.MeshData(p, n, np.array([0, 1, 2, 0, 2, 3], np.uint32), world=world)


def analytic_hits(rays, meshes):
    """the closest Möller–Trumbore hit of every ray with the meshes' world-space triangles, worked in float64 and handed on as the
    float32 records a query returns: data for both sides of the comparison"""
    tri = [motion.world_triangles(m) for _, m in meshes]
    p0, e1, e2 = (np.concatenate([t[k] for t in tri]).astype(np.float64) for k in range(3))
    o, d = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        pvec = np.cross(d, e2[None])
        det = (e1[None] * pvec).sum(-1)
        tvec = o - p0[None]
        u = (tvec * pvec).sum(-1) / det
        qvec = np.cross(tvec, e1[None])
        v = (d * qvec).sum(-1) / det
        t = (e2[None] * qvec).sum(-1) / det
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(ok, t, np.inf)
    best = t.argmin(axis=1)
    rows = np.arange(len(rays))
    hit = np.isfinite(t[rows, best])
    hits = np.zeros(len(rays), ffi.HIT_DTYPE)
    hits["prim"] = np.where(hit, best, -1)
    for k, a in (("t", t), ("u", u), ("v", v)):
        hits[k] = np.where(hit, a[rows, best], 0.0).astype(F)
    return hits


def mesh_table(current, snapshot):
    """per current mesh (first triangle, its first triangle in the snapshot or -1): the table hr_motion.inl builds"""
    first_in_snapshot, at = {}, 0
    for gid, m in snapshot:
        T = len(triangles(m.indices, m.mode))
        first_in_snapshot[gid] = (at, T)
        at += T
    table, at = [], 0
    for gid, m in current:
        T = len(triangles(m.indices, m.mode))
        old = first_in_snapshot.get(gid)
        table.append((at, old[0] if old is not None and old[1] == T else -1))
        at += T
    return table


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    exe = cpu_header.build("motion", tmp_path_factory.mktemp("motion_cpu"))

    def run(hist, old_cam, new, new_cam, p, hits, current, snapshot):
        H, W = new[0].shape[:2]
        snap = motion.reference_snapshot([m for _, m in snapshot])
        table = mesh_table(current, snapshot)
        cam_floats = lambda pp: np.array(list(pp.view_matrix) + [pp.aspect_ratio, pp.fov_tan], F)
        data = [np.array([W, H, p.max_history, len(snap), len(table), 0, 0, 0], np.int32), np.array([p.normal_cos, p.plane_tol, p.min_weight, 0], F),
                cam_floats(old_cam), cam_floats(new_cam), np.ascontiguousarray(hist, F), np.ascontiguousarray(new[0], F)]
        data += [np.ascontiguousarray(new[1][k], F) for k in history.PLANES]
        data += [hits, np.array([v for row in table for v in row], np.int64).astype(np.uint32).view(np.int32) if table else np.zeros(0, np.int32), snap]
        raw = np.frombuffer(cpu_header.run(exe, b"".join(a.tobytes() for a in data)), np.uint8)
        n = W * H * 16
        mv = raw[:2 * n].view(F).reshape(2, H, W, 4)
        at = 2 * n
        tr = raw[at:at + 24].view(np.uint64)
        at += 24
        planes = [raw[at + k * n:at + (k + 1) * n].view(F).reshape(H, W, 4) for k in range(4)]
        at += 4 * n
        res = raw[at:at + 24].view(np.uint64)
        at += 24
        vec = raw[at:at + n].view(F).reshape(H, W, 4)
        return (mv, dict(zip(("surface_pixels", "sky_pixels", "unmatched_pixels"), map(int, tr))), planes[0], dict(zip(history.PLANES, planes[1:])),
                dict(zip(("reused_pixels", "rejected_pixels", "history_samples"), map(int, res))), vec)
    return run


def _check(cpu, old, old_cam, new, new_cam, p, current, snapshot, what):
    """the CPU build of the header against the numpy reference, bit for bit; returns the reference's answers"""
    H, W = new[0].shape[:2]
    rays = motion.camera_rays(new_cam, W, H)
    hits = analytic_hits(rays, current)
    hist = history.reference_capture(*old)
    mv, tr = motion.reference_trace(hits, rays, current, snapshot, new_cam)
    mv = mv.reshape(2, H, W, 4)
    frame, planes, res = motion.reference_merge(hist, old_cam, mv, new[0], new[1], new_cam, p)
    vec = motion.reference_vectors(mv, old_cam, new_cam, W, H)
    cmv, ctr, cframe, cplanes, cres, cvec = cpu(hist, old_cam, new, new_cam, p, hits, current, snapshot)
    same_bits(cmv, mv, what + ": motion planes")
    assert ctr == tr, (what, ctr, tr)
    same_bits(cframe, frame, what + ": frame")
    for k in history.PLANES:
        same_bits(cplanes[k], planes[k], f"{what}: {k}")
    assert cres == {k: res[k] for k in cres}, (what, cres, res)
    same_bits(cvec, vec, what + ": vectors")
    # what holds for every merge
    assert tr["surface_pixels"] + tr["sky_pixels"] + tr["unmatched_pixels"] == W * H
    same_bits(frame[..., 3], planes["moments"][..., 3], what + ": F.a against M.a")
    assert (frame[..., 3] == np.floor(frame[..., 3])).all(), what
    empty = ~(new[0][..., 3] > 0)
    same_bits(frame[empty], new[0][empty], what + ": a pixel with n = 0 is untouched (frame)")
    for k in history.PLANES:
        same_bits(planes[k][empty], new[1][k][empty], f"{what}: a pixel with n = 0 is untouched ({k})")
    assert res["reused_pixels"] + res["rejected_pixels"] == int((new[0][..., 3] > 0).sum()), what
    unmatched = mv[0, ..., 3] == -1
    assert not res["nh"][unmatched].any(), what + ": a pixel with Mv0.w == -1 gains nothing"
    same_bits(vec[unmatched][:, :3], np.zeros((int(unmatched.sum()), 3), F), what + ": ... and has no vector")
    # the sky branch is hr_history_merge's
    hframe, hplanes, _ = history.reference_merge(hist, old_cam, new[0], new[1], new_cam, p)
    with np.errstate(all="ignore"):
        sky = (new[0][..., 3] > 0) & (mv[0, ..., 3] == 0) & (new[1]["albedo"][..., 3] / new[0][..., 3] < F(0.5))
    same_bits(frame[sky], hframe[sky], what + ": sky pixels against history.reference_merge (frame)")
    for k in history.PLANES:
        same_bits(planes[k][sky], hplanes[k][sky], f"{what}: sky pixels against history.reference_merge ({k})")
    return mv, tr, frame, planes, res, vec


def poses(moved):
    """a wall that leaves a margin of sky (mesh 0), a strip in front of part of it that moves (mesh 2), a mesh added since (mesh 3)"""
    wall = quad(2.6, 1.2, -6.0)
    snapshot = [(0, wall), (2, quad(0.8, 0.5, -4.5, world=translate(-0.6, 0.1, 0.0) @ rot_y(0.3), strip=True))]
    current = [(0, wall), (2, quad(0.8, 0.5, -4.5, world=moved, strip=True)), (3, quad(0.3, 0.3, -3.0, world=translate(1.0, -0.4, 0.0)))]
    return current, snapshot


MOVES = {k: synthetic_frames.MOVES[k] for k in ("none", "yaw", "orbit", "pitch_shift", "zoom")}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("move", sorted(MOVES))
def test_cpu_header_equals_numpy_reference_bit_for_bit(cpu, size, move):
    W, H = size
    base = translate(0.1, 0.05, 0.3) @ rot_y(0.05) @ rot_x(-0.02)  # (no identity matrices: every product rounds)
    m, fov_new = MOVES[move]()
    old_cam, new_cam = camera(base, 0.24, W=W, H=H), camera(base @ m, fov_new, W=W, H=H)
    old, new = plane_view(W, H, old_cam, 1), plane_view(W, H, new_cam, 101)
    current, snapshot = poses(translate(-0.35, 0.2, 0.1) @ rot_y(0.25))
    mv, tr, _, _, res, vec = _check(cpu, old, old_cam, new, new_cam, params(), current, snapshot, f"{size}, {move}")
    assert min(tr.values()) > 0, tr  # the inputs exercise every class of pixel
    assert res["reused_pixels"] > 0 and res["rejected_pixels"] > 0, res
    known = mv[0, ..., 3] == 1
    assert (vec[known][:, 2] > 0).all() and (vec[..., 3] == mv[0, ..., 3]).all()


@pytest.mark.parametrize("p", [params(max_history=1), params(max_history=65536), params(normal_cos=-1.0), params(normal_cos=1.0), params(plane_tol=1e-30),
                               params(plane_tol=1e30), params(min_weight=1e-30), params(min_weight=1.0)],
                         ids=["max1", "max65536", "cos-1", "cos1", "tol-tiny", "tol-huge", "minw-tiny", "minw1"])
def test_parameters_at_both_ends_of_their_ranges(cpu, p):
    W, H = 67, 41
    old_cam = camera(rot_y(0.02), 0.24, W=W, H=H)
    new_cam = camera(rot_y(0.02) @ translate(0.1, 0.0, 0.0) @ rot_y(0.01), 0.24, W=W, H=H)
    old, new = plane_view(W, H, old_cam, 21, max_n=100000 if p.max_history > 32 else 40), plane_view(W, H, new_cam, 22)
    current, snapshot = poses(translate(-0.5, 0.1, 0.0) @ rot_y(0.3))
    _, _, _, _, res, _ = _check(cpu, old, old_cam, new, new_cam, p, current, snapshot, "ends")
    nh = res["nh"]
    assert nh.max() <= p.max_history and (nh == np.floor(nh)).all()
    if p.max_history == 65536:
        assert nh.max() > 32


def test_a_wall_moved_sideways_by_whole_pixels_takes_its_history_from_there(cpu):
    """The camera stands still and the wall moves k pixel footprints to the right: pixel x shows the material point pixel x - k showed,
    so it takes that pixel's history, and its motion vector is (-k, 0) to within the rounding of the projection."""
    W, H, k, depth, fov = 64, 40, 5, 6.0, 0.25
    step = 2 * (W / H) * fov * depth / W  # the width of a pixel on the wall
    cam = camera(np.eye(4), fov, W=W, H=H)
    snapshot = [(0, quad(8.0, 4.0, -depth))]
    current = [(0, quad(8.0, 4.0, -depth, world=translate(k * step, 0, 0)))]
    col = uniform(scenes.SplitMix64(3), (W, 3))  # a colour per column
    old = flat(W, H, 32, depth=depth)
    old[0][..., :3] = col[None] * F(32)
    new = flat(W, H, 1, colour=(0, 0, 0), depth=depth)
    mv, tr, frame, _, res, vec = _check(cpu, old, cam, new, cam, params(), current, snapshot, "shift")
    assert tr == {"surface_pixels": W * H, "sky_pixels": 0, "unmatched_pixels": 0}
    nh = res["nh"]
    assert (nh[:, k:] == 32).all() and (nh[:, :k] == 0).all()  # the k columns whose points were outside the old image have no history
    assert res["rejected_pixels"] == k * H
    got = frame[:, k:, :3].astype(np.float64) / 32.0
    assert np.abs(got - col[None, :W - k].astype(np.float64)).max() < 1e-3
    assert np.abs(vec[..., 0] + k).max() < 1e-3 and np.abs(vec[..., 1]).max() < 1e-3
    assert np.abs(vec[..., 2] - depth).max() < 1e-4 and (vec[..., 3] == 1).all()
    # hr_history_merge, which does not know that the wall moved, takes every pixel's history from the pixel itself
    hframe = history.reference_merge(history.reference_capture(*old), cam, new[0], new[1], cam, params())[0]
    assert np.abs(hframe[..., :3].astype(np.float64) / 32.0 - col[None].astype(np.float64)).max() < 1e-3


def test_a_traced_depth_off_the_planes_mean_is_rejected(cpu):
    """plane_tol = 0.02: a pixel whose samples saw a surface 5 % nearer or farther than the centre ray's hit (a silhouette) takes nothing;
    1 % passes."""
    W, H, depth = 64, 40, 6.0
    cam = camera(np.eye(4), 0.25, W=W, H=H)
    meshes = [(0, quad(8.0, 4.0, -depth))]
    old, new = flat(W, H, 32, depth=depth), flat(W, H, 2, depth=depth)
    for x, scale in ((10, 1.05), (11, 0.95), (12, 1.01), (13, 0.99)):
        new[1]["normal_depth"][:, x, 3] = F(depth * scale) * F(2)
    _, _, _, _, res, _ = _check(cpu, old, cam, new, cam, params(), meshes, meshes, "depth")
    nh = res["nh"]
    assert (nh[:, [10, 11]] == 0).all() and (nh[:, [12, 13]] == 32).all() and (nh[:, 14:] == 32).all() and (nh[:, :10] == 32).all()


def test_a_mesh_the_snapshot_does_not_hold_is_rejected(cpu):
    W, H, depth = 64, 40, 6.0
    cam = camera(np.eye(4), 0.25, W=W, H=H)
    wall = quad(8.0, 4.0, -depth)
    old, new = flat(W, H, 32, depth=depth), flat(W, H, 2, depth=depth)
    for what, snapshot in (("another id", [(1, wall)]), ("another size", [(0, quad(8.0, 4.0, -depth, strip=True)), (1, wall)]), ("no mesh", [])):
        if what == "another size":
            snapshot[0][1].indices = np.array([0, 1, 3], np.uint32)  # (one triangle where the current mesh has two)
        mv, tr, frame, _, res, _ = _check(cpu, old, cam, new, cam, params(), [(0, wall)], snapshot, what)
        assert tr == {"surface_pixels": 0, "sky_pixels": 0, "unmatched_pixels": W * H}, what
        assert res["reused_pixels"] == 0 and res["rejected_pixels"] == W * H, what
        same_bits(frame, new[0], what + ": nothing changed")
        assert (mv[1, ..., 3] > 0).all() and not mv[1, ..., :3].any()


def test_the_previous_poses_normal_guards_the_taps(cpu):
    """the snapshot's geometric normal against the history's shading normal, either winding: a history normal turned past normal_cos is
    not gathered, one turned by pi is"""
    W, H, depth = 32, 8, 6.0
    cam = camera(np.eye(4), 0.25, W=W, H=H)
    meshes = [(0, quad(8.0, 4.0, -depth))]
    old, new = flat(W, H, 32, depth=depth), flat(W, H, 1, depth=depth)
    for x, cosine in ((3, 0.75), (4, 0.85), (5, 0.0), (6, -1.0)):
        old[1]["normal_depth"][:, x, :3] = F([np.sqrt(1 - cosine * cosine), 0.0, cosine]) * F(32)
    _, _, _, _, res, _ = _check(cpu, old, cam, new, cam, params(normal_cos=0.8), meshes, meshes, "normal")
    assert (res["nh"][:, [3, 5]] == 0).all() and (res["nh"][:, [4, 6]] == 32).all() and (res["nh"][:, 7:] == 32).all()


def test_default_params_are_the_documented_ones():
    p = motion.default_params()
    assert (p.max_history, p.normal_cos, p.plane_tol, p.min_weight) == (32, F(0.8), F(0.02), F(0.25)) and list(p.reserved) == [0, 0, 0, 0]
