"""Known answers for heatray_amd.query, the numpy restatement of include/hrcore_query.h (no GPU): the GPU tests check the device against
it, these check it against values worked out by hand."""
import math

import numpy as np

from heatray_amd import _ffi as ffi
from heatray_amd import host, query, scenes

F = np.float32


def _hits(rows):
    h = np.zeros(len(rows), dtype=ffi.HIT_DTYPE)
    for k, (prim, t, u, v) in enumerate(rows):
        h[k] = (prim, t, u, v)
    return h


def _camera(view=None, fov_tan=0.5, aspect=2.0, focus=3.0):
    p = ffi.PassParams()
    p.fov_tan, p.aspect_ratio, p.focus_distance = fov_tan, aspect, focus
    m = np.eye(4, dtype=F) if view is None else np.asarray(view, F)
    p.view_matrix = (ffi.C.c_float * 16)(*m.T.reshape(-1))
    return p


def test_camera_at_the_origin_looks_down_minus_z_and_its_corners_are_symmetric():
    view = scenes._translate(1.0, 2.0, 3.0)
    W, H = 32, 18
    cam = _camera(view)
    r = query.camera_rays(cam, W, H, [[W / 2, H / 2], [0, 0], [W, 0], [0, H], [W, H]])
    assert r.dtype == F and r.shape == (5, 6)
    assert (r[:, :3] == np.array([1.0, 2.0, 3.0], F)).all()  # o = the view matrix's column 3
    assert r[0, 3:].tolist() == [0.0, 0.0, -1.0]
    d = r[1:, 3:]
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # row 0 is the bottom row: (0, 0) looks left and down, and the four corners mirror each other exactly
    assert d[0, 0] < 0 and d[0, 1] < 0 and d[0, 2] < 0
    assert d[1].tolist() == [-d[0, 0], d[0, 1], d[0, 2]] and d[2].tolist() == [d[0, 0], -d[0, 1], d[0, 2]] and d[3].tolist() == [-d[0, 0], -d[0, 1], d[0, 2]]
    # the corner's direction is (-aspect * fov_tan, -fov_tan, -1) normalised
    want = np.array([-1.0, -0.5, -1.0]) / math.sqrt(2.25)
    assert np.allclose(d[0], want, atol=1e-6)
    # a rotated camera: column 3 is still the origin, the centre ray is minus the view matrix's z column
    rot = host.orbit_view_matrix(8.0, 0.5, 0.35, target=(0, -0.5, 0))
    r = query.camera_rays(_camera(rot), W, H, [[W / 2, H / 2]])
    assert (r[0, :3] == np.asarray(rot, F)[:3, 3]).all() and np.allclose(r[0, 3:], -np.asarray(rot, F)[:3, 2], atol=1e-6)


def _triangle(world=None, **kw):
    pos = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], F)
    nrm = np.array([[0, 0, 1], [0, 3, 4], [3, 0, 4]], F)  # (not unit length on purpose: the record's normal is)
    uv = np.array([[0, 0], [1, 0], [0, 1]], F)
    return scenes.MeshData(pos, nrm, np.array([0, 1, 2], np.uint32), uvs=uv, world=world, material_id=7, **kw)


def test_one_triangle_position_interpolation_and_the_windings_sign():
    mesh = _triangle()
    o = np.array([[0.5, 0.25, 5.0], [0.5, 0.25, -5.0]], F)
    d = np.array([[0, 0, -1], [0, 0, 2]], F)  # (the second from behind, with a direction of length 2: t is in units of |d|)
    hits = _hits([(0, 5.0, 0.25, 0.125), (0, 2.5, 0.25, 0.125)])
    s = query.reference_surface([mesh], [4], hits, o, d)
    assert s.dtype == ffi.SURFACE_DTYPE and s.itemsize == 64
    for k in range(2):
        assert (s["geom"][k], s["material"][k], s["prim_in_geom"][k]) == (4, 7, 0)
        assert s["position"][k].tolist() == [0.5, 0.25, 0.0]
        assert s["uv"][k].tolist() == [0.25, 0.125]  # uv = u, v with these vertex uvs
        w, u, v = 0.625, 0.25, 0.125
        N = np.array([0, 0, 1.0]) * w + np.array([0, 3, 4.0]) * u + np.array([3, 0, 4.0]) * v
        assert np.allclose(s["normal"][k], N / np.linalg.norm(N), atol=1e-6) and abs(np.linalg.norm(s["normal"][k].astype(np.float64)) - 1) < 1e-6
        assert s["geometric_normal"][k].tolist() == [0.0, 0.0, 1.0]  # of the triangle as wound, whichever side the ray came from
        assert s["reserved"][k] == 0
    assert s["flags"][0] == ffi.HR_QUERY_SF_FRONT | ffi.HR_QUERY_SF_HAS_UV and s["flags"][1] == ffi.HR_QUERY_SF_HAS_UV
    # the other winding: the geometric normal turns, and so does FRONT
    flipped = _triangle()
    flipped.indices = np.array([0, 2, 1], np.uint32)
    s2 = query.reference_surface([flipped], [0], hits, o, d)
    assert s2["geometric_normal"][0].tolist() == [0.0, 0.0, -1.0] and not s2["flags"][0] & ffi.HR_QUERY_SF_FRONT and s2["flags"][1] & ffi.HR_QUERY_SF_FRONT
    # a miss and an invalid ray: geom = -1 and nothing else
    s3 = query.reference_surface([mesh], [4], _hits([(-1, 0, 0, 0), (ffi.HR_QUERY_INVALID_RAY, 0, 0, 0)]), o, d)
    blank = np.zeros(1, ffi.SURFACE_DTYPE)
    blank["geom"] = -1
    assert s3[0].tobytes() == s3[1].tobytes() == blank.tobytes()
    # no uvs, a non-occluder
    bare = _triangle(is_occluder=False)
    bare.uvs = None
    s4 = query.reference_surface([bare], [0], hits[:1], o[:1], d[:1])
    assert s4["uv"][0].tolist() == [0.0, 0.0] and s4["flags"][0] == ffi.HR_QUERY_SF_FRONT | ffi.HR_QUERY_SF_NON_OCCLUDER


def test_a_strip_gives_both_triangles_the_same_geometric_normal_and_ids_skip_empty_meshes():
    p, n, uv, i = scenes.plane_strip(4, 4)
    strip = scenes.MeshData(p, n, i, uvs=uv, mode=ffi.HR_TRIANGLE_STRIP, material_id=1)
    empty = scenes.MeshData(p, n, np.zeros(0, np.uint32))
    o = np.array([[0.5, 3.0, 0.5], [-0.5, 3.0, -0.5]], F)
    d = np.array([[0, -1, 0], [0, -1, 0]], F)
    hits = _hits([(0, 3.0, 0.2, 0.3), (1, 3.0, 0.2, 0.3)])
    s = query.reference_surface([empty, strip], [0, 1], hits, o, d)
    assert s["prim_in_geom"].tolist() == [0, 1] and s["geom"].tolist() == [1, 1]
    assert s["geometric_normal"][0].tolist() == s["geometric_normal"][1].tolist() == [0.0, 1.0, 0.0]
    assert (s["flags"] & ffi.HR_QUERY_SF_FRONT).all()


def test_a_mirrored_world_flips_front_and_not_the_geometric_normal():
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(F)
    mirror[:3, 3] = (1.0, 0.0, 0.0)
    o, d = np.array([[0.5, 0.25, 5.0]], F), np.array([[0, 0, -1]], F)
    hits = _hits([(0, 5.0, 0.25, 0.125)])
    s = query.reference_surface([_triangle(mirror)], [0], hits, o, d)  # front_face_cw from the determinant, as Engine.add_mesh decides it
    # mirrored in x the triangle is wound clockwise as seen from +z: its geometric normal as wound is -z, and the ray from +z sees
    # it clockwise, which for a front_face_cw mesh IS the front
    assert s["geometric_normal"][0].tolist() == [0.0, 0.0, -1.0] and s["flags"][0] & ffi.HR_QUERY_SF_FRONT
    told = _triangle(mirror)
    told.front_face_cw = False
    s2 = query.reference_surface([told], [0], hits, o, d)
    assert s2["geometric_normal"][0].tolist() == [0.0, 0.0, -1.0] and not s2["flags"][0] & ffi.HR_QUERY_SF_FRONT


def test_a_zero_area_triangle_and_cancelling_normals_give_zero_vectors():
    pos = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], F)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0]], F)
    mesh = scenes.MeshData(pos, nrm, np.array([0, 1, 2], np.uint32))
    s = query.reference_surface([mesh], [0], _hits([(0, 1.0, 0.5, 0.0)]), np.zeros((1, 3), F), np.ones((1, 3), F))
    assert s["geometric_normal"][0].tolist() == [0.0, 0.0, 0.0] and s["normal"][0].tolist() == [0.0, 0.0, 0.0]
    assert s["position"][0].tolist() == [1.0, 1.0, 1.0]


def test_the_screen_flags_nan_inf_and_zero_directions_and_nothing_else():
    n = 12
    o = np.zeros((n, 3), F)
    d = np.tile(np.array([0, 0, 1], F), (n, 1))
    tm = np.full(n, 5.0, F)
    o[1, 2] = np.nan
    o[2, 0] = np.inf
    d[3, 1] = -np.inf
    d[4] = 0.0
    d[5] = (0.0, -0.0, 0.0)
    d[6, 0] = np.nan
    tm[7] = np.nan
    tm[8] = -np.inf
    tm[9] = np.inf      # "no limit": traced
    tm[10] = -1.0       # an ordinary miss: traced
    d[11] = (1e-38, 0.0, 0.0)  # tiny is not zero
    want = np.zeros(n, bool)
    want[[1, 2, 3, 4, 5, 6, 7, 8]] = True
    assert query.reference_screen(o, d, tm).tolist() == want.tolist()
    want[[7, 8]] = False
    assert query.reference_screen(o, d).tolist() == want.tolist()
    o[0] = 3e38  # huge but finite
    assert not query.reference_screen(o, d)[0]
