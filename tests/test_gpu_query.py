"""Ray queries (include/hrcore_query.h) on the GPU: the hits are the CPU oracle's and hr_debug_trace's byte for byte, the surface records
are heatray_amd.query.reference_surface's, invalid rays get their defined answer, strides and device pointers are honoured, commits and
queries order themselves, pixel queries see what the renderer's first surface AOV sees, and a context group answers like a plain
context."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from heatray_amd import _ffi as ffi
from heatray_amd import core, host, meshprep, query, scenes

pytestmark = pytest.mark.gpu

F = np.float32
N_RAYS = 4099  # no multiple of 64 or 256: the last wave and the last workgroup are partly empty


def soup_rays(sc, n, seed):
    """the rays of test_traversal_hits_bit_exact: origins in a box around the scene, a third of them aimed at triangle centroids"""
    rng = np.random.default_rng(seed)
    org = rng.uniform(-1.2, 1.2, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    tgt = np.concatenate([m.positions.reshape(-1, 3, 3).mean(axis=1) for m in sc.meshes])
    k = n // 3
    aim = tgt[rng.integers(0, tgt.shape[0], k)] - org[:k]
    d[:k] = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(F)
    tm = rng.uniform(0.05, 2.5, n).astype(F)
    return org, d, tm


_SOUP = {}


def soup(n_tris):
    """(scene, gpu engine, rays, the oracle's closest hits, the oracle's occlusion answers): made once per size and left unchanged"""
    if n_tris not in _SOUP:
        sc = scenes.triangle_soup(n_tris, width=32, height=32)
        g, o = core.create_engine(), oracle_lib.engine()
        sc.apply(g), sc.apply(o)
        org, d, tm = soup_rays(sc, N_RAYS, n_tris)
        ho = o.debug_trace(org, d)
        ao = o.debug_trace(org, d, tmax=tm, skip_prim=ho["prim"], any_hit=True)
        o.close()
        _SOUP[n_tris] = (sc, g, (org, d, tm), ho, ao)
    return _SOUP[n_tris]


# ------------------------------------------------------------------------------- 1. hits
@pytest.mark.parametrize("n_tris", [3, 40, 3000])
def test_hits_are_the_oracles(n_tris):
    sc, g, (org, d, tm), ho, ao = soup(n_tris)
    assert (ho["prim"] >= 0).sum() > 100
    hq = g.query(org, d, tmin=None)
    assert hq.tobytes() == ho.tobytes(), f"{(hq != ho).sum()} of {N_RAYS} closest hits differ from the oracle's"
    assert hq.tobytes() == g.debug_trace(org, d).tobytes()
    assert g.query_last() == {"rays": N_RAYS, "hits": int((ho["prim"] >= 0).sum()), "invalid": 0}
    aq = g.query(org, d, tmax=tm, skip_prim=ho["prim"], any_hit=True)
    assert aq.tobytes() == ao.tobytes(), f"{(aq != ao).sum()} of {N_RAYS} occlusion answers differ from the oracle's"
    assert g.query_last() == {"rays": N_RAYS, "hits": int((ao["prim"] >= 0).sum()), "invalid": 0}
    # the surface records of the same hits (n_tris = 3: a tree that is one root leaf)
    hs, surf = g.query(org, d, surface=True)
    assert hs.tobytes() == ho.tobytes()
    assert surf.tobytes() == query.reference_surface(sc.meshes, range(len(sc.meshes)), ho, org, d).tobytes()


# ------------------------------------------------------------------------------- 2. strides
def test_strided_rays_give_the_tight_calls_bytes_and_bad_strides_are_refused():
    sc, g, (org, d, tm), ho, ao = soup(40)
    buf = np.zeros((N_RAYS, 8), F)
    buf[:, 0:3], buf[:, 4:7], buf[:, 7] = org, d, tm
    buf[:, 3] = np.nan  # (padding nobody may read)
    want = g.query(org, d, tmax=tm)
    got = g.query(buf[:, 0:3], buf[:, 4:7], tmax=buf[:, 7])
    assert got.tobytes() == want.tobytes() and (want["prim"] >= 0).sum() > 50
    sk = np.zeros((N_RAYS, 3), np.int32)
    sk[:, 1] = ho["prim"]
    assert g.query(buf[:, 0:3], buf[:, 4:7], tmax=buf[:, 7], skip_prim=sk[:, 1], any_hit=True).tobytes() == ao.tobytes()
    hits = np.empty(N_RAYS, ffi.HIT_DTYPE)
    for k, bad in ((0, 10), (0, 8), (1, 30), (1, 4), (2, 2), (2, 6), (3, 3), (0, -32)):
        strides = [32, 32, 32, 0]
        strides[k] = bad
        desc = g._query_desc(N_RAYS, buf.ctypes.data, buf.ctypes.data + 16, buf.ctypes.data + 28, None, strides, False, None, hits.ctypes.data, None)
        with pytest.raises(ffi.EngineError, match="stride"):
            g._feature_call("query", "query_trace_host", C.byref(desc))


# ------------------------------------------------------------------------------- 3. surface records
def world_triangles(mesh):
    tri = meshprep.triangles(mesh.indices, mesh.mode)
    m = np.eye(4) if mesh.world is None else np.asarray(mesh.world, np.float64)
    p = np.asarray(mesh.positions, np.float64).reshape(-1, 3) @ m[:3, :3].T + m[:3, 3]
    return p[tri]  # T x 3 x 3


def surface_scene():
    sc = scenes.multi_material(width=32, height=18, slices=8)
    p, n, _, i = scenes.uv_sphere(6, 6, 0.4)
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(F)
    mirror[:3, 3] = (0.0, 1.0, 0.0)
    sc.meshes.append(scenes.MeshData(p, n, i, world=mirror, material_id=1))  # (no uvs: HAS_UV clear; det < 0: front_face_cw)
    return sc


def centroid_rays(sc, n, seed):
    rng = np.random.default_rng(seed)
    tris = np.concatenate([world_triangles(m) for m in sc.meshes])
    pick = rng.integers(0, len(tris), n)
    t = tris[pick]
    c = t.mean(axis=1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    side = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)[:, None]
    org = c + nrm * side * 0.3 + rng.uniform(-0.05, 0.05, (n, 3))
    d = c - org + rng.uniform(-1e-3, 1e-3, (n, 3))
    return org.astype(F), d.astype(F)  # (directions are not unit length: t is in units of |d|)


def test_surface_records_are_the_references_bytes():
    sc = surface_scene()
    g = core.create_engine()
    sc.apply(g)
    ids = list(range(len(sc.meshes)))
    org, d = centroid_rays(sc, N_RAYS, 7)
    hits, surf = g.query(org, d, surface=True)
    assert hits.tobytes() == g.debug_trace(org, d).tobytes()
    hit = hits["prim"] >= 0
    assert hit.sum() > 3000
    geoms = set(surf["geom"][hit].tolist())
    assert len(geoms) >= 3 and 0 in geoms and 4 in geoms, geoms  # mesh 0 is the ground's strip, mesh 4 the mirrored sphere
    assert sc.meshes[0].mode == ffi.HR_TRIANGLE_STRIP and set(surf["prim_in_geom"][surf["geom"] == 0].tolist()) == {0, 1}
    front = (surf["flags"][hit] & ffi.HR_QUERY_SF_FRONT) != 0
    assert front.any() and (~front).any()
    on_mirror = surf["geom"] == 4
    assert ((surf["flags"][on_mirror] & ffi.HR_QUERY_SF_FRONT) != 0).any() and ((surf["flags"][on_mirror] & ffi.HR_QUERY_SF_FRONT) == 0).any()
    assert ((surf["flags"][on_mirror] & ffi.HR_QUERY_SF_HAS_UV) == 0).all() and ((surf["flags"][surf["geom"] == 1] & ffi.HR_QUERY_SF_HAS_UV) != 0).all()
    want = query.reference_surface(sc.meshes, ids, hits, org, d)
    assert surf.tobytes() == want.tobytes(), f"{(surf != want).sum()} of {N_RAYS} surface records differ"
    ln = np.linalg.norm(surf["normal"][hit].astype(np.float64), axis=1)
    assert (np.abs(ln - 1.0) < 1e-6).all() and (np.abs(np.linalg.norm(surf["geometric_normal"][hit].astype(np.float64), axis=1) - 1.0) < 1e-6).all()
    # rays that miss: aimed away from the scene
    away = np.tile(np.array([[0.0, 1.0, 0.0]], F), (70, 1))
    hm, sm = g.query(org[:70] + F(20.0), away, surface=True)
    blank = np.zeros(70, ffi.SURFACE_DTYPE)
    blank["geom"] = -1
    assert (hm["prim"] == -1).all() and sm.tobytes() == blank.tobytes()
    # ids, not positions: without the first mesh the others keep their names
    g.remove_mesh(0)
    g.commit()
    h2, s2 = g.query(org, d, surface=True)
    assert s2.tobytes() == query.reference_surface(sc.meshes[1:], ids[1:], h2, org, d).tobytes()
    left = set(s2["geom"][h2["prim"] >= 0].tolist())
    assert 0 not in left and 4 in left and left <= {1, 2, 3, 4} and len(left) >= 3, left
    g.close()


# ------------------------------------------------------------------------------- 4. invalid rays
def test_invalid_rays_are_not_traced_and_the_others_do_not_notice():
    sc, g, (org, d, tm), ho, ao = soup(3000)
    n = 200
    o1, d1, t1 = org[:n].copy(), d[:n].copy(), np.full(n, 50.0, F)
    clean_h, clean_s = g.query(o1, d1, tmax=t1, surface=True)
    assert (clean_h["prim"] >= 0).sum() > 20
    rows = [3, 64, 130, 199]
    o1[3, 1] = np.nan
    d1[64, 2] = np.inf
    d1[130] = 0.0
    t1[199] = np.nan
    assert query.reference_screen(o1, d1, t1).nonzero()[0].tolist() == rows
    h, s = g.query(o1, d1, tmax=t1, surface=True)
    assert g.query_last() == {"rays": n, "hits": int((h["prim"] >= 0).sum()), "invalid": 4}
    bad = np.zeros(n, bool)
    bad[rows] = True
    assert (h["prim"][bad] == ffi.HR_QUERY_INVALID_RAY).all() and (h["t"][bad] == 0).all() and (h["u"][bad] == 0).all() and (h["v"][bad] == 0).all()
    blank = np.zeros(4, ffi.SURFACE_DTYPE)
    blank["geom"] = -1
    assert s[bad].tobytes() == blank.tobytes()
    assert h[~bad].tobytes() == clean_h[~bad].tobytes() and s[~bad].tobytes() == clean_s[~bad].tobytes()
    a = g.query(o1, d1, tmax=t1, any_hit=True)
    assert (a["prim"][bad] == ffi.HR_QUERY_INVALID_RAY).all() and set(a["prim"][~bad].tolist()) <= {0, -1}
    assert g.query_last()["invalid"] == 4
    t1[199] = np.inf  # +inf is "no limit", not an invalid ray
    assert g.query(o1, d1, tmax=t1)["prim"][199] == g.query(org[199:200], d[199:200])["prim"][0] != ffi.HR_QUERY_INVALID_RAY


# ------------------------------------------------------------------------------- 5. refusals and edges
def test_refusals_and_edges():
    sc, g, (org, d, tm), ho, ao = soup(40)
    n = 64
    o1, d1 = np.ascontiguousarray(org[:n]), np.ascontiguousarray(d[:n])
    hits = np.full(n, 0x5A, np.uint8).repeat(16).view(ffi.HIT_DTYPE)
    surf = np.empty(n, ffi.SURFACE_DTYPE)
    before = hits.tobytes()

    def call(n_=n, origins=o1.ctypes.data, dirs=d1.ctypes.data, any_hit=False, hits_=hits.ctypes.data, surf_=None, flags=None, eng=g):
        desc = eng._query_desc(n_, origins, dirs, None, None, (0, 0, 0, 0), any_hit, None, hits_, surf_)
        if flags is not None:
            desc.flags = flags
        eng._feature_call("query", "query_trace_host", C.byref(desc))

    call(n_=0)
    assert hits.tobytes() == before  # n = 0 is fine and writes nothing
    none = g.query(np.zeros((0, 3), F), np.zeros((0, 3), F), surface=True)
    assert none[0].shape == (0,) and none[1].shape == (0,) and g.query_pixels(sc.options.pass_params(0), np.zeros((0, 2), F), surface=False).shape == (0,)
    for kw, cause in ((dict(n_=-1), "negative"), (dict(origins=None), "null origins"), (dict(dirs=None), "null directions"),
                      (dict(hits_=None), "no output"), (dict(any_hit=True, surf_=surf.ctypes.data), "ANY_HIT"), (dict(flags=6), "unknown flags 6")):
        with pytest.raises(ffi.EngineError, match=cause):
            call(**kw)
    assert hits.tobytes() == before
    with pytest.raises(ffi.EngineError, match="16-byte aligned"):
        g.query_to_device(n, 4096, 8192, hits_ptr=4100)
    # an uncommitted scene
    e = core.create_engine()
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        call(eng=e)
    # a committed empty scene: every valid ray misses
    e.commit()
    he, se = e.query(o1, d1, surface=True)
    assert (he["prim"] == -1).all() and (he["t"] == 0).all() and (se["geom"] == -1).all()
    assert e.query_last() == {"rays": n, "hits": 0, "invalid": 0}
    with pytest.raises(ffi.EngineError, match="no frame"):
        e.query_pixels(sc.options.pass_params(0), [[0.5, 0.5]])
    e.close()
    # tmax <= tmin is an ordinary miss
    full = g.query(o1, d1)
    assert (full["prim"] >= 0).sum() > 5
    eps = g.scene_info().ray_epsilon
    for tmax, tmin in ((np.full(n, eps, F), None), (np.full(n, 0.5, F), 0.5), (np.zeros(n, F), 0.0), (np.full(n, -1.0, F), None)):
        assert (g.query(o1, d1, tmax=tmax, tmin=tmin)["prim"] == -1).all()
    assert g.query_last() == {"rays": n, "hits": 0, "invalid": 0}
    # a larger tmin drops exactly the hits in front of it
    far = g.query(o1, d1, tmin=0.7)
    near = full["prim"] >= 0
    assert (far[near & (full["t"] > F(0.7))].tobytes() == full[near & (full["t"] > F(0.7))].tobytes()) and ((far["t"] > F(0.7)) | (far["prim"] < 0)).all()


def test_queries_leave_the_frame_and_the_statistics_alone():
    sc = scenes.triangle_soup(3000, width=32, height=32)
    g = core.create_engine(collect_stats=True)
    sc.apply(g)
    org, d, tm = soup_rays(sc, 1000, 5)
    for s in range(2):
        g.render_pass(sc.options.pass_params(s))
    frame = g.readback()
    stats = {k: v for k, v in g.stats().as_dict().items() if k != "ms"}
    assert stats["rays_closest"] > 0
    g.query(org, d)
    g.query(org, d, tmax=tm, any_hit=True)
    g.query_pixels(sc.options.pass_params(0), [[3.5, 4.5], [16.0, 16.0]])
    assert g.readback().tobytes() == frame.tobytes()
    assert {k: v for k, v in g.stats().as_dict().items() if k != "ms"} == stats
    g.clear()
    for s in range(2):
        g.render_pass(sc.options.pass_params(s))
    assert g.readback().tobytes() == frame.tobytes()
    g.close()


# ------------------------------------------------------------------------------- 6. device pointers and ordering
def test_device_pointers_on_a_torch_stream_and_the_order_of_commits_and_queries():
    import torch
    sc = scenes.triangle_soup(3000, width=32, height=32)
    org, d, tm = soup_rays(sc, N_RAYS, 3000)
    _, _, _, ho, ao = soup(3000)
    g, o = core.create_engine(), oracle_lib.engine()
    sc.apply(g), sc.apply(o)
    dev = torch.device("cuda:0")
    to = torch.from_numpy(org).to(dev)
    td = torch.from_numpy(d).to(dev)
    tt = torch.from_numpy(tm).to(dev)
    ts = torch.from_numpy(ho["prim"].copy()).to(dev)
    h1, h2, a1 = (torch.full((N_RAYS, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(3))
    s1 = torch.zeros((N_RAYS, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    raw = stream.cuda_stream
    g.query_to_device(N_RAYS, to.data_ptr(), td.data_ptr(), hits_ptr=a1.data_ptr(), tmax_ptr=tt.data_ptr(), skip_ptr=ts.data_ptr(), any_hit=True, stream=raw)
    g.query_to_device(N_RAYS, to.data_ptr(), td.data_ptr(), hits_ptr=h1.data_ptr(), surfaces_ptr=s1.data_ptr(), stream=raw)
    # no wait in between: the commit has to wait for the queries above, and the query below for the commit
    move = scenes._translate(0.25, -0.125, 0.0625)
    for eng in (g, o):
        for gid in range(len(sc.meshes)):
            eng.set_transform(gid, move)
        eng.commit()
    g.query_to_device(N_RAYS, to.data_ptr(), td.data_ptr(), hits_ptr=h2.data_ptr(), stream=raw)
    assert g.query_last() == {"rays": N_RAYS, "hits": int((o.debug_trace(org, d)["prim"] >= 0).sum()), "invalid": 0}
    stream.synchronize()
    first = h1.cpu().numpy().view(ffi.HIT_DTYPE).reshape(-1)
    assert first.tobytes() == ho.tobytes()
    assert a1.cpu().numpy().view(ffi.HIT_DTYPE).reshape(-1).tobytes() == ao.tobytes()
    surf = s1.cpu().numpy().view(ffi.SURFACE_DTYPE).reshape(-1)
    assert surf.tobytes() == query.reference_surface(sc.meshes, range(len(sc.meshes)), ho, org, d).tobytes()
    want = o.debug_trace(org, d)
    assert (want["prim"] >= 0).sum() > 100 and want.tobytes() != ho.tobytes()
    assert h2.cpu().numpy().view(ffi.HIT_DTYPE).reshape(-1).tobytes() == want.tobytes()
    g.close(), o.close()


# ------------------------------------------------------------------------------- 7. pixel queries
def test_pixel_queries_see_what_the_renderer_sees():
    sc = scenes.multi_material(width=32, height=18, slices=8)
    W, H = sc.width, sc.height
    g = core.create_engine()
    P = sc.options.max_render_passes
    half = np.full((16, P, 2), 0.5, F)  # every jitter and every aperture sample is the centre
    off = np.zeros((W * H, 2), F)
    sc.apply(g, tables=(half, half, off))
    g.set_aovs(ffi.HR_AOV_SURFACE)
    pp = sc.options.pass_params(0)
    pp.aperture_radius = 0.0
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=-1).astype(F)  # row 0 is the bottom row, as in the frame
    hits, surf, rays = g.query_pixels(pp, xy, surface=True, rays=True)
    assert rays.tobytes() == query.camera_rays(pp, W, H, xy).tobytes()
    h2, s2 = g.query(rays[:, :3], rays[:, 3:], tmin=0.0, surface=True)
    assert hits.tobytes() == h2.tobytes() and surf.tobytes() == s2.tobytes()
    hit = hits["prim"] >= 0
    assert 100 < hit.sum() < W * H and {0, 1, 2} <= set(surf["geom"][hit].tolist())
    # what makes the AOV's hit flag comparable: every hit is a front face of a PBR or glass material
    assert ((surf["flags"][hit] & ffi.HR_QUERY_SF_FRONT) != 0).all()
    assert all(sc.materials[m].type in (ffi.HR_MAT_PBR, ffi.HR_MAT_GLASS) for m in set(surf["material"][hit].tolist()))
    g.render_pass(pp)
    alpha = g.aovs()["albedo"][..., 3]
    assert alpha.shape == (H, W)
    assert (alpha.reshape(-1)[hit] == 1).all() and (alpha.reshape(-1)[~hit] == 0).all()
    # autofocus and pick at a pixel that shows the metal sphere
    k = int(np.nonzero(surf["geom"] == 1)[0][0])
    x, y = float(xy[k, 0]), float(xy[k, 1])
    sc.options.fstop = host.FSTOP_DISABLED
    assert query.autofocus(g, sc.options, x, y) == float(hits["t"][k]) > 0
    p = query.pick(g, sc.options, x, y)
    assert (p["geom"], p["material"], p["prim"]) == (1, 1, int(hits["prim"][k])) and p["position"].tobytes() == surf["position"][k].tobytes()
    m = int(np.nonzero(~hit)[0][0])
    assert query.pick(g, sc.options, float(xy[m, 0]), float(xy[m, 1])) is None and query.autofocus(g, sc.options, float(xy[m, 0]), float(xy[m, 1])) is None
    g.close()


# ------------------------------------------------------------------------------- 8. groups
def test_a_group_answers_like_a_plain_context():
    sc = surface_scene()
    plain, grp = core.create_engine(), core.create_group([0, 0])
    sc.apply(plain), sc.apply(grp)
    org, d = centroid_rays(sc, 1000, 11)
    hp, sp = plain.query(org, d, surface=True)
    hg, sg = grp.query(org, d, surface=True)
    assert (hp["prim"] >= 0).sum() > 500 and hg.tobytes() == hp.tobytes() and sg.tobytes() == sp.tobytes()
    assert grp.query_last() == plain.query_last()
    tm = np.full(1000, 0.5, F)
    assert grp.query(org, d, tmax=tm, any_hit=True).tobytes() == plain.query(org, d, tmax=tm, any_hit=True).tobytes()
    xy = np.array([[0.5, 0.5], [16.0, 9.0], [20.25, 4.75], [31.5, 17.5]], F)
    pp = sc.options.pass_params(0)
    for a, b in zip(grp.query_pixels(pp, xy, rays=True), plain.query_pixels(pp, xy, rays=True)):
        assert a.tobytes() == b.tobytes()
    grp.close(), plain.close()
