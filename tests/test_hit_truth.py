"""The hit test against float64 TRUTH: every other test of the ray / triangle hit compares the GPU with the oracle, which
evaluates the same float32 operations — they prove that both agree, not that what they agree on is a hit.  Here the reference is float64
Möller–Trumbore in numpy on the same float32 inputs (tests/thin_cases.py), on thin triangles in axis-aligned, slightly tilted and freely
rotated planes seen from 0.2 to 5 scene diagonals away: where the box condition alone (conditions 1-3) turned real hits away — up to 97 %
of them at aspect 1:10 000 — and the plane retry (hr_trace.h::hitOnPlane) keeps them.

The statement, per cell of the grid (aspect x plane x distance, 64 triangles, 2 000 rays): EVERY robust true hit (float64: u, v > 0.1,
u + v < 0.9, t > 10 eps, |d.n| > 0.3) is reported, on the triangle float64 names, at a distance within the bound below of float64's.

The distance bound.  Möller–Trumbore's t = e2.(tvec x e1) / det; on a triangle of width w = L / aspect seen from distance R the
numerator and the determinant are sums of products of magnitude ~ R L |d| whose exact value is ~ w L |d| cos: each rounding (2^-24
relative to the products) is amplified by R / w, so |t - t64| <~ c 2^-24 aspect (R / L) t with a dozen roundings behind c.  With R ~ t ~
D |diagonal| and L >= 0.2 that is 16 * 2^-24 * aspect ~ 1e-6 aspect, as a share of D |diagonal|: 1e-3 at aspect 1:1000 and below,
1e-2 at 1:10 000.  (The retry's t' = n.(v0 - o) / n.d is tighter, a few 2^-24 on thin boxes; the bound is Möller–Trumbore's, which
every candidate that passes the box condition still carries.)

CPU: the numpy float32 restatement of the rule, the oracle's tree and its brute force (tree == brute force bit for bit, closest hit and
any hit; restatement == brute force bit for bit).  GPU: debug_trace and query under both builders, after a refit, and a rendered floor
of 1:1000 boards through k_trace and the packet lanes."""
import math
import os

import numpy as np
import pytest

import oracle_lib
import thin_cases as tc
from heatray_amd import core, host, scenes

F = np.float32
CELLS = [(a, p) for a in tc.ASPECTS for p in tc.PLANES]
ANCHORS = np.array([tc.N_TRIS, tc.N_TRIS + 1])


def t_bound(aspect):
    return 1e-2 if aspect >= 10000 else 1e-3   # of D |diagonal| (the module's docstring derives them)


def check_truth(hits, occluded, k, robust, alone, t64, aspect, D, diag, what):
    """hits: closest hits (HIT_DTYPE-like: prim, t), occluded: any-hit answers (prim 0 blocked / -1 clear) or None"""
    prim, t = hits["prim"], hits["t"]
    lost = robust & (prim < 0)
    wrong = alone & (prim != k)
    with np.errstate(invalid="ignore"):
        err = np.where(alone & (prim == k), np.abs(t.astype(np.float64) - t64), 0.0).max() / (D * diag)
    clear = robust & (occluded["prim"] != 0) if occluded is not None else np.zeros_like(lost)
    print(f"{what}: aspect 1:{aspect} D {D}: robust {robust.sum()} (unshadowed {alone.sum()}), lost {lost.sum()}, on another triangle "
          f"{wrong.sum()}, any-hit clear {clear.sum()}, max |t - t64| / (D diag) {err:.2e}")
    assert alone.sum() >= 1500, f"{what}: the cell has too few robust rays to mean anything ({alone.sum()})"
    assert lost.sum() == 0, f"{what}: {lost.sum()} of {robust.sum()} robust true hits are not reported (aspect 1:{aspect}, D {D})"
    assert wrong.sum() == 0, f"{what}: {wrong.sum()} robust true hits are reported on another triangle"
    assert clear.sum() == 0, f"{what}: {clear.sum()} robust true hits do not occlude"
    assert err <= t_bound(aspect), f"{what}: |t - t64| = {err:.2e} D |diagonal|"


def as_hits(prim, t, u, v):
    from heatray_amd._ffi import HIT_DTYPE
    h = np.empty(prim.shape[0], HIT_DTYPE)
    h["prim"], h["t"], h["u"], h["v"] = prim, t, u, v
    return h


def cell_rays(aspect, plane, eps):
    """[(D, origins, directions, aimed-at, robust, alone, t64)] of a cell"""
    tris = tc.make_cell(aspect, plane)
    out = []
    for D in tc.DISTANCES:
        o, d, k = tc.make_rays(aspect, plane, D)
        out.append((D, o, d, k) + tc.truth(tris, o, d, k, float(eps), D))
    return out


# ------------------------------------------------------------------------------------------------ CPU
def test_the_cells_are_what_they_claim():
    for aspect, plane in CELLS:
        T = tc.make_cell(aspect, plane).astype(np.float64)
        assert np.abs(T).max() == 1.0 and abs(tc.diagonal(T) - 2 * math.sqrt(3)) < 1e-6        # the anchors span [-1, 1]^3
        e = np.stack([T[:64, 1] - T[:64, 0], T[:64, 2] - T[:64, 0], T[:64, 2] - T[:64, 1]], 1)
        L = np.linalg.norm(e, axis=2).max(axis=1)
        w = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1) / L
        assert np.allclose(L / w, aspect, rtol=1e-2), (aspect, plane)   # (float32 vertices: 0.4 % of the thinnest width)
        if plane in "xyz":   # exactly in an axis-aligned plane: the box has NO thickness on that axis
            assert np.ptp(T[:64, :, "xyz".index(plane)]) == 0.0
        elif plane.startswith("tilt"):   # the plane through all 192 vertices (a single thin triangle's normal feels their rounding)
            P = T[:64].reshape(-1, 3)
            n = np.linalg.svd(P - P.mean(axis=0))[2][2]
            assert abs(math.asin(math.hypot(n[0], n[1])) / float(plane[4:]) - 1) < 0.01, (aspect, plane)


@pytest.mark.parametrize("aspect,plane", CELLS)
def test_every_robust_true_hit_is_reported_restatement_and_oracle(aspect, plane):
    tris = tc.make_cell(aspect, plane)
    sc = tc.scene(tris)
    o, ob = oracle_lib.engine(), oracle_lib.engine()
    sc.apply(o), sc.apply(ob)
    oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
    eps, h, diag = tc.scene_constants(o.scene_info())
    assert eps == F(o.scene_info().ray_epsilon) and abs(float(diag) - 2 * math.sqrt(3)) < 1e-6
    for D, org, d, k, robust, alone, t64 in cell_rays(aspect, plane, eps):
        prim, t, u, v, retried = tc.closest(tris, org, d, eps, h)
        check_truth(as_hits(prim, t, u, v), None, k, robust, alone, t64, aspect, D, float(diag), f"numpy float32 ({retried.sum()} by the retry)")
        ht, hb = o.debug_trace(org, d), ob.debug_trace(org, d)
        assert ht.tobytes() == hb.tobytes(), f"{(ht != hb).sum()} closest hits differ between the tree and brute force"
        at, ab = o.debug_trace(org, d, any_hit=True), ob.debug_trace(org, d, any_hit=True)
        assert at.tobytes() == ab.tobytes()
        check_truth(hb, ab, k, robust, alone, t64, aspect, D, float(diag), "oracle")
        # the restatement IS the contract: the same hit, the same bits
        hit = prim >= 0
        assert np.array_equal(prim, hb["prim"])
        for name, mine in (("t", t), ("u", u), ("v", v)):
            assert mine[hit].tobytes() == hb[name][hit].tobytes(), name
    o.close(), ob.close()


def test_the_retry_is_what_keeps_them_and_the_phantoms_stay_away():
    """Conditions 1-3 alone (the rule before the retry) lose robust true hits on thin boxes — most of them at 1:10 000 — and the
    retry takes none of the fixture's phantom hits back (without its guard, 8 of the 24 return)."""
    tris = tc.make_cell(10000, "z")
    diag = F(tc.diagonal(tris))
    eps, h = F(1e-4) * diag, F(0.5) * (F(1e-5) * diag)
    o, d, k = tc.make_rays(10000, "z", 1.5)
    robust, alone, t64 = tc.truth(tris, o, d, k, float(eps), 1.5)
    before = tc.hit_rule(tris[k, 0], tris[k, 1], tris[k, 2], o, d, eps, np.inf, h, retry=False)[0]
    after = tc.hit_rule(tris[k, 0], tris[k, 1], tris[k, 2], o, d, eps, np.inf, h, retry=True)[0]
    assert (robust & ~before).sum() > 0.5 * robust.sum() and (robust & ~after).sum() == 0
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phantom_hits.npz"))
    for diag in (2.0, 3.5, 7.0):   # (whatever the scene they stand in: h only grows the box)
        eps, h = F(1e-4) * F(diag), F(0.5) * (F(1e-5) * F(diag))
        hit = tc.hit_rule(fx["p0"], fx["p1"], fx["p2"], fx["origin"], fx["direction"], eps, np.inf, h)[0]
        assert not hit.any(), hit.sum()
    e1, e2 = (fx["p1"] - fx["p0"]).astype(np.float64), (fx["p2"] - fx["p0"]).astype(np.float64)
    s = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    assert s.max() < 3e-5 / 5   # the guard's threshold lies a factor of five above every sliver of the fixture ...
    T = tc.make_cell(10000, "free").astype(np.float64)[:64]
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    s = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    assert s.min() > 3e-5 * 4   # ... and well below a real 1:10 000 triangle


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def brute_force_answers():
    """{(aspect, plane): [(D, rays..., truth..., oracle brute force closest, any)]}: computed once, shared by the three builders"""
    out = {}
    for aspect, plane in CELLS:
        tris = tc.make_cell(aspect, plane)
        ob = oracle_lib.engine()
        tc.scene(tris).apply(ob)
        oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
        eps, h, diag = tc.scene_constants(ob.scene_info())
        rows = []
        for D, org, d, k, robust, alone, t64 in cell_rays(aspect, plane, eps):
            hb, ab = ob.debug_trace(org, d), ob.debug_trace(org, d, any_hit=True)
            for a in (hb, ab):
                a.setflags(write=False)
            rows.append((D, org, d, k, robust, alone, t64, hb, ab))
        out[aspect, plane] = (float(diag), rows)
        ob.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["", "ploc=2", "ploc=0"])
def test_gpu_reports_every_robust_true_hit_like_the_oracles_brute_force(monkeypatch, brute_force_answers, tune):
    monkeypatch.setenv("HR_TUNE", tune)
    for aspect, plane in CELLS:
        g = core.create_engine()
        tc.scene(tc.make_cell(aspect, plane)).apply(g)
        diag, rows = brute_force_answers[aspect, plane]
        for D, org, d, k, robust, alone, t64, hb, ab in rows:
            hg, ag = g.debug_trace(org, d), g.debug_trace(org, d, any_hit=True)
            check_truth(hg, ag, k, robust, alone, t64, aspect, D, diag, f"GPU debug_trace [{tune}] {plane}")
            assert hg.tobytes() == hb.tobytes(), f"{(hg != hb).sum()} closest hits differ from the oracle's brute force"
            assert ag.tobytes() == ab.tobytes()
            hq, aq = g.query(org, d), g.query(org, d, any_hit=True)
            assert hq.tobytes() == hb.tobytes(), f"query: {(hq != hb).sum()} closest hits differ from the oracle's brute force"
            assert aq.tobytes() == ab.tobytes()
        g.close()


@pytest.mark.gpu
def test_gpu_keeps_every_robust_true_hit_after_a_refit(brute_force_answers):
    """A deformed mesh keeps the property: the cell's triangles arrive by an in-place vertex update of a smaller copy (a refit)."""
    aspect, plane = 1000, "y"
    tris = tc.make_cell(aspect, plane)
    g = core.create_engine()
    tc.scene((tris * F(0.97)).astype(F)).apply(g)
    g.update_mesh(0, np.ascontiguousarray(tris).reshape(-1, 3))
    g.commit()
    assert g.scene_info().refitted == 1
    diag, rows = brute_force_answers[aspect, plane]
    for D, org, d, k, robust, alone, t64, hb, ab in rows:
        hg, ag = g.debug_trace(org, d), g.debug_trace(org, d, any_hit=True)
        check_truth(hg, ag, k, robust, alone, t64, aspect, D, diag, "GPU after a refit")
        assert hg.tobytes() == hb.tobytes() and ag.tobytes() == ab.tobytes()
        assert g.query(org, d).tobytes() == hb.tobytes()
    g.close()


# ------------------------------------------------------------------------------------------------ render
EMISSION = (0.25, 0.5, 1.0)
FLOOR_Z, BOARD_W, BOARD_PITCH, FLOOR_TURN = F(-0.25), 0.002, 0.0016, 0.3


def board_floor():
    """A floor of 2 x 2 units in the plane z = FLOOR_Z, turned by FLOOR_TURN radians inside it (boards along a coordinate axis are the
    one case float32 Möller–Trumbore gets right: half of its products are exact zeros), of boards 2 long and 0.002 wide (aspect 1:1000,
    every triangle of them too), each overlapping its neighbours by a fifth of its width.  (Sixty-four such boards cover a strip 0.1
    wide; the 2 x 2 floor takes 1 250.)
    A board is two triangles that OVERLAP along its diagonal instead of sharing it — the second one reaches a fifth of a width across —
    so that every point inside the floor lies well inside some triangle and a leak through a shared edge cannot occur."""
    n = int(round((2.0 - BOARD_W) / BOARD_PITCH)) + 1
    y0 = -1.0 + BOARD_PITCH * np.arange(n)
    y0[-1] = 1.0 - BOARD_W
    w, s = BOARD_W, 0.2 * BOARD_W
    z = float(FLOOR_Z)
    tris = []
    for y in y0:
        tris.append([(-1, y, z), (1, y, z), (1, y + w, z)])              # below the diagonal
        tris.append([(-1, y - s, z), (1, y + w - s, z), (-1, y + w, z)])  # above the diagonal lowered by a fifth of the width
    t = np.array(tris, dtype=np.float64)
    c, sn = math.cos(FLOOR_TURN), math.sin(FLOOR_TURN)
    x, y = t[..., 0].copy(), t[..., 1].copy()
    t[..., 0], t[..., 1] = c * x - sn * y, sn * x + c * y
    return t.astype(F)


def floor_scene():
    tris = board_floor()
    sc = scenes.Scene("boards", width=128, height=128, use_multiscatter_lut=False)
    sc.materials[0] = host.bake_pbr(base_color=(0, 0, 0), emissive_color=EMISSION, roughness=1.0, specular_f0=0.0)
    pos = tris.reshape(-1, 3)
    sc.meshes.append(scenes.MeshData(pos, np.tile(np.array([0, 0, 1], F), (pos.shape[0], 1)), np.arange(pos.shape[0], dtype=np.uint32), material_id=0))
    diag = tc.diagonal(tris)
    o = sc.options
    o.max_ray_depth, o.max_render_passes, o.aspect_ratio, o.fstop = 1, 8, 1.0, host.FSTOP_DISABLED
    o.max_channel_value = 4.0
    o.focal_length = 48.0                                             # the turned floor fills 5/6 of the frame
    o.view_matrix = host.orbit_view_matrix(1.5 * diag, 0.0, 0.0, target=(0.0, 0.0, float(FLOOR_Z)))   # 1.5 diagonals above, looking down -z
    o.focus_distance = 1.5 * diag
    return sc, tris, diag


def interior_pixels(sc, diag):
    """Pixels whose footprint on the floor's plane, grown by one pixel on every side, lies inside the floor (float64 projection of the
    pinhole camera straight above: x = (2 u - 1) aspect fovTan dist, the same in y, turned back into the floor's own axes; the floor is
    symmetric under the flips an image convention could add, and so is the set)."""
    W, H = sc.width, sc.height
    fov_tan = sc.options.pass_params(0).fov_tan
    dist = 1.5 * diag
    edges = lambda n: (2.0 * (np.arange(n + 1) / n) - 1.0) * fov_tan * dist
    ex, ey = edges(W) * sc.options.aspect_ratio, edges(H)
    px, py = ex[1] - ex[0], ey[1] - ey[0]
    assert min(px, py) > 0.015
    c, sn = math.cos(FLOOR_TURN), math.sin(FLOOR_TURN)
    inside = np.ones((H, W), bool)
    for sgn in (1.0, -1.0):   # (a mirrored image turns the floor the other way: inside under both)
        for cx in (ex[:-1] - px, ex[1:] + px):
            for cy in (ey[:-1] - py, ey[1:] + py):
                X, Y = cx[None, :], cy[:, None]
                fx, fy = c * X + sgn * sn * Y, -sgn * sn * X + c * Y
                inside &= (np.abs(fx) <= 1.0) & (np.abs(fy) <= 1.0)
    return inside


def check_floor(img, inside, what):
    want = np.array([8 * c for c in EMISSION] + [8.0], dtype=F)
    bad = inside & (img != want).any(axis=-1)
    print(f"{what}: {inside.sum()} interior pixels, {bad.sum()} do not hold 8 x the emission")
    assert inside.sum() > 0.35 * inside.size
    assert bad.sum() == 0, f"{what}: {bad.sum()} of {inside.sum()} interior pixels lost samples through the floor (min weight {img[inside][:, 0].min() / want[0] * 8:.2f} of 8)"


def test_the_board_floor_has_no_seams_and_the_oracle_renders_it_opaque():
    sc, tris, diag = floor_scene()
    T = tris.astype(np.float64)
    assert np.ptp(T[..., 2]) == 0.0
    c, sn = math.cos(FLOOR_TURN), math.sin(FLOOR_TURN)
    x, y = T[..., 0].copy(), T[..., 1].copy()
    T[..., 0], T[..., 1] = c * x + sn * y, -sn * x + c * y            # back into the floor's own axes
    assert abs(np.abs(T[..., :2]).max() - 1.0) < 0.21 * BOARD_W         # (the first board's second triangle reaches a fifth of a width further)
    e = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], T[:, 2] - T[:, 1]], 1)
    L = np.linalg.norm(e, axis=2).max(axis=1)
    assert np.allclose(L / (np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1) / L), 1000, rtol=0.25)
    # every point further than 0.015 inside the floor (less than the one pixel, 0.019, that interior_pixels keeps clear) is WELL inside
    # some triangle: u, v > 0.005, u + v < 0.995 in float64, on 200 000 random points.  (float32 moves u and v of such a triangle by
    # 2^-24 * distance / width ~ 1e-4 from 1.5 diagonals away.)
    rng = np.random.default_rng(5)
    p = rng.uniform(-1 + 0.015, 1 - 0.015, (200000, 2))
    covered = np.zeros(p.shape[0], bool)
    first = np.floor((p[:, 1] + 1.0) / BOARD_PITCH).astype(int)
    for back in range(0, 3):                       # the boards whose width can hold the point
        b = np.clip(first - back, 0, tris.shape[0] // 2 - 1)
        for half in (0, 1):
            t = T[2 * b + half]
            a, e1, e2 = t[:, 0, :2], t[:, 1, :2] - t[:, 0, :2], t[:, 2, :2] - t[:, 0, :2]
            det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            q = p - a
            u = (q[:, 0] * e2[:, 1] - q[:, 1] * e2[:, 0]) / det
            v = (e1[:, 0] * q[:, 1] - e1[:, 1] * q[:, 0]) / det
            covered |= (u > 0.005) & (v > 0.005) & (u + v < 0.995)
    assert covered.all(), (~covered).sum()
    o = oracle_lib.engine()
    sc.apply(o)
    for s in range(8):
        o.render_pass(sc.options.pass_params(s))
    check_floor(o.readback(), interior_pixels(sc, diag), "oracle")
    o.close()


@pytest.fixture(scope="module")
def oracle_floor():
    sc, tris, diag = floor_scene()
    o = oracle_lib.engine()
    sc.apply(o)
    for s in range(8):
        o.render_pass(sc.options.pass_params(s))
    img = o.readback()
    img.setflags(write=False)
    o.close()
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["packets=0", "packets=1,corun=0", "packets=1,corun=2"])
def test_a_floor_of_thin_boards_renders_opaque_however_camera_rays_travel(monkeypatch, oracle_floor, tune):
    # the render path: k_trace, and the packet kernel's lanes (packetTriangles), which debug_trace does not reach
    monkeypatch.setenv("HR_TUNE", tune)
    sc, tris, diag = floor_scene()
    g = core.create_engine()
    sc.apply(g)
    for s in range(8):
        g.render_pass(sc.options.pass_params(s))
    img = g.readback()
    g.close()
    check_floor(img, interior_pixels(sc, diag), f"GPU [{tune}]")
    assert img.tobytes() == oracle_floor.tobytes(), f"{int((img != oracle_floor).any(axis=-1).sum())} pixels differ from the oracle"
