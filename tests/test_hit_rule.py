"""The hit test's second half (hr_trace.h / oracle_bvh.cpp: hitInTriBox): a Möller–Trumbore candidate is a hit only if
its hit point lies inside the triangle's own bounding box grown by half the leaf padding.

float32 Möller–Trumbore alone accepts, about once in 10^9 rays of the benchmark soup, a ray that passes a SLIVER triangle at a distance;
whether a traversal ever tests that triangle depends on the boxes of its tree, so "the hit is defined by the triangle test alone" was
false for such rays.  tests/golden/phantom_hits.npz holds 24 of them (seeded search, tests/golden/make_phantoms.py).
CPU part: the fixture really is what it claims (numpy float32 restatement), the oracle turns every phantom away with its tree AND by
brute force, and real hits are untouched.  GPU part: the library agrees with the oracle's brute force on the phantoms and on a scene
made of slivers, whichever tree it walks and however the rays travel."""
import os

import numpy as np
import pytest

import oracle_lib
from heatray_amd import core, host, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
f = np.float32


def _fixture():
    return np.load(os.path.join(HERE, "golden", "phantom_hits.npz"))


def _scene(tris, name="slivers"):
    """tris: (n, 3, 3) float32 vertex positions, identity transform (the engines form v0, e1 = p1 - p0, e2 = p2 - p0 from them)."""
    sc = scenes.Scene(name, width=32, height=32)
    pos = np.ascontiguousarray(tris, dtype=f).reshape(-1, 3)
    nrm = np.tile(np.array([0, 0, 1], f), (pos.shape[0], 1))
    sc.materials = scenes._material_palette(scenes.SplitMix64(1), 2)
    sc.meshes.append(scenes.MeshData(pos, nrm, np.arange(pos.shape[0], dtype=np.uint32), material_id=0))
    sc.lights.add_directional(color=(1, 1, 1), illuminance=10.0, phi=0.3, theta=0.5)
    scenes._camera_for(sc, np.array([-1, -1, -1], f), np.array([1, 1, 1], f))
    sc.options.max_ray_depth, sc.options.max_render_passes = 3, 8
    sc.options.fstop = host.FSTOP_DISABLED
    return sc


def _phantom_scene():
    """The fixture's slivers plus 400 ordinary triangles (so that there is a tree, and real hits to keep)."""
    fx = _fixture()
    sl = np.stack([fx["p0"], fx["p1"], fx["p2"]], axis=1)
    rng = np.random.default_rng(3)
    c = rng.uniform(-1, 1, (400, 1, 3))
    ordinary = (c + rng.normal(scale=0.05, size=(400, 3, 3))).astype(f)
    return _scene(np.concatenate([sl, ordinary])), fx, ordinary


def _sliver_soup(n=20000, seed=7):
    """n triangles whose third vertex lies on the edge of the other two up to float32 rounding — every one a phantom-hit candidate."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-1, 1, (n, 3)).astype(f)
    e1 = (rng.normal(size=(n, 3)) * 0.05).astype(f)
    s = rng.uniform(0.2, 0.9, (n, 1)).astype(f)
    p1 = (p0 + e1).astype(f)
    p2 = (p0 + e1 * s + rng.normal(size=(n, 3)).astype(f) * f(3e-8)).astype(f)
    return np.stack([p0, p1, p2], axis=1)


def _rays_past(tris, n, seed, noise=1e-7):
    """Rays from a camera's distance through the LINE a sliver's vertices lie on, mostly outside the segment the sliver occupies (and a
    seventh of them through it: real hits): the configuration in which the determinant is rounding noise.  Without the hit test's
    second half the oracle's tree and its brute force disagree on ~3 % of such rays (1696 of 60000 at noise 0)."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * 3.0).astype(f)
    k = rng.integers(0, tris.shape[0], n)
    s = rng.uniform(-3, 4, (n, 1)).astype(f)
    q = tris[k, 0] + (tris[k, 1] - tris[k, 0]) * s + rng.normal(scale=noise, size=(n, 3)).astype(f)
    d = q - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f)


# ------------------------------------------------------------------------------------------------ CPU
def test_the_fixture_holds_phantom_hits_of_float32_moller_trumbore():
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_phantoms import moller_trumbore
    fx = _fixture()
    ok, t, u, v = moller_trumbore(fx["p0"], fx["p1"], fx["p2"], fx["origin"], fx["direction"])
    assert ok.all() and (t > 1e-3).all()                      # the triangle test's first half accepts every one of them
    assert t.tobytes() == fx["t"].tobytes()
    P = fx["origin"] + t[:, None] * fx["direction"]
    lo = np.minimum(np.minimum(fx["p0"], fx["p1"]), fx["p2"])
    hi = np.maximum(np.maximum(fx["p0"], fx["p1"]), fx["p2"])
    miss = np.maximum(np.maximum(lo - P, P - hi), 0).max(axis=1)
    assert (miss > 0.01).all()                                # ... centimetres to metres away from the sliver it "hit"
    # float64 agrees: the rays cross the LINE the three vertices lie on (that is what makes the determinant noise), but outside the
    # segment the sliver occupies — for most of them the closest point of the ray to the segment p0 p1 is centimetres from it
    a, b = fx["p0"].astype(np.float64), fx["p1"].astype(np.float64)
    o, d = fx["origin"].astype(np.float64), fx["direction"].astype(np.float64)
    best = np.full(a.shape[0], np.inf)
    for s in np.linspace(0.0, 1.0, 201):   # (p2 lies between p0 and p1)
        q = a + s * (b - a)
        tt = np.einsum("ij,ij->i", q - o, d) / np.einsum("ij,ij->i", d, d)
        best = np.minimum(best, np.linalg.norm(o + tt[:, None] * d - q, axis=1))
    assert (best > 5e-3).sum() >= 12, best   # (the others graze their sliver at a flat angle: the computed hit POINT is still centimetres off)


def test_oracle_turns_phantoms_away_with_its_tree_and_by_brute_force():
    sc, fx, ordinary = _phantom_scene()
    o, ob = oracle_lib.engine(), oracle_lib.engine()
    sc.apply(o), sc.apply(ob)
    oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
    n_sl = fx["p0"].shape[0]
    # each phantom ray, with everything but its own sliver out of the way (tmax just behind the phantom distance)
    tm = (fx["t"] * f(1.001)).astype(f)
    for eng in (o, ob):
        h = eng.debug_trace(fx["origin"], fx["direction"], tmax=tm)
        assert not np.isin(h["prim"], np.arange(n_sl)).any(), h["prim"]
        a = eng.debug_trace(fx["origin"], fx["direction"], tmax=tm, skip_prim=np.where(h["prim"] >= 0, h["prim"], -1).astype(np.int32), any_hit=True)
        assert a.tobytes() == eng.debug_trace(fx["origin"], fx["direction"], tmax=tm, skip_prim=np.where(h["prim"] >= 0, h["prim"], -1).astype(np.int32),
                                              any_hit=True).tobytes()
    assert o.debug_trace(fx["origin"], fx["direction"]).tobytes() == ob.debug_trace(fx["origin"], fx["direction"]).tobytes()
    # real hits are untouched: rays aimed at the ordinary triangles' centroids hit (mostly the triangle aimed at), tree == brute force
    rng = np.random.default_rng(11)
    org = rng.uniform(-2.5, 2.5, (4000, 3)).astype(f)
    cent = ordinary.mean(axis=1)
    k = rng.integers(0, cent.shape[0], 4000)
    d = cent[k] - org
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f)
    h, hb = o.debug_trace(org, d), ob.debug_trace(org, d)
    assert h.tobytes() == hb.tobytes()
    assert (h["prim"] >= n_sl).mean() > 0.99 and (h["prim"] == k + n_sl).mean() > 0.8
    # ... and against float64 truth, not the oracle's own answer (tests/test_hit_truth.py has the thin triangles): every ray that float64
    # Möller–Trumbore calls a robust hit of the triangle it was aimed at (u, v > 0.1, u + v < 0.9, t > 10 eps, |d.n| > 0.3) is reported —
    # on that triangle or on something in front of it — and where it is reported on that triangle, at float64's distance: these
    # triangles are as wide as they are long, so t carries a few 2^-24 of the coordinates, 1e-5 |diagonal| with a factor of ten to spare
    import thin_cases
    every = np.concatenate([np.stack([fx["p0"], fx["p1"], fx["p2"]], axis=1), ordinary])
    diag = thin_cases.diagonal(every)
    robust, _, t64 = thin_cases.truth(every, org, d, k + n_sl, o.scene_info().ray_epsilon, 1.0)
    assert robust.sum() > 1000, robust.sum()
    assert (h["prim"][robust] >= 0).all(), f"{(h['prim'][robust] < 0).sum()} robust true hits are not reported"
    assert (h["t"][robust] <= t64[robust] + 1e-5 * diag).all()
    on = robust & (h["prim"] == k + n_sl)
    assert on.sum() > 0.8 * robust.sum() and np.abs(h["t"][on] - t64[on]).max() <= 1e-5 * diag
    o.close(), ob.close()


def test_oracle_tree_equals_brute_force_on_a_scene_of_slivers():
    tris = _sliver_soup(3000)
    sc = _scene(tris)
    o, ob = oracle_lib.engine(), oracle_lib.engine()
    sc.apply(o), sc.apply(ob)
    oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
    for noise in (0.0, 1e-7, 1e-5):
        org, d = _rays_past(tris, 60000, 5, noise)
        h, hb = o.debug_trace(org, d), ob.debug_trace(org, d)
        assert h.tobytes() == hb.tobytes(), f"{(h != hb).sum()} closest hits differ between the tree and brute force"
        tm = np.full(org.shape[0], 6.0, f)
        assert o.debug_trace(org, d, tmax=tm, any_hit=True).tobytes() == ob.debug_trace(org, d, tmax=tm, any_hit=True).tobytes()
    o.close(), ob.close()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["", "ploc=2", "ploc=0"])
def test_gpu_turns_phantoms_away_like_the_oracles_brute_force(monkeypatch, tune):
    monkeypatch.setenv("HR_TUNE", tune)
    sc, fx, ordinary = _phantom_scene()
    g, ob = core.create_engine(), oracle_lib.engine()
    sc.apply(g), sc.apply(ob)
    oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
    tm = (fx["t"] * f(1.001)).astype(f)
    hg, hb = g.debug_trace(fx["origin"], fx["direction"], tmax=tm), ob.debug_trace(fx["origin"], fx["direction"], tmax=tm)
    assert hg.tobytes() == hb.tobytes()
    assert not np.isin(hg["prim"], np.arange(fx["p0"].shape[0])).any()
    assert g.debug_trace(fx["origin"], fx["direction"]).tobytes() == ob.debug_trace(fx["origin"], fx["direction"]).tobytes()
    ag = g.debug_trace(fx["origin"], fx["direction"], tmax=tm, any_hit=True)
    assert ag.tobytes() == ob.debug_trace(fx["origin"], fx["direction"], tmax=tm, any_hit=True).tobytes()
    g.close(), ob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["", "ploc=2"])
def test_gpu_equals_brute_force_on_a_scene_of_slivers(monkeypatch, tune):
    monkeypatch.setenv("HR_TUNE", tune)
    tris = _sliver_soup(20000)
    sc = _scene(tris)
    g, ob = core.create_engine(), oracle_lib.engine()
    sc.apply(g), sc.apply(ob)
    oracle_lib.load().ora_set_brute_force(ob._ctx, 1)
    for noise in (0.0, 1e-7, 1e-5):
        org, d = _rays_past(tris, 30000, 9, noise)
        hg, hb = g.debug_trace(org, d), ob.debug_trace(org, d)
        assert hg.tobytes() == hb.tobytes(), f"{(hg != hb).sum()} closest hits differ from brute force"
        tm = np.full(org.shape[0], 6.0, f)
        assert g.debug_trace(org, d, tmax=tm, any_hit=True).tobytes() == ob.debug_trace(org, d, tmax=tm, any_hit=True).tobytes()
    g.close(), ob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["packets=0", "packets=1,corun=0", "packets=1,corun=2"])
def test_sliver_scene_renders_bit_exact_however_camera_rays_travel(monkeypatch, golden, tune):
    # the render path (k_trace, and the packet kernel's lanes, which test every triangle their PACKET reaches) against the oracle
    monkeypatch.setenv("HR_TUNE", tune)
    tris = _sliver_soup(20000)
    # slivers as wide as a pixel so that camera rays graze them all the time
    sc = _scene(tris)
    sc.width, sc.height = 256, 256
    g, o = core.create_engine(), oracle_lib.engine()
    sc.apply(g, lut=golden["multiscatter_lut"]), sc.apply(o, lut=golden["multiscatter_lut"])
    for s in range(8):
        g.render_pass(sc.options.pass_params(s)), o.render_pass(sc.options.pass_params(s))
    a, b = g.readback(), o.readback()
    assert a.tobytes() == b.tobytes(), f"{int((a != b).any(axis=-1).sum())} pixels differ"
    g.close(), o.close()
