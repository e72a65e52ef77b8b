"""The committed tree, read back (include/hrcore_tree.h: hr_scene_tree_layout, hr_scene_tree_read) and held to tests/tree_audit.py:
the float64 audit of every node box — structure, agreement of the two node formats, containment of every triangle grown by hit_pad
in every box above it with zero tolerance, tightness, the nodeBox array — and byte equality with the float32 restatement of the
encoders over the device's own topology.  After builds by both builders with and without the SAH subtrees, after refits (a translation,
an anisotropic scale, a shrink, a pose) and the rebuild behind the 1.25 x guard, for a tree from the cache file and for scenes far from
the origin.  The scenes are test_gpu_sah_subtrees.SCENES: 1 to ~8500 triangles reach every branch of the build.

Byte equality holds at build time too: k_collapse4 unites the boxes of the binary tree, k_refit4 and k_encode32 those of the 4-wide
tree, and a union by min / max does not depend on the grouping."""
import ctypes as C

import numpy as np
import pytest

import tree_audit as ta
from heatray_amd import _ffi as ffi
from heatray_amd import core, scenes
from test_gpu_sah_subtrees import SCENES, _engine

pytestmark = pytest.mark.gpu

F = np.float32
TUNES = ("", "sahsub=0", "ploc=0", "ploc=2")


def check(g, what, consts_from_triangles=True):
    """audit + byte equality of the engine's committed tree; returns (tree, margins)"""
    tree, info = g.tree_readback(), g.scene_info()
    lay = tree["layout"]
    assert (lay["n_nodes"], lay["n_triangles"], lay["levels"]) == (info.n_nodes, info.n_triangles, info.bvh_levels)
    assert lay["ray_epsilon"] == info.ray_epsilon and list(lay["lo"]) == list(info.aabb_min) and list(lay["hi"]) == list(info.aabb_max)
    bad, margins = ta.audit(tree, expected_levels=info.bvh_levels)
    spares = {k: round(v, 4) for k, v in margins.items() if k.startswith("containment")}
    print(f"{what}: {lay['n_nodes']} nodes, {lay['levels']} levels, builder {info.builder}, refitted {info.refitted}, spare / hit_pad {spares}")
    assert bad == [], what
    if consts_from_triangles:  # k_scene_consts and gridOf, restated from the triangles the tree holds
        want = ta.scene_consts(tree["tris"])
        for k, v in want.items():
            assert np.array_equal(np.asarray(lay[k], np.asarray(v).dtype).view(np.uint32), np.asarray(v).view(np.uint32)), (what, k, lay[k], v)
    if lay["n_nodes"]:
        assert ta.bytes_differ(tree, ta.encode(ta.topology_of(tree), tree["tris"], lay)) == {}, what
    return tree, margins


@pytest.mark.parametrize("tune", TUNES, ids=[t or "default" for t in TUNES])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_build_passes_the_audit_and_is_the_restatements_bytes(monkeypatch, name, tune):
    sc = SCENES[name]()
    g = _engine(monkeypatch, tune)
    sc.apply(g)
    tree, _ = check(g, f"{name} [{tune}]")
    assert g.scene_info().refitted == 0 and tree["layout"]["n_triangles"] == sc.n_triangles
    if tune == "ploc=2" and name == "soup3000":
        assert g.scene_info().builder == 1
    if tune == "ploc=0":
        assert g.scene_info().builder == 0
    g.close()


def _box_area_ratio_is(g, tree, built_ratio, what):
    """hr_scene_info's box_area_ratio against float64 over the read-back arrays; n_nodes * 2^-23: the worst case of the float32 sums"""
    want = ta.area_ratio(tree["node_box"], tree["tris"]) / built_ratio
    got = g.scene_info().box_area_ratio
    print(f"{what}: box_area_ratio {got:.7f}, float64 {want:.7f}")
    assert abs(got - want) <= int(tree["layout"]["n_nodes"]) * 2.0 ** -23, (what, got, want)


def _scale(x, y, z):
    return np.diag([x, y, z, 1.0]).astype(F)


@pytest.mark.parametrize("name", ["soup3000", "terrain120x60"])
def test_every_refit_passes_the_audit_and_the_guard_rebuilds(name):
    sc = scenes.triangle_soup(3000, width=16, height=16) if name == "soup3000" else scenes.terrain(120, 60, width=16, height=16)
    g = core.create_engine()
    sc.apply(g)
    tree, _ = check(g, f"{name} built")
    built = ta.area_ratio(tree["node_box"], tree["tris"])
    _box_area_ratio_is(g, tree, built, f"{name} built")
    meshes = range(len(sc.meshes))

    def refit(what, edit, want_refit=1):
        edit()
        g.commit()
        assert g.scene_info().refitted == want_refit, (what, g.scene_info().box_area_ratio)
        return check(g, f"{name} {what}")[0]

    t = refit("translated", lambda: [g.set_transform(m, scenes._translate(0.31, -0.17, 0.05)) for m in meshes])
    _box_area_ratio_is(g, t, built, "translated")
    t = refit("scaled by diag(2.5, 0.4, 1.7)", lambda: [g.set_transform(m, _scale(2.5, 0.4, 1.7)) for m in meshes])
    _box_area_ratio_is(g, t, built, "scaled")
    big = t["node_box"][0, 3:6] - t["node_box"][0, 0:3]
    # a uniform shrink through the vertices: a refit that only ever grew its boxes would keep the hits and fail the tightness rule
    t = refit("shrunk to 0.5", lambda: [g.update_mesh(m, sc.meshes[m].positions * F(0.5)) for m in meshes])
    _box_area_ratio_is(g, t, built, "shrunk")
    small = t["node_box"][0, 3:6] - t["node_box"][0, 0:3]
    assert (small < 0.51 * big).all() and (small > 0.49 * big).all()
    rng = np.random.default_rng(11)
    rest = sc.meshes[0].positions * F(0.5)
    g.deform_bind(0, morph_positions=rng.uniform(-0.01, 0.01, (1,) + rest.shape).astype(F))
    t = refit("posed", lambda: g.deform_pose(0, morph_weights=[1.0]))
    _box_area_ratio_is(g, t, built, "posed")
    # ... and a step behind which the boxes are more than 1.25 x what the build left: the commit rebuilds
    if name == "soup3000":   # every triangle of one mesh flung, rigidly, somewhere in a box many times the scene's size
        flung = (rest.reshape(-1, 3, 3) + rng.uniform(-8, 8, (len(rest) // 3, 1, 3))).reshape(-1, 3).astype(F)
        edit = lambda: g.update_mesh(0, flung)  # noqa: E731
    else:                    # the height field turned 45 degrees about z: flat boxes become fat ones
        c = np.sqrt(0.5)
        turn = np.array([[c, -c, 0, 0], [c, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F)
        edit = lambda: g.set_transform(0, turn)  # noqa: E731
    t = refit("past the guard", edit, want_refit=0)
    _box_area_ratio_is(g, t, ta.area_ratio(t["node_box"], t["tris"]), "rebuilt")
    g.close()


def test_a_tree_from_the_cache_file_passes_the_audit(monkeypatch, tmp_path):
    sc = scenes.triangle_soup(3000, width=16, height=16)
    trees = []
    for want in (0, 2):
        g = _engine(monkeypatch, "")
        g.set_scene_cache(tmp_path / "scene.hrbvh")
        sc.apply(g)
        assert g.scene_info().refitted == want
        trees.append(check(g, f"cache, refitted {want}")[0])
        g.close()
    assert all(trees[0][k].tobytes() == trees[1][k].tobytes() for k in ("node4", "node32", "leaf_keys", "tris", "node_box", "slot_of_prim"))


@pytest.mark.parametrize("tune", ["ploc=0", "ploc=2"])
@pytest.mark.parametrize("k", [6, 10, 13])
def test_far_from_the_origin(monkeypatch, k, tune):
    """the soup translated by 2^k (1, -0.5, 0.25), as in test_tree_audit_ref.py: there the float32 frame origin k_encode32 used to round
    cut 3.4 hit_pad into triangles at 2^10"""
    sc = scenes.triangle_soup(3000, width=16, height=16)
    off = 2.0 ** k * np.array([1.0, -0.5, 0.25])
    for m in sc.meshes:
        m.positions = (m.positions.astype(np.float64) + off).astype(F)
    g = _engine(monkeypatch, tune)
    sc.apply(g)
    lay = check(g, f"soup3000 + 2^{k} [{tune}]")[0]["layout"]
    assert (lay["grid_cell"] >= np.spacing(np.abs(lay["grid_lo"]))).all()  # the precondition: a cell is no finer than the coordinates
    g.close()


def test_refusals_and_a_readback_between_passes():
    sc = scenes.cornell_box(32, 32, bounces=3, passes=4)
    g = core.create_engine()
    lay, buf = ffi.TreeLayout(), np.zeros(1 << 16, np.uint8)

    def refused(match, call, *args):
        with pytest.raises(ffi.EngineError, match=match):
            g._feature_call("tree", call, *args)

    refused("scene not committed", "scene_tree_layout", C.byref(lay))  # before the first commit
    refused("scene not committed", "scene_tree_read", ffi.HR_TREE_NODE4, buf.ctypes.data, buf.nbytes)
    with pytest.raises(ffi.EngineError, match="scene not committed"):
        g.tree_readback()
    sc.apply(g)
    refused("null output", "scene_tree_layout", None)
    g._feature_call("tree", "scene_tree_layout", C.byref(lay))
    assert lay.n_nodes > 0 and lay.bytes[ffi.HR_TREE_NODE4] == 64 * lay.n_nodes and lay.bytes[ffi.HR_TREE_TRIS] == 48 * lay.tri_slots
    for what in (-1, ffi.HR_TREE_ARRAYS):
        refused("no such array", "scene_tree_read", what, buf.ctypes.data, buf.nbytes)
    refused("null output", "scene_tree_read", ffi.HR_TREE_NODE4, None, buf.nbytes)
    buf[:] = 0xAB
    refused("shorter than the array", "scene_tree_read", ffi.HR_TREE_NODE4, buf.ctypes.data, lay.bytes[ffi.HR_TREE_NODE4] - 1)
    assert (buf == 0xAB).all()  # (a refused read writes nothing)
    g.set_transform(0, scenes._translate(0.01, 0, 0))  # an edit: no scene until the next commit
    refused("scene not committed", "scene_tree_layout", C.byref(lay))
    g.commit()
    check(g, "cornell box", consts_from_triangles=True)
    # a readback between passes leaves the frame's bits alone
    frames = []
    for read in (False, True):
        g.clear()
        for s in range(3):
            g.render_pass(sc.options.pass_params(s))
            if read:
                g.tree_readback()
        frames.append(g.readback())
    assert np.isfinite(frames[0]).all() and frames[0][..., :3].max() > 0 and frames[0].tobytes() == frames[1].tobytes()
    g.close()
    grp = core.create_group([0, 0])
    sc.apply(grp)
    with pytest.raises(ffi.EngineError, match="a context group is not supported"):
        grp.tree_readback()
    with pytest.raises(ffi.EngineError, match="a context group is not supported"):
        grp._feature_call("tree", "scene_tree_read", ffi.HR_TREE_NODE4, buf.ctypes.data, buf.nbytes)
    grp.close()
    # a tile-sharded context holds a whole tree and answers
    half = core.create_engine(rank=1, world=2, tile_size=16)
    sc.apply(half)
    check(half, "rank 1 of 2")
    half.close()
