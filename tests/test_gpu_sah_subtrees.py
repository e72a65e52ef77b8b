"""GPU tests of the full-sweep SAH rebuild of the radix tree's bottom subtrees (hr_build.hip: k_sah_find, k_sah_subtrees; HR_TUNE
sahsub=T, 0 = off): hits and frames do not depend on it, the tree's cost never rises with it and falls on the soup by at least half of
what the numpy prototype (tools/tree_proto.py) finds, a refit keeps working, and the tree cache tells the two settings apart."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib
from heatray_amd import core, host, scenes
from test_gpu_parity import _hostile_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene_of(name, pos):
    sc = scenes.Scene(name, width=16, height=16)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (pos.shape[0] * 3, 1))
    sc.materials = scenes._material_palette(scenes.SplitMix64(2), 1)
    sc.meshes.append(scenes.MeshData(pos.reshape(-1, 3), nrm, np.arange(pos.shape[0] * 3, dtype=np.uint32), material_id=0))
    return sc


def _coincident():
    rng = np.random.default_rng(3)
    one = np.array([[-0.3, -0.2, 0.1], [0.4, -0.1, 0.0], [0.0, 0.5, 0.2]], np.float32)
    filler = rng.uniform(-1, 1, (100, 1, 3)).astype(np.float32) + rng.uniform(-0.1, 0.1, (100, 3, 3)).astype(np.float32)
    return _scene_of("coincident", np.concatenate([np.tile(one[None], (200, 1, 1)), filler]).astype(np.float32))


def _deep():
    # the deliberately deep tree of test_deep_tree_stresses_the_traversal_stack (test_gpu_parity.py)
    rng = np.random.default_rng(123)
    one = np.array([[-0.01, -0.01, 0.5], [0.02, -0.01, 0.5], [-0.01, 0.02, 0.5]], np.float32)
    sheets = []
    for j in range(28):
        c, s = 700.0 * 2.0 ** -j, 2.5 * 700.0 * 2.0 ** -j
        sheets.append([[c - s, c - s, 1.0 + 0.01 * j], [c + 2 * s, c - s, 1.0 + 0.01 * j], [c - s, c + 2 * s, 1.0 + 0.01 * j]])
    filler = rng.uniform(-1000, 1000, (300, 1, 3)).astype(np.float32) + rng.uniform(-30, 30, (300, 3, 3)).astype(np.float32)
    return _scene_of("deep", np.concatenate([np.tile(one[None], (8192, 1, 1)), np.array(sheets, np.float32), filler]).astype(np.float32))


SCENES = {**{f"soup{n}": (lambda n=n: scenes.triangle_soup(n, width=16, height=16)) for n in (1, 2, 3, 4, 64, 65, 128, 3000)},
          "coincident": _coincident, "hostile": lambda: _hostile_scene()[0], "deep": _deep}


def _rays(sc, n=4000):
    """origins around the triangles, half of the rays aimed at one (a ray distribution that works for the hostile and the deep scene too)"""
    rng = np.random.default_rng(5)
    tgt = np.concatenate([m.positions[m.indices.astype(np.int64)].reshape(-1, 3, 3).mean(axis=1) for m in sc.meshes])
    at = tgt[rng.integers(0, tgt.shape[0], n)]
    org = (at + rng.normal(scale=1.5, size=(n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d[: n // 2] = at[: n // 2] + rng.normal(scale=1e-3, size=(n // 2, 3)) - org[: n // 2]
    return org, (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)).astype(np.float32)


def _engine(monkeypatch, tune):
    monkeypatch.setenv("HR_TUNE", tune)
    return core.create_engine()


def _kept_cost(info):
    return info.cost_ploc if info.builder else info.cost_radix


@pytest.mark.parametrize("name", list(SCENES))
def test_hits_equal_the_oracles_with_and_without_the_rebuild_and_the_cost_never_rises(monkeypatch, name):
    sc = SCENES[name]()
    o = oracle_lib.engine()
    sc.apply(o)
    org, d = _rays(sc)
    want = o.debug_trace(org, d)
    if sc.n_triangles >= 64:
        assert (want["prim"] >= 0).sum() > 100
    tm = np.full(len(org), 2.0, np.float32)
    want_any = o.debug_trace(org, d, tmax=tm, skip_prim=want["prim"], any_hit=True)
    infos = {}
    for tune in ("sahsub=64", "sahsub=0", "sahsub=64,packets=1"):
        g = _engine(monkeypatch, tune)
        sc.apply(g)
        infos[tune] = (g.scene_info(), g.tree_info())
        hg = g.debug_trace(org, d)
        assert hg.tobytes() == want.tobytes(), f"{name} {tune}: {(hg != want).sum()} of {len(org)} closest hits differ"
        assert g.debug_trace(org, d, tmax=tm, skip_prim=want["prim"], any_hit=True).tobytes() == want_any.tobytes(), (name, tune)
        g.close()
    (on, ton), (off, toff) = infos["sahsub=64"], infos["sahsub=0"]
    print(f"{name}: cost_radix {off.cost_radix:.4f} -> {on.cost_radix:.4f}, kept {_kept_cost(off):.4f} -> {_kept_cost(on):.4f}, "
          f"subtrees {ton.subtrees_replaced} of {ton.subtrees_found} replaced, levels {off.bvh_levels} -> {on.bvh_levels}")
    # the radix candidate never gets dearer.  The tree that is KEPT is chosen as before (PLOC only where it is 5 % cheaper than the radix
    # candidate, hr_build.hip): where the improved radix tree comes within that margin of a PLOC tree that used to win (the deep scene),
    # it is kept at a cost of at most the PLOC tree's / 0.95; in every other case the kept cost does not rise
    assert on.cost_radix <= off.cost_radix
    assert _kept_cost(on) <= _kept_cost(off) or (off.builder == 1 and on.builder == 0 and 0.95 * on.cost_radix <= off.cost_ploc)
    assert (toff.cost_before, toff.cost_after, toff.subtrees_found, toff.subtrees_replaced, toff.max_triangles) == (0, 0, 0, 0, 0)
    assert ton.max_triangles == 64 and ton.subtrees_replaced <= ton.subtrees_found and ton.cost_after <= ton.cost_before
    if sc.n_triangles > 64:
        assert ton.cost_before == off.cost_radix or off.cost_radix == 0   # the tree before the rebuild is the tree without it
        assert ton.cost_after == on.cost_radix or on.cost_radix == 0
    else:
        assert ton.subtrees_found == 0                                     # no node of more than 64 triangles: nothing to rebuild
    if name == "soup3000":
        assert ton.subtrees_replaced > 20


@pytest.mark.parametrize("packets", ["", ",packets=1"])
def test_a_frame_is_the_same_with_and_without_the_rebuild(monkeypatch, packets):
    sc = scenes.triangle_soup(3000, width=64, height=64, bounces=4, passes=2)
    frames = []
    for tune in ("sahsub=64", "sahsub=0"):
        g = _engine(monkeypatch, tune + packets)
        sc.apply(g)
        for s in range(2):
            g.render_pass(sc.options.pass_params(s))
        frames.append(g.readback())
        g.close()
    assert np.isfinite(frames[0]).all() and frames[0][..., :3].max() > 0
    assert frames[0].tobytes() == frames[1].tobytes()


def test_the_cost_falls_by_at_least_half_of_the_prototypes_reduction(monkeypatch):
    # tools/tree_proto.py on the same 30 000 triangles: the radix tree, and the radix tree with its subtrees of at most 64 triangles rebuilt
    # by sah_sweep, both collapsed by its DP.  The device's collapse and tie-breaks differ from the prototype's: half of its
    # reduction is what shows that the builder works.
    spec = importlib.util.spec_from_file_location("tree_proto", os.path.join(ROOT, "tools", "tree_proto.py"))
    tp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tp)
    sc = scenes.triangle_soup(30000, width=16, height=16)
    pos = np.concatenate([m.positions[m.indices.astype(np.int64)].reshape(-1, 3, 3) for m in sc.meshes])
    lo, hi = pos.min(1), pos.max(1)
    pad = 1e-5 * np.linalg.norm(hi.max(0) - lo.min(0))
    lo, hi = lo - pad, hi + pad
    keys = tp.morton(lo, hi)
    order = np.argsort(keys, kind="stable")
    lo, hi, keys = lo[order], hi[order], keys[order]
    L, R, seq, root = tp.lbvh(keys)
    base = tp.evaluate(L, R, seq, root, lo, hi, "radix tree")
    L, R, seq, root = tp.hybrid(keys, lo, hi, 64, "sah")
    proto = 1.0 - tp.evaluate(L, R, seq, root, lo, hi, "radix tree, subtrees <= 64 by full-sweep SAH") / base
    g = _engine(monkeypatch, "sahsub=64")
    sc.apply(g)
    t = g.tree_info()
    device = 1.0 - t.cost_after / t.cost_before
    print(f"30000-triangle soup: prototype {base:.3f} -{100 * proto:.2f} %, device {t.cost_before:.3f} -> {t.cost_after:.3f} -{100 * device:.2f} %, "
          f"{t.subtrees_replaced} of {t.subtrees_found} subtrees replaced")
    assert proto > 0.03            # (profiles/r4_tree_proto.txt: -5.1 %)
    assert device >= 0.5 * proto


def test_a_refit_of_a_tree_with_rebuilt_subtrees_gives_the_oracles_hits(monkeypatch):
    sc = scenes.triangle_soup(3000, width=16, height=16)
    g, o = _engine(monkeypatch, "sahsub=64"), oracle_lib.engine()
    sc.apply(g), sc.apply(o)
    assert g.tree_info().subtrees_replaced > 20
    org, d = _rays(sc)
    for step in range(2):
        m = scenes._translate(0.01 * (step + 1), 0.02, -0.01)
        g.set_transform(0, m), o.set_transform(0, m)
        g.commit(), o.commit()
        assert g.scene_info().refitted == 1
        assert g.debug_trace(org, d).tobytes() == o.debug_trace(org, d).tobytes()


def test_the_tree_cache_tells_the_two_settings_apart(monkeypatch, tmp_path):
    sc = scenes.triangle_soup(3000, width=16, height=16)
    path = tmp_path / "scene.hrbvh"
    seen = []
    for tune, want in (("sahsub=0", 0), ("sahsub=64", 0), ("sahsub=64", 2), ("sahsub=0", 0)):
        g = _engine(monkeypatch, tune)
        g.set_scene_cache(path)
        sc.apply(g)
        seen.append(g.scene_info().refitted)   # 2: the tree came from the file
        assert seen[-1] == want, (tune, seen)
        g.close()
