"""tests/tree_audit.py without a GPU: the float32 restatement of the encoders, run over trees a small numpy builder makes, satisfies
every invariant the audit states (so the restatement alone is a valid reference on these inputs), and each way a tree can be subtly
wrong is caught under its own name: a checker that catches nothing proves nothing.

The far-from-origin cases translate the soup by 2^k (1, -0.5, 0.25) for k = 6, 10, 13 and assert their precondition, grid_cell >=
ulp32(grid_lo) per axis: a frame origin grid_lo + g * cell is then a float32 wherever it does not cross into a coarser binade.  Larger
offsets (k >= 14 on this scene's x axis) are outside what the two node formats claim and are left out."""
import numpy as np
import pytest

import tree_audit as ta
from heatray_amd import scenes

F, U = np.float32, np.uint32


def build_topology(positions):
    """A valid topology over (n, 3, 3) triangles: median split over the centroids along the widest axis, collapsed 4-wide (the child with
    the most triangles is opened until there are four), one triangle per leaf, nodes breadth-first, siblings contiguous, inner children
    first, a node's triangles together and descending with the slot.  Returns (topology, Tri array in leaf order)."""
    p = np.asarray(positions, F)
    cent = p.astype(np.float64).mean(axis=1)
    tris = ta.tris_of(p)

    def split(ids):
        c = cent[ids]
        axis = int(np.argmax(c.max(0) - c.min(0)))
        ids = ids[np.argsort(c[:, axis], kind="stable")]
        return ids[: len(ids) // 2], ids[len(ids) // 2:]

    inner_base, n_inner, n_valid, leaf_key, level_start, order = [], [], [], [], [0], []
    level = [np.arange(len(p))]
    while level:
        nxt = []
        first_child = level_start[-1] + len(level)
        for ids in level:
            kids = list(split(ids))
            while len(kids) < 4 and max(len(k) for k in kids) > 1:
                kids[j:j + 1] = split(kids[j := int(np.argmax([len(k) for k in kids]))])
            inner, leaves = [k for k in kids if len(k) > 1], [k for k in kids if len(k) == 1]
            inner_base.append(first_child + len(nxt) if inner else 0), n_inner.append(len(inner)), n_valid.append(len(kids))
            # leaf child c (c >= nInner) is the triangle in slot top - c, top = leafBase + nValid - 1: leafKey = ~top
            leaf_key.append(~(len(order) + len(kids) - 1))
            order += [int(k[0]) for k in reversed(leaves)]
            nxt += inner
        level_start.append(level_start[-1] + len(level))
        level = nxt
    topo = {"inner_base": np.array(inner_base, U), "n_inner": np.array(n_inner), "n_valid": np.array(n_valid), "leaf_key": np.array(leaf_key, np.int32),
            "level_start": level_start}
    return topo, tris[np.array(order)]


def _positions(sc):
    return np.concatenate([m.positions[m.indices.astype(np.int64)].reshape(-1, 3, 3) for m in sc.meshes]).astype(F)


def _hostile():
    from test_gpu_parity import _hostile_scene
    return _hostile_scene()[1]


def _coincident():
    from test_gpu_sah_subtrees import _coincident
    return _positions(_coincident())


def _soup(n, k=None):
    p = _positions(scenes.triangle_soup(n, width=16, height=16))
    if k is not None:
        p = (p.astype(np.float64) + 2.0 ** k * np.array([1.0, -0.5, 0.25])).astype(F)
    return p


CASES = {"soup4": lambda: _soup(4), "soup65": lambda: _soup(65), "soup3000": lambda: _soup(3000), "hostile": _hostile, "coincident": _coincident,
         "soup3000+2^6": lambda: _soup(3000, 6), "soup3000+2^10": lambda: _soup(3000, 10), "soup3000+2^13": lambda: _soup(3000, 13)}
_TREES = {}


def reference_tree(name):
    """the restatement's tree of a case, built once and never changed (the mutation tests copy it)"""
    if name not in _TREES:
        topo, tris = build_topology(CASES[name]())
        _TREES[name] = ta.as_tree(topo, tris, ta.scene_consts(tris))
    return _TREES[name]


def _copy(tree):
    return {k: (dict(v) if isinstance(v, dict) else v.copy()) for k, v in tree.items()}


def _names(tree):
    return {name for name, _ in ta.audit(tree)[0]}


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_satisfies_every_invariant(name):
    tree = reference_tree(name)
    lay = tree["layout"]
    if "+2^" in name:  # the precondition of the far cases
        ulp = np.spacing(np.abs(np.asarray(lay["grid_lo"], F)))
        assert (np.asarray(lay["grid_cell"], F) >= ulp).all(), (lay["grid_cell"], ulp)
    bad, margins = ta.audit(tree, expected_levels=lay["levels"])
    print(name, lay["n_nodes"], "nodes", lay["levels"], "levels", margins)
    assert bad == []
    assert lay["n_nodes"] >= 1 and lay["n_triangles"] == len(tree["tris"])
    assert margins["containment_spare_root_frame"] >= 0 and margins["loosest_plane_node4"] < 1 and margins["loosest_plane_node32"] < 1


def test_a_frame_origin_rounded_to_float32_is_caught_far_from_the_origin():
    """k_encode32 before this audit: origin = fmaf(g, cell, gLo) in float32.  Harmless at the origin, 3.4 hit_pad into a triangle at 2^10"""
    for name, caught in (("soup3000", False), ("soup3000+2^10", True)):
        tree = _copy(reference_tree(name))
        tree["node32"] = ta.encode(ta.topology_of(tree), tree["tris"], tree["layout"], frame=F)["node32"]
        bad, margins = ta.audit(tree)
        print(name, margins["containment_spare_node32"])
        assert ({n for n, _ in bad} == {"containment/node32"}) == caught and (bad == []) != caught


def test_the_builder_makes_every_kind_of_node():
    kinds, deepest = set(), 0
    for name in ("soup65", "soup3000", "hostile"):
        t = ta.topology_of(reference_tree(name))
        kinds |= set(zip(t["n_inner"].tolist(), t["n_valid"].tolist()))
        deepest = max(deepest, len(t["level_start"]) - 1)
    assert (4, 4) in kinds and any(i == 0 for i, v in kinds) and any(0 < i < v for i, v in kinds) and deepest > 4, kinds


# ---- mutations


def _slot_to_move(tree, level, fmt, side):
    """(node, slot, axis) at `level` whose plane can move a quantum inwards and MUST then cut a triangle: the widest valid slot of the node
    with the coarsest quantum, on an axis where the spare to the triangles below is less than that quantum"""
    lay = tree["layout"]
    ls = lay["level_start"]
    level = level if level >= 0 else int(lay["levels"]) + level
    qlo, qhi = (ta.planes4 if fmt == "node4" else ta.planes32)(tree[fmt])
    scale = ta.frame4(tree["node4"])[1] if fmt == "node4" else ta.frame32(tree["node32"], lay)[1]
    t = ta.topology_of(tree)
    best = None
    for i in range(int(ls[level]), int(ls[level + 1])):
        for c in range(int(t["n_valid"][i])):
            for a in range(3):
                if qhi[i, c, a] - qlo[i, c, a] >= 2 and scale[i, a] > 4 * float(lay["pad"]) and (best is None or scale[i, a] > best[0]):
                    best = (scale[i, a], i, c, a)
    assert best is not None
    return best[1:]


def _bump(tree, fmt, node, slot, axis, side, by):
    """add `by` to one plane byte: the words are (qlo.x, qlo.y, qlo.z, qhi.x, qhi.y, qhi.z) at 4.. of Node4 and 0.. of Node32"""
    word = (4 if fmt == "node4" else 0) + axis + (3 if side == "hi" else 0)
    byte = (int(tree[fmt][node, word]) >> (8 * slot)) & 0xFF
    assert 0 <= byte + by <= 255
    tree[fmt][node, word] = U((int(tree[fmt][node, word]) & ~(0xFF << (8 * slot))) | ((byte + by) << (8 * slot)))


@pytest.mark.parametrize("fmt", ["node4", "node32"])
@pytest.mark.parametrize("level", [-1, 1], ids=["leaf-parent", "upper"])
@pytest.mark.parametrize("side", ["lo", "hi"])
def test_a_plane_one_quantum_too_tight_is_caught_in_its_format_only(fmt, level, side):
    tree = _copy(reference_tree("soup3000"))
    node, slot, axis = _slot_to_move(tree, level, fmt, side)
    _bump(tree, fmt, node, slot, axis, side, +1 if side == "lo" else -1)
    assert _names(tree) == {f"containment/{fmt}"}


@pytest.mark.parametrize("name", ["soup3000", "soup3000+2^13"])
def test_an_exponent_too_small_and_a_grid_byte_too_large_are_caught(name):
    ref = reference_tree(name)
    tree = _copy(ref)
    tree["node4"][0, 3] -= U(1)  # the root's x exponent
    assert "containment/node4" in _names(tree) and "containment/root-frame" in _names(tree)
    tree = _copy(ref)
    assert tree["node32"][0, 6] >> U(28) > 0
    tree["node32"][0, 6] -= U(1 << 28)  # ex of the root's 32-byte node
    assert "containment/node32" in _names(tree) and _names(tree) <= {"containment/node32", "tightness/node32"}  # (lo planes move outwards)
    tree = _copy(ref)
    node = int(np.argmax(tree["node32"][:, 7] & U(0xFF) < 255) if (tree["node32"][0, 7] & U(0xFF)) == 255 else 0)
    tree["node32"][node, 7] += U(1)  # gx: the frame moves up by a cell
    assert "containment/node32" in _names(tree) and "containment/node4" not in _names(tree)


def _leaf_nodes(t):
    """the nodes without inner children that hold the most common number of triangles"""
    pure = t["n_inner"] == 0
    count = np.bincount(t["n_valid"][pure]).argmax()
    return np.nonzero(pure & (t["n_valid"] == count))[0]


def test_leaf_keys_swapped_across_nodes_are_caught():
    tree = _copy(reference_tree("soup3000"))
    t = ta.topology_of(tree)
    full = _leaf_nodes(t)
    a, b = int(full[0]), int(full[-1])
    for arr, col in ((tree["node4"], (slice(None), 11)), (tree["leaf_keys"], (slice(None),))):
        v = arr[col]
        v[a], v[b] = v[b].copy(), v[a].copy()
    names = _names(tree)
    assert "containment/node4" in names and "containment/node32" in names and not any(n.startswith("structure") for n in names)


def test_a_triangle_dropped_named_twice_and_a_wrong_child_count_are_caught():
    ref = reference_tree("soup3000")
    t = ta.topology_of(ref)
    leafy = _leaf_nodes(t)
    tree = _copy(ref)
    tree["node4"][leafy[0], 3] -= U(1 << 27)  # nValid one less: the last leaf child is gone
    assert _names(tree) == {"structure/leaves"}
    tree = _copy(ref)
    tree["node4"][leafy[0], 11] = tree["node4"][leafy[1], 11]  # two nodes name the same triangles
    tree["leaf_keys"][leafy[0]] = tree["leaf_keys"][leafy[1]]
    assert _names(tree) == {"structure/leaves"}
    tree = _copy(ref)
    tree["tris"][5, 9] = tree["tris"][6, 9]  # a prim id twice
    assert _names(tree) == {"structure/prim-ids"}
    tree = _copy(ref)
    tree["slot_of_prim"][[3, 4]] = tree["slot_of_prim"][[4, 3]]
    assert _names(tree) == {"structure/prim-ids"}
    # nInner off by one in Node4 (the topology): a fourth inner child read as a triangle, a first triangle read as an inner child
    tree = _copy(ref)
    tree["node4"][int(np.nonzero(t["n_inner"] == 4)[0][-1]), 3] -= U(1 << 24)
    assert _names(tree) and all(n.startswith("structure/") for n in _names(tree))
    tree = _copy(ref)
    tree["node4"][leafy[0], 3] += U(1 << 24)
    assert _names(tree) == {"structure/children"}
    tree = _copy(ref)
    tree["node32"][0, 6] ^= U(1 << 25)  # ... and in Node32 only
    assert _names(tree) == {"formats/node32-children"}


def test_format_disagreements_are_caught():
    ref = reference_tree("soup65")
    tree = _copy(ref)
    tree["leaf_keys"][1] += 1
    assert _names(tree) == {"formats/leaf-keys"}
    tree = _copy(ref)
    tree["node4"][2, 13] = 7
    assert _names(tree) == {"formats/node4-d"}
    tree = _copy(ref)
    t = ta.topology_of(tree)
    node = int(np.nonzero(t["n_valid"] < 4)[0][0])
    tree["node32"][node, 0] &= U(0x00FFFFFF)  # the empty fourth slot's qlo.x = 0: it could be entered
    assert _names(tree) == {"formats/node32-empty-slot"}


def test_a_box_loosened_by_three_quanta_is_caught_by_the_tightness_check_alone():
    for fmt in ("node4", "node32"):
        tree = _copy(reference_tree("soup3000"))
        qlo, _ = (ta.planes4 if fmt == "node4" else ta.planes32)(tree[fmt])
        valid = np.arange(4)[None, :] < ta.topology_of(tree)["n_valid"][:, None]
        node, slot, axis = [int(v[0]) for v in np.nonzero((qlo >= 3) & valid[:, :, None])]
        _bump(tree, fmt, node, slot, axis, "lo", -3)
        assert _names(tree) == {f"tightness/{fmt}"}


def test_a_stale_node_box_is_caught():
    tree = _copy(reference_tree("soup3000"))
    tree["node_box"][7, 3:6] = np.nextafter(tree["node_box"][7, 3:6], F(np.inf))  # one ulp on the large side: no ray test would see it
    assert _names(tree) == {"nodebox"}
    tree = _copy(reference_tree("soup3000"))
    tree["node_box"][7, 0] = np.nextafter(tree["node_box"][7, 0], F(-np.inf))
    assert _names(tree) == {"nodebox", "formats/node4-origin"}


def test_a_frame_two_powers_of_two_too_coarse_is_caught():
    ref = reference_tree("soup3000")
    enc = ta.encode(ta.topology_of(ref), ref["tris"], ref["layout"])
    assert ta.bytes_differ(ref, enc) == {}
    # node 9 of the 64-byte format re-encoded with its x exponent two higher: conservative, tight to its (coarser) quantum, only wasteful.
    # (The smallest scale has 255 * s >= extent, so four times it breaks 255 * s < 4 * extent whatever the guard did.)
    tree, i = _copy(ref), 9
    s = ta.pow2((int(tree["node4"][i, 3]) & 0xFF) + 2).astype(np.float64)
    nv = int(ta.topology_of(ref)["n_valid"][i])
    lo = np.floor((enc["child_lo"][i, :, 0].astype(np.float64) - float(enc["node_box"][i, 0])) / s)
    hi = np.ceil((enc["child_hi"][i, :, 0].astype(np.float64) - float(enc["node_box"][i, 0])) / s)
    lo[nv:], hi[nv:] = 255, 0
    tree["node4"][i, 3] += U(2)
    tree["node4"][i, 4], tree["node4"][i, 7] = ta._pack4(lo[None])[0], ta._pack4(hi[None])[0]
    assert _names(tree) == {"quantum/node4"}
