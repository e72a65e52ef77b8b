"""The committed 4-wide tree against float64 truth: the check of the premise of the hit rule (hr_trace.h: "every
conservative tree's leaf box contains the triangle's box grown by the WHOLE padding, so a hit point inside the half-grown box is inside
every ancestor's box").  numpy only; nothing here imports the device library.

Two parts.

encode(topology, tris, consts) restates, in float32 and in their operation order, the encoders of hr_build.hip: triBounds, the leaf
padding (lo - pad, hi + pad), the bottom-up union, quantExponent, encodeNode4, gridOf / gridCellExponent and k_encode32.  Given a
topology (who is whose child) and the triangles in leaf order it returns the bytes the device holds: nodeBox, Node4, Node32, leafKeys.
One part is float64 on the device and here: k_encode32 takes the frame origin gLo + g * cell, and the planes' distances from it, in
float64, where they are exact.  (It used to round the origin to float32 with one fmaf; this audit found planes cutting 3.4 hit_pad into
triangles on a scene 2^10 units from the origin, where half an ulp of a coordinate exceeds the leaf padding.)

audit(tree) takes what Engine.tree_readback() returns (or encode()'s arrays put into the same dict) and returns (violations, margins):
a list of (name, detail) and a dict of measured figures.  Every decode is done in float64, where it is exact but for the additions
of a quantum far below an ulp of the origin; those round monotonically (a <= b implies fl(o + a) <= fl(o + b)), so each comparison
below holds to float64 resolution, 2^-29 of a float32 ulp.  The 32-byte node is decoded as the TRAVERSAL decodes it, grid_lo + g * cell
+ q * cell * 2^(e - 8) (hr_trace.h: nodeStep32 folds grid_lo and cell into the ray's constants), not with the float32 frame origin the
encoder rounds for itself.

Names of the violations: "structure/..." (the tree is not a tree over the triangles; the audit stops there), "formats/..." (Node4,
Node32, leafKeys and nodeBox disagree), "containment/node4", "containment/node32", "containment/root-frame" (a decoded box does not
contain a triangle below it grown by hit_pad: zero tolerance), "tightness/node4", "tightness/node32" (a decoded plane lies a quantum or
more outside the float32 child box), "quantum/node4", "quantum/node32" (a frame coarser than its encoder makes it) and "nodebox" (not
the float32 union of the padded leaf boxes below it, bit for bit).

The two quantum rules, as read from the encoders: quantExponent picks the smallest power of two s with ext / s <= 255 and may double it
once to guard the rounding of ext / 255, so 255 * s < 4 * ext wherever ext > 0 and the exponent is not clamped (e > 1); k_encode32
raises e while hi - origin > 255 * scale(e), so at e > 0 hi - origin > 255 * scale(e - 1), i.e. 255 * scale < 2 * (hi - origin).
"""
import numpy as np

F = np.float32
U = np.uint32
MAX_STACK = 16 + 160  # kStackLDS + kStackOvf (hr_trace.h): three entries per level of inner nodes


def _f(bits):
    return np.asarray(bits, U).view(F)


def _bits(x):
    return np.ascontiguousarray(x, F).view(U)


def _fmin(x, y):  # hr_math.h: fmin_(x, y) = (y < x) ? y : x
    return np.where(y < x, y, x)


def _fmax(x, y):  # fmax_(x, y) = (x < y) ? y : x
    return np.where(x < y, y, x)


def pow2(e):
    """as_float(e << 23)"""
    return _f(np.asarray(e, U) << U(23))


def tri_bounds(tris):
    """triBounds / hitInTriBoxAxis: min and max over v0, v0 + e1, v0 + e2, formed in float32"""
    t = np.asarray(tris, F)
    v0, p1, p2 = t[:, 0:3], t[:, 0:3] + t[:, 3:6], t[:, 0:3] + t[:, 6:9]
    return _fmin(_fmin(v0, p1), p2), _fmax(_fmax(v0, p1), p2)


def tris_of(positions):
    """(n, 3, 3) vertices -> the (n, 12) float32 Tri array of k_assemble in submission order: v0, e1 = p1 - p0, e2 = p2 - p0, prim id bits"""
    p = np.asarray(positions, F)
    t = np.zeros((p.shape[0], 12), F)
    t[:, 0:3], t[:, 3:6], t[:, 6:9] = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    t[:, 9] = np.arange(p.shape[0], dtype=U).view(F)
    return t


def scene_consts(tris):
    """k_scene_consts and gridOf: bounds, pad = 1e-5 |diagonal|, hit_pad = pad / 2 and the grid of the 32-byte nodes"""
    lo, hi = tri_bounds(tris)
    lo, hi = lo.min(0), hi.max(0)
    e = hi - lo
    diag = np.sqrt(F(F(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]), dtype=F)
    pad = F(1e-5) * diag
    c = {"lo": lo, "hi": hi, "pad": pad, "hit_pad": F(0.5) * pad, "ray_epsilon": F(1e-4) * diag}
    c.update(grid_of(lo, hi, pad))
    return c


def grid_cell_exponent(ext):
    e = (_bits(ext) >> U(23)) & U(0xFF)
    c = np.where(e > 7, e - U(7), U(0))
    return np.clip(c, 24, 230).astype(U)


def grid_of(lo, hi, pad):
    lo, hi, pad = np.asarray(lo, F), np.asarray(hi, F), F(pad)
    g_lo = lo - F(2.0) * pad
    cexp = grid_cell_exponent((hi + F(2.0) * pad) - g_lo)
    return {"grid_lo": g_lo, "grid_cell": pow2(cexp), "grid_cell_exp": cexp}


def quant_exponent(ext):
    ext = np.asarray(ext, F)
    bits = _bits(ext * (F(1.0) / F(255.0)))
    e = (bits >> U(23)) & U(0xFF)
    e = e + ((bits & U(0x007FFFFF)) != 0)
    with np.errstate(over="ignore"):
        e = e + (pow2(e) * F(255.0) < ext)
    return np.clip(e, 1, 254).astype(U)


def topology_of(tree):
    """the topology a read-back tree states in its 64-byte nodes"""
    n4, lay = tree["node4"], tree["layout"]
    meta = n4[:, 3]
    return {"inner_base": n4[:, 10].copy(), "n_inner": ((meta >> U(24)) & U(7)).astype(np.int64), "n_valid": (meta >> U(27)).astype(np.int64),
            "leaf_key": n4[:, 11].view(np.int32).copy(), "level_start": [int(v) for v in lay["level_start"][: int(lay["levels"]) + 1]]}


def _pack4(q):  # (n, 4) bytes -> a dword, byte j = child j
    q = q.astype(U)
    return q[:, 0] | (q[:, 1] << U(8)) | (q[:, 2] << U(16)) | (q[:, 3] << U(24))


def _quantise(clo, chi, origin, inv, valid):
    """floor / ceil of (plane - origin) * inv clamped to a byte; a slot without a child: lo = 255, hi = 0.  (n, 4, 3) -> two (n, 4, 3) uint32"""
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor((clo - origin[:, None, :]) * inv[:, None, :])
        fh = np.ceil((chi - origin[:, None, :]) * inv[:, None, :])
        qlo = _fmin(_fmax(fl, 0.0), 255.0)
        qhi = _fmin(_fmax(fh, 0.0), 255.0)
    qlo = np.where(valid[:, :, None], np.nan_to_num(qlo), 255).astype(U)
    qhi = np.where(valid[:, :, None], np.nan_to_num(qhi), 0).astype(U)
    return qlo, qhi


def encode(topo, tris, consts, frame=np.float64):
    """hr_build.hip's k_refit4 / k_collapse4 + encodeNode4 and k_encode32 over a given topology, in float32.  Returns node_box, node4,
    node32, leaf_keys as the device lays them out, and child_lo / child_hi (n, 4, 3), the float32 child boxes, which the audit's tightness
    rules refer to.  frame=np.float32 is k_encode32 as it was before the audit, with the frame origin rounded to float32: kept so that a
    test can show the audit catching it."""
    tris = np.asarray(tris, F)
    n = len(topo["inner_base"])
    base, n_inner, n_valid = np.asarray(topo["inner_base"], np.int64), np.asarray(topo["n_inner"], np.int64), np.asarray(topo["n_valid"], np.int64)
    leaf_key = np.asarray(topo["leaf_key"], np.int64)
    pad = F(consts["pad"])
    tlo, thi = tri_bounds(tris)
    tlo, thi = tlo - pad, thi + pad
    slot = np.arange(4)[None, :]
    valid, inner = slot < n_valid[:, None], slot < n_inner[:, None]
    leaf_slot = np.where(valid & ~inner, ~(leaf_key[:, None] + slot), 0)
    child = np.where(inner, base[:, None] + slot, 0)
    clo, chi = np.full((n, 4, 3), np.inf, F), np.full((n, 4, 3), -np.inf, F)
    box = np.zeros((n, 6), F)
    ls = topo["level_start"]
    for level in range(len(ls) - 2, -1, -1):
        s = slice(ls[level], ls[level + 1])
        lf = (valid & ~inner)[s]
        clo[s][lf], chi[s][lf] = tlo[leaf_slot[s][lf]], thi[leaf_slot[s][lf]]
        clo[s][inner[s]], chi[s][inner[s]] = box[child[s][inner[s]], 0:3], box[child[s][inner[s]], 3:6]
        nlo, nhi = np.full((s.stop - s.start, 3), np.inf, F), np.full((s.stop - s.start, 3), -np.inf, F)
        for c in range(4):
            v = valid[s, c][:, None]
            nlo, nhi = np.where(v, _fmin(nlo, clo[s, c]), nlo), np.where(v, _fmax(nhi, chi[s, c]), nhi)
        box[s, 0:3], box[s, 3:6] = nlo, nhi
    blo, bhi = box[:, 0:3], box[:, 3:6]
    # ---- encodeNode4
    e4 = quant_exponent(bhi - blo)
    qlo, qhi = _quantise(clo, chi, blo, F(1.0) / pow2(e4), valid)
    node4 = np.zeros((n, 16), U)
    node4[:, 0:3] = _bits(blo)
    node4[:, 3] = e4[:, 0] | (e4[:, 1] << U(8)) | (e4[:, 2] << U(16)) | (n_inner.astype(U) << U(24)) | (n_valid.astype(U) << U(27))
    node4[:, 4], node4[:, 5], node4[:, 6], node4[:, 7] = _pack4(qlo[:, :, 0]), _pack4(qlo[:, :, 1]), _pack4(qlo[:, :, 2]), _pack4(qhi[:, :, 0])
    node4[:, 8], node4[:, 9] = _pack4(qhi[:, :, 1]), _pack4(qhi[:, :, 2])
    node4[:, 10], node4[:, 11] = base.astype(U), leaf_key.astype(np.int32).view(U)
    # ---- k_encode32
    g_lo, cexp = np.asarray(consts["grid_lo"], F), np.asarray(consts["grid_cell_exp"], U)
    cell, inv_cell = pow2(cexp), pow2(U(254) - cexp)
    g = _fmin(_fmax(np.floor((blo - g_lo) * inv_cell), F(0)), F(255)).astype(U)
    d = frame  # the frame origin g_lo + g * cell and everything measured from it is float64 in k_encode32: exact, as the traversal means it
    origin = g_lo.astype(d) + g.astype(d) * cell.astype(d)
    back = (origin > blo.astype(d)) & (g > 0)  # (the rounding of f)
    g = np.where(back, g - U(1), g)
    origin = g_lo.astype(d) + g.astype(d) * cell.astype(d)
    e32 = np.zeros((n, 3), U)
    for _ in range(15):
        e32 = e32 + ((e32 < 15) & (bhi.astype(d) - origin > d(255.0) * pow2(cexp + e32 - U(8)).astype(d)))
    qlo, qhi = _quantise(clo.astype(d), chi.astype(d), origin, pow2(U(254) - (cexp + e32 - U(8))).astype(d), valid)
    node32 = np.zeros((n, 8), U)
    node32[:, 0], node32[:, 1], node32[:, 2], node32[:, 3] = _pack4(qlo[:, :, 0]), _pack4(qlo[:, :, 1]), _pack4(qlo[:, :, 2]), _pack4(qhi[:, :, 0])
    node32[:, 4], node32[:, 5] = _pack4(qhi[:, :, 1]), _pack4(qhi[:, :, 2])
    node32[:, 6] = (base.astype(U) & U(0x01FFFFFF)) | (n_inner.astype(U) << U(25)) | (e32[:, 0] << U(28))
    node32[:, 7] = g[:, 0] | (g[:, 1] << U(8)) | (g[:, 2] << U(16)) | (e32[:, 1] << U(24)) | (e32[:, 2] << U(28))
    return {"node_box": box, "node4": node4, "node32": node32, "leaf_keys": leaf_key.astype(np.int32), "child_lo": clo, "child_hi": chi}


def as_tree(topo, tris, consts, n_triangles=None):
    """encode()'s arrays in the dict Engine.tree_readback() returns, with the layout the device would report"""
    enc = encode(topo, tris, consts)
    prim = _bits(tris[:, 9])
    n_tri = int((prim != 0xFFFFFFFF).sum()) if n_triangles is None else n_triangles
    slot_of_prim = np.zeros(n_tri, U)
    used = prim != 0xFFFFFFFF
    slot_of_prim[prim[used]] = np.nonzero(used)[0]
    ls = np.zeros(65, U)
    ls[: len(topo["level_start"])] = topo["level_start"]
    lay = {"n_nodes": len(enc["node4"]), "n_triangles": n_tri, "tri_slots": len(tris), "root_leaf_count": 0, "levels": len(topo["level_start"]) - 1,
           "level_start": ls, **{k: consts[k] for k in ("pad", "hit_pad", "ray_epsilon", "grid_lo", "grid_cell", "grid_cell_exp", "lo", "hi")}}
    return {"layout": lay, "tris": np.asarray(tris, F).copy(), "slot_of_prim": slot_of_prim,
            **{k: enc[k] for k in ("node4", "node32", "leaf_keys", "node_box")}}


def _bytes4(w):  # (n,) dwords -> (n, 4): byte j of each
    return np.stack([(w >> U(8 * j)) & U(0xFF) for j in range(4)], axis=1).astype(np.int64)


def planes4(node4):
    """(qlo, qhi) (n, 4, 3) of the 64-byte nodes"""
    return (np.stack([_bytes4(node4[:, 4]), _bytes4(node4[:, 5]), _bytes4(node4[:, 6])], axis=2),
            np.stack([_bytes4(node4[:, 7]), _bytes4(node4[:, 8]), _bytes4(node4[:, 9])], axis=2))


def planes32(node32):
    return (np.stack([_bytes4(node32[:, 0]), _bytes4(node32[:, 1]), _bytes4(node32[:, 2])], axis=2),
            np.stack([_bytes4(node32[:, 3]), _bytes4(node32[:, 4]), _bytes4(node32[:, 5])], axis=2))


def frame4(node4):
    """(origin, scale) (n, 3) float64 of the 64-byte nodes: a.xyz and as_float(e << 23)"""
    meta = node4[:, 3]
    e = np.stack([meta & U(0xFF), (meta >> U(8)) & U(0xFF), (meta >> U(16)) & U(0xFF)], axis=1)
    return node4[:, 0:3].view(F).astype(np.float64), pow2(e).astype(np.float64)


def frame32(node32, lay):
    """(offset from grid_lo, scale, g, e) of the 32-byte nodes as the traversal decodes them: origin = grid_lo + g * cell, scale = cell * 2^(e - 8)"""
    w6, w7 = node32[:, 6], node32[:, 7]
    g = np.stack([w7 & U(0xFF), (w7 >> U(8)) & U(0xFF), (w7 >> U(16)) & U(0xFF)], axis=1).astype(np.float64)
    e = np.stack([w6 >> U(28), (w7 >> U(24)) & U(15), w7 >> U(28)], axis=1).astype(np.int64)
    cell = np.asarray(lay["grid_cell"], F).astype(np.float64)
    return g * cell, cell * np.exp2(e - 8.0), g, e


def audit(tree, expected_levels=None):
    """(violations, margins) of a read-back tree: see the module's docstring"""
    bad, margins = [], {}

    def fail(name, detail):
        bad.append((name, detail))

    lay = tree["layout"]
    n, n_tri, slots = int(lay["n_nodes"]), int(lay["n_triangles"]), int(lay["tri_slots"])
    n4, n32, tris = tree["node4"], tree["node32"], np.asarray(tree["tris"], F)
    levels = int(lay["levels"])
    if expected_levels is not None and levels != int(expected_levels):
        fail("structure/levels", f"layout says {levels}, scene_info {expected_levels}")
    if int(lay["root_leaf_count"]) > 0:  # the trivial case: the root is a leaf, there are no nodes
        if n != 0 or levels != 0 or int(lay["root_leaf_count"]) != n_tri or slots < n_tri:
            fail("structure/root-leaf", f"{n} nodes, {levels} levels, {lay['root_leaf_count']} of {n_tri} triangles in {slots} slots")
        prim = _bits(tris[:, 9])[:n_tri]
        if sorted(prim.tolist()) != list(range(n_tri)) or not np.array_equal(tree["slot_of_prim"][prim], np.arange(n_tri)):
            fail("structure/prim-ids", "a root leaf's prim ids are not a permutation that slot_of_prim inverts")
        return bad, margins
    # ---- structure
    if not (len(n4) == len(n32) == len(tree["leaf_keys"]) == len(tree["node_box"]) == n and len(tris) == slots and len(tree["slot_of_prim"]) == n_tri and n > 0):
        fail("structure/sizes", "the arrays do not have the layout's sizes")
        return bad, margins
    ls = [int(v) for v in lay["level_start"][: levels + 1]]
    if levels < 1 or ls[0] != 0 or (levels >= 1 and ls[1] != 1) or ls[-1] != n or any(b <= a for a, b in zip(ls, ls[1:])):
        fail("structure/levels", f"level_start {ls} does not partition {n} nodes into {levels} levels with node 0 alone at the top")
        return bad, margins
    if 3 * levels > MAX_STACK:
        fail("structure/levels", f"{levels} levels do not fit the traversal stack")
    topo = topology_of(tree)
    base, n_inner, n_valid, leaf_key = topo["inner_base"].astype(np.int64), topo["n_inner"], topo["n_valid"], topo["leaf_key"].astype(np.int64)
    if not ((n_inner <= n_valid) & (n_valid <= 4)).all():
        fail("structure/counts", f"nodes {np.nonzero(~((n_inner <= n_valid) & (n_valid <= 4)))[0][:8]}: not 0 <= nInner <= nValid <= 4")
        return bad, margins
    level_of = np.searchsorted(np.asarray(ls), np.arange(n), side="right") - 1
    nxt = np.asarray(ls + [n, n])
    has = n_inner > 0
    out_of_level = has & ((base < nxt[level_of + 1]) | (base + n_inner > nxt[level_of + 2]))
    if out_of_level.any():
        fail("structure/children", f"nodes {np.nonzero(out_of_level)[0][:8]}: inner children outside the next level")
        return bad, margins
    slot = np.arange(4)[None, :]
    valid, inner = slot < n_valid[:, None], slot < n_inner[:, None]
    named = np.bincount((base[:, None] + slot)[inner], minlength=n)
    if named[0] != 0 or (named[1:] != 1).any():
        fail("structure/children", f"nodes {np.nonzero(named != (np.arange(n) > 0))[0][:8]} are not named exactly once as innerBase + j one level up")
        return bad, margins
    leaf = valid & ~inner
    tri_slot = ~(leaf_key[:, None] + slot)
    if ((tri_slot[leaf] < 0) | (tri_slot[leaf] >= slots)).any():
        fail("structure/leaves", "a leaf child ~(leafKey + slot) is outside the triangle array")
        return bad, margins
    uses = np.bincount(tri_slot[leaf], minlength=slots)
    prim = _bits(tris[:, 9])
    if (uses > 1).any() or uses.sum() != n_tri:
        fail("structure/leaves", f"{int((uses > 1).sum())} triangle slots are named more than once, {int(uses.sum())} leaf children for {n_tri} triangles")
        return bad, margins
    if sorted(prim[uses == 1].tolist()) != list(range(n_tri)):
        fail("structure/prim-ids", "the prim ids of the slots the leaves name are not a permutation of 0 .. n_triangles - 1")
        return bad, margins
    if not np.array_equal(tree["slot_of_prim"][prim[uses == 1]], np.nonzero(uses == 1)[0]):
        fail("structure/prim-ids", "slot_of_prim does not invert the prim ids of the leaf-order triangles")
    # ---- the two formats agree
    lo4, hi4 = planes4(n4)
    lo32, hi32 = planes32(n32)
    if not np.array_equal(n32[:, 6] & U(0x01FFFFFF), n4[:, 10] & U(0x01FFFFFF)) or not np.array_equal((n32[:, 6] >> U(25)) & U(7), n_inner.astype(U)):
        fail("formats/node32-children", "Node32 does not carry Node4's innerBase (25 bits) and nInner")
    if not np.array_equal(tree["leaf_keys"].view(U), n4[:, 11]):
        fail("formats/leaf-keys", f"leafKeys differs from Node4.c.w at nodes {np.nonzero(tree['leaf_keys'].view(U) != n4[:, 11])[0][:8]}")
    for name, qlo, qhi in (("node4", lo4, hi4), ("node32", lo32, hi32)):
        if not ((qlo[~valid] == 255).all() and (qhi[~valid] == 0).all()):
            fail(f"formats/{name}-empty-slot", "a slot without a child is not lo = 255, hi = 0")
        if (qlo[valid] > qhi[valid]).any():
            fail(f"formats/{name}-inverted", f"a valid slot has lo > hi at nodes {np.nonzero((qlo > qhi).any(2) & valid)[0][:8]}")
    if not np.array_equal(n4[:, 0:3], _bits(tree["node_box"][:, 0:3])):
        fail("formats/node4-origin", "Node4.a.xyz is not nodeBox.lo")
    if n4[:, 12:16].any():
        fail("formats/node4-d", "Node4.d is not 0")
    # ---- containment: per slot the union of the triangles below it, each grown by hit_pad in float32 as hitInTriBoxAxis grows it
    h = F(lay["hit_pad"])
    tlo, thi = tri_bounds(tris)
    tlo, thi = (tlo - h).astype(np.float64), (thi + h).astype(np.float64)
    ulo, uhi = np.full((n, 4, 3), np.inf), np.full((n, 4, 3), -np.inf)
    nlo, nhi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    child = np.where(inner, base[:, None] + slot, 0)
    for level in range(levels - 1, -1, -1):
        s = slice(ls[level], ls[level + 1])
        ulo[s][leaf[s]], uhi[s][leaf[s]] = tlo[tri_slot[s][leaf[s]]], thi[tri_slot[s][leaf[s]]]
        ulo[s][inner[s]], uhi[s][inner[s]] = nlo[child[s][inner[s]]], nhi[child[s][inner[s]]]
        nlo[s], nhi[s] = ulo[s].min(axis=1), uhi[s].max(axis=1)
    o4, s4 = frame4(n4)
    off32, s32, _, e32 = frame32(n32, lay)
    g_lo = np.asarray(lay["grid_lo"], F).astype(np.float64)
    dec = {"node4": (o4[:, None, :] + lo4 * s4[:, None, :], o4[:, None, :] + hi4 * s4[:, None, :]),
           "node32": (g_lo + (off32[:, None, :] + lo32 * s32[:, None, :]), g_lo + (off32[:, None, :] + hi32 * s32[:, None, :]))}
    unit = float(h) if float(h) > 0 else 1.0
    for name, (dlo, dhi) in dec.items():
        spare = np.minimum(ulo - dlo, dhi - uhi)[valid]
        margins[f"containment_spare_{name}"] = float(spare.min()) / unit
        if (spare < 0).any():
            where = np.nonzero((np.minimum(ulo - dlo, dhi - uhi) < 0).any(2) & valid)
            fail(f"containment/{name}", f"{int((spare < 0).sum())} planes inside a triangle's grown box, worst {float(spare.min()) / unit:.3g} hit_pad, "
                                        f"(node, slot) {list(zip(*[w[:6].tolist() for w in where]))}")
    root_spare = min((nlo[0] - o4[0]).min(), (o4[0] + 255.0 * s4[0] - nhi[0]).min())
    margins["containment_spare_root_frame"] = float(root_spare) / unit
    if root_spare < 0:
        fail("containment/root-frame", f"the root's frame misses a triangle by {-float(root_spare) / unit:.3g} hit_pad")
    # ---- tightness and nodeBox, against the float32 restatement over this topology
    enc = encode(topo, tris, lay)
    clo, chi = enc["child_lo"].astype(np.float64), enc["child_hi"].astype(np.float64)
    for name, (dlo, dhi), scale in (("node4", dec["node4"], s4), ("node32", dec["node32"], s32)):
        slack = np.maximum(clo - dlo, dhi - chi) / scale[:, None, :]
        margins[f"loosest_plane_{name}"] = float(slack[valid].max())
        if (slack[valid] >= 1.0).any():
            where = np.nonzero((slack >= 1.0).any(2) & valid)
            fail(f"tightness/{name}", f"a plane lies {float(slack[valid].max()):.3g} quanta outside its float32 child box, (node, slot) "
                                      f"{list(zip(*[w[:6].tolist() for w in where]))}")
    blo, bhi = enc["node_box"][:, 0:3].astype(np.float64), enc["node_box"][:, 3:6].astype(np.float64)
    e4 = np.stack([n4[:, 3] & U(0xFF), (n4[:, 3] >> U(8)) & U(0xFF), (n4[:, 3] >> U(16)) & U(0xFF)], axis=1)
    coarse4 = (bhi - blo > 0) & (e4 > 1) & ~(255.0 * s4 < 4.0 * (bhi - blo))
    if coarse4.any():
        fail("quantum/node4", f"nodes {np.nonzero(coarse4.any(1))[0][:8]}: 255 * scale >= 4 * extent")
    coarse32 = (e32 > 0) & ~(255.0 * s32 < 2.0 * (bhi - (g_lo + off32)))
    if coarse32.any():
        fail("quantum/node32", f"nodes {np.nonzero(coarse32.any(1))[0][:8]}: 255 * scale >= 2 * (hi - origin) at e > 0")
    if _bits(tree["node_box"]).tobytes() != _bits(enc["node_box"]).tobytes():
        diff = np.nonzero((_bits(tree["node_box"]) != _bits(enc["node_box"])).any(1))[0]
        fail("nodebox", f"{len(diff)} node boxes are not the float32 union of the padded leaf boxes below them, first {diff[:8]}")
    margins["node_area_over_triangle_area"] = area_ratio(tree["node_box"], tris)
    return bad, margins


def area_ratio(node_box, tris):
    """(sum of the node boxes' half surface areas dx dy + dy dz + dz dx) / (sum of the triangles' areas) in float64: what hr_scene_info's
    box_area_ratio compares between a refit and the build before it"""
    b, t = np.asarray(node_box, np.float64), np.asarray(tris, F)
    used = _bits(t[:, 9]) != 0xFFFFFFFF
    d = b[:, 3:6] - b[:, 0:3]
    t = t[used].astype(np.float64)
    tri = 0.5 * np.linalg.norm(np.cross(t[:, 3:6], t[:, 6:9]), axis=1)
    return float((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]).sum() / tri.sum())


def bytes_differ(tree, enc):
    """the arrays of a read-back tree that are not encode()'s bytes: {name: number of differing nodes}"""
    out = {}
    for k in ("node_box", "node4", "node32", "leaf_keys"):
        a, b = np.ascontiguousarray(tree[k]).view(U).reshape(len(tree[k]), -1), np.ascontiguousarray(enc[k]).view(U).reshape(len(enc[k]), -1)
        if a.shape != b.shape or not np.array_equal(a, b):
            out[k] = int((a != b).any(1).sum()) if a.shape == b.shape else -1
    return out
