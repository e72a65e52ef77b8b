"""Mesh preparation of include/hrcore_mesh.h restated in numpy float32, operation for operation: `reference(positions, indices, ...)`
gives the bits the device kernels (heatray_amd/csrc/hr_mesh.h) give, all three arrays and the eight counters.  It is the checker of the
GPU tests and works without a GPU.

    n, t, b = eng.prepare_mesh(positions, indices, uvs=uvs, params=meshprep.params(want=3))      # on the device
    n, t, b, result = meshprep.reference(positions, indices, uvs=uvs, params=meshprep.params(want=3))   # the same bits, on the host
"""
import numpy as np

from . import _ffi as ffi

F = np.float32
NO_CORNER = np.uint32(0xFFFFFFFF)  # "no non-degenerate corner"
RESULT_KEYS = tuple(k for k, _ in ffi.MeshResult._fields_)

_PI, _PIO2, _PIO4 = F(3.14159265358979323846), F(1.5707963267948966192), F(0.7853981633974483096)
_T_HIGH, _T_LOW = F(2.414213562373095), F(0.4142135623730950)  # atan_'s two range thresholds
_INF = F(np.inf)


def default_params():
    """hr_mesh_default_params: weight ANGLE, weld 1, want NORMALS."""
    return ffi.MeshParams(ffi.HR_MESH_WEIGHT_ANGLE, 1, ffi.HR_MESH_WANT_NORMALS)


def params(weight=ffi.HR_MESH_WEIGHT_ANGLE, weld=1, want=ffi.HR_MESH_WANT_NORMALS):
    return ffi.MeshParams(weight, weld, want)


def _check(p):
    if p.weight not in (ffi.HR_MESH_WEIGHT_ANGLE, ffi.HR_MESH_WEIGHT_AREA, ffi.HR_MESH_WEIGHT_UNIFORM):
        raise ValueError(f"unknown weight {p.weight}")
    if p.weld not in (0, 1):
        raise ValueError(f"weld = {p.weld} is neither 0 nor 1")
    if p.want == 0 or p.want & ~(ffi.HR_MESH_WANT_NORMALS | ffi.HR_MESH_WANT_TANGENTS):
        raise ValueError(f"want = {p.want}")
    if any(p.reserved):
        raise ValueError("reserved words must be 0")


# ---- hr_math.h's functions, one float32 operation per written operation
def atan_(xx):
    xx = np.asarray(xx, F)
    with np.errstate(all="ignore"):
        x = np.abs(xx)
        big = x > _T_HIGH
        mid = ~big & (x > _T_LOW)
        y = np.where(big, _PIO2, np.where(mid, _PIO4, F(0.0))).astype(F)
        x = np.where(big, -(F(1.0) / x), np.where(mid, (x - F(1.0)) / (x + F(1.0)), x)).astype(F)
        z = x * x
        y = y + ((((F(8.05374449538e-2) * z - F(1.38776856032e-1)) * z + F(1.99777106478e-1)) * z - F(3.33329491539e-1)) * z * x + x)
    return np.where(xx < F(0.0), -y, y).astype(F)


def atan2_(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    with np.errstate(all="ignore"):
        w = np.where(x < F(0.0), np.where(y < F(0.0), -_PI, _PI), F(0.0)).astype(F)
        r = w + atan_(y / x)
    r = np.where(y == F(0.0), np.where(x < F(0.0), _PI, F(0.0)), r)
    r = np.where(x == F(0.0), np.where(y > F(0.0), _PIO2, np.where(y < F(0.0), -_PIO2, F(0.0))), r)
    return r.astype(F)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def valid(l2):
    return (l2 > F(0.0)) & (l2 < _INF)


def normalize(v):
    with np.errstate(all="ignore"):
        return v * (F(1.0) / np.sqrt(dot(v, v)))[..., None]


# ---- the per-element functions of hr_mesh.h
def triangles(indices, mode=ffi.HR_TRIANGLES):
    """the triangle list as T x 3 vertex indices"""
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    if mode == ffi.HR_TRIANGLE_STRIP:
        T = max(idx.size - 2, 0)
        tri = np.stack([idx[0:T], idx[1:T + 1], idx[2:T + 2]], axis=-1) if T else np.zeros((0, 3), np.uint32)
        odd = (np.arange(T) & 1) == 1
        tri[odd, 0], tri[odd, 1] = tri[odd, 1].copy(), tri[odd, 0].copy()
        return tri
    T = idx.size // 3
    return idx[:3 * T].reshape(T, 3).copy()


def face_terms(p0, p1, p2, weight):
    """msFace: (face, e1, e2, u, w) of T triangles; u and w are 0 where a triangle is DEGENERATE"""
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        fn = cross(e1, e2)
        l2 = dot(fn, fn)
        face = valid(l2)
        ln = np.sqrt(l2)
        u = fn * (F(1.0) / ln)[:, None]
        if weight == ffi.HR_MESH_WEIGHT_ANGLE:
            w = np.stack([atan2_(ln, dot(e1, e2)), atan2_(ln, dot(p2 - p1, p0 - p1)), atan2_(ln, dot(p0 - p2, p1 - p2))], axis=-1)
        elif weight == ffi.HR_MESH_WEIGHT_AREA:
            w = np.repeat(ln[:, None], 3, axis=1)
        else:
            w = np.ones((len(ln), 3), F)
    u = np.where(face[:, None], u, F(0.0)).astype(F)
    w = np.where(face[:, None], w, F(0.0)).astype(F)
    return face, e1, e2, u, w


def face_tangents(e1, e2, uv0, uv1, uv2):
    """msFaceTangents of non-degenerate triangles: (ok, unit T, unit B); 0 where a triangle is DEGENERATE-UV"""
    with np.errstate(all="ignore"):
        d1, d2 = uv1 - uv0, uv2 - uv0
        det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
        T = e1 * d2[:, 1:2] - e2 * d1[:, 1:2]
        B = e2 * d1[:, 0:1] - e1 * d2[:, 0:1]
        neg = (det < F(0.0))[:, None]
        T, B = np.where(neg, -T, T), np.where(neg, -B, B)
        ok = (det != F(0.0)) & np.isfinite(det) & valid(dot(T, T)) & valid(dot(B, B))
        Tn, Bn = normalize(T), normalize(B)
    return ok, np.where(ok[:, None], Tn, F(0.0)).astype(F), np.where(ok[:, None], Bn, F(0.0)).astype(F)


def finish_normal(G, first, u_first):
    """msFinishNormal: (N, class) with class 0 normal, 1 cancelled, 2 unreferenced"""
    with np.errstate(all="ignore"):
        ok = valid(dot(G, G))
    none = first == NO_CORNER
    N = np.where(ok[:, None], normalize(G), np.where(none[:, None], F(0.0), u_first)).astype(F)
    return N, np.where(ok, 0, np.where(none, 2, 1))


def given_normal(n):
    """msGivenNormal: (have, N)"""
    with np.errstate(all="ignore"):
        have = valid(dot(n, n))
    return have, np.where(have[:, None], normalize(n), F(0.0)).astype(F)


def finish_tangent(have, N, Ta, Ba):
    """msFinishTangent: (tangent, bitangent, fallback)"""
    with np.errstate(all="ignore"):
        t = Ta - N * dot(N, Ta)[:, None]
        own = valid(dot(t, t))
        ax, ay, az = np.abs(N[:, 0]), np.abs(N[:, 1]), np.abs(N[:, 2])
        pick = np.where((ax <= ay) & (ax <= az), 0, np.where(ay <= az, 1, 2))
        a = np.eye(3, dtype=F)[pick]
        fb = normalize(a - N * dot(N, a)[:, None])
        tangent = np.where(own[:, None], normalize(t), fb).astype(F)
        c = cross(N, tangent)
        bitangent = np.where((dot(c, Ba) < F(0.0))[:, None], -c, c).astype(F)
    tangent = np.where(have[:, None], tangent, F(0.0)).astype(F)
    bitangent = np.where(have[:, None], bitangent, F(0.0)).astype(F)
    return tangent, bitangent, have & ~own


def _sum_lists(values, use, order, begin, counts):
    """out[d] = the values[order[begin[d] + r]], r = 0 .. counts[d] - 1, for which `use` holds, added to +0 one after the other: the
    r-th entry of every destination's list at once"""
    out = np.zeros((len(counts), 3), F)
    with np.errstate(all="ignore"):
        for r in range(int(counts.max()) if len(counts) else 0):
            d = np.nonzero(counts > r)[0]
            s = order[begin[d] + r]
            out[d] = out[d] + np.where(use[s][:, None], values[s], F(0.0))  # (x + 0 is x for every sum that can arise: none is -0)
    return out


def reference(positions, indices, uvs=None, normals=None, mode=ffi.HR_TRIANGLES, params=None):
    """-> (normals, tangents, bitangents, result): V x 3 float32 each (None for what params.want does not ask for) and the
    hr_mesh_result as a dict, as include/hrcore_mesh.h defines them."""
    p = params if params is not None else default_params()
    _check(p)
    want_n, want_t = bool(p.want & ffi.HR_MESH_WANT_NORMALS), bool(p.want & ffi.HR_MESH_WANT_TANGENTS)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V = pos.shape[0]
    if want_t and uvs is None:
        raise ValueError("tangents need uvs")
    if want_t and not want_n and normals is None:
        raise ValueError("tangents need normals")
    tri = triangles(indices, mode)
    T = tri.shape[0]
    if T and int(tri.max()) >= V:
        raise ValueError("index out of range")
    face, e1, e2, u, w = face_terms(pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]], p.weight)
    # the inverted index: every vertex's corners in ascending corner index
    cv = tri.reshape(-1).astype(np.int64)
    order = np.argsort(cv, kind="stable")
    valence = np.bincount(cv, minlength=V)
    begin = np.concatenate([[0], np.cumsum(valence)[:-1]]).astype(np.int64)
    cface = np.repeat(face, 3)
    res = dict.fromkeys(RESULT_KEYS, 0)
    res["triangles"], res["degenerate_triangles"], res["max_valence"] = T, int((~face).sum()), int(valence.max()) if T else 0
    N = None
    if want_n:
        with np.errstate(all="ignore"):
            contrib = (u[:, None, :] * w[:, :, None]).reshape(-1, 3)
        S = _sum_lists(contrib, cface, order, begin, valence)
        first = np.full(V, NO_CORNER, np.uint32)
        np.minimum.at(first, cv[cface], np.arange(3 * T, dtype=np.uint32)[cface])
        if p.weld:
            key = pos + F(0.0)
            vorder = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))  # stable: equal positions stay in ascending vertex index
            ks = key[vorder]
            head = np.ones(V, bool)
            head[1:] = (ks[1:] != ks[:-1]).any(axis=1)
            gid = np.cumsum(head) - 1
            group_of = np.empty(V, np.int64)
            group_of[vorder] = gid
            gbegin = np.nonzero(head)[0]
            gcount = np.diff(np.concatenate([gbegin, [V]]))
        else:
            vorder = group_of = gbegin = np.arange(V)
            gcount = np.ones(V, np.int64)
        Gs = _sum_lists(S, np.ones(V, bool), vorder, gbegin, gcount)
        gfirst = np.full(len(gcount), NO_CORNER, np.uint32)
        np.minimum.at(gfirst, group_of, first)
        u_first = u[np.where(gfirst == NO_CORNER, 0, gfirst // 3)] if T else np.zeros((len(gcount), 3), F)
        gN, gcls = finish_normal(Gs, gfirst, u_first)
        N, cls = gN[group_of], gcls[group_of]
        have = cls != 2
        res["weld_groups"], res["unreferenced_vertices"], res["cancelled_vertices"] = len(gcount), int((cls == 2).sum()), int((cls == 1).sum())
    tangent = bitangent = None
    if want_t:
        uv = np.ascontiguousarray(uvs, F).reshape(-1, 2)
        ok, Tn, Bn = face_tangents(e1, e2, uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]])
        ok = ok & face
        res["degenerate_uv_triangles"] = int((face & ~ok).sum())
        with np.errstate(all="ignore"):
            cT, cB = (Tn[:, None, :] * w[:, :, None]).reshape(-1, 3), (Bn[:, None, :] * w[:, :, None]).reshape(-1, 3)
        cuv = np.repeat(ok, 3)
        Ta, Ba = _sum_lists(cT, cuv, order, begin, valence), _sum_lists(cB, cuv, order, begin, valence)
        if want_n:
            Nt = N
        else:
            have, Nt = given_normal(np.ascontiguousarray(normals, F).reshape(-1, 3))
        tangent, bitangent, fallback = finish_tangent(have, Nt, Ta, Ba)
        res["fallback_tangents"] = int(fallback.sum())
    return N, tangent, bitangent, res
