"""Ray queries of include/hrcore_query.h restated in numpy float32, operation for operation: `reference_screen` says which rays are
traced, `reference_surface` gives the bytes of the surface records k_query_trace writes (heatray_amd/csrc/hr_query.h) from the hits, and
`camera_rays` the rays hr_query_pixels makes.  They are the checkers of the GPU tests and work without a GPU.  Two conveniences on top of
an engine: `pick` and `autofocus`.

    hits, surf = eng.query(origins, dirs, surface=True)                                         # on the device
    surf.tobytes() == query.reference_surface(scene.meshes, geom_ids, hits, origins, dirs).tobytes()

Every product and sum below is one float32 operation on float32 arrays, parenthesised as the header writes it: numpy neither fuses nor
reorders them (see deform.py, meshprep.py).
"""
import numpy as np

from . import _ffi as ffi
from .deform import direction, point
from .meshprep import F, cross, dot, normalize, triangles, valid

_INF = F(np.inf)


def reference_screen(origins, dirs, tmax=None):
    """The invalid mask: a ray whose origin or direction has a component that is not finite, whose direction is 0 0 0, or whose tmax is
    NaN or -inf (+inf is "no limit") is not traced."""
    o, d = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        finite = (np.abs(o) < _INF).all(axis=1) & (np.abs(d) < _INF).all(axis=1)  # (a NaN compares false)
        zero = (d == F(0.0)).all(axis=1)
        ok = finite & ~zero
        if tmax is not None:
            ok &= np.ascontiguousarray(tmax, F).reshape(-1) > -_INF
    return ~ok


def camera_rays(pass_params, W, H, xy):
    """The rays hr_query_pixels makes for the points xy (n x 2, pixel units) of a W x H frame -> n x 6 float32 (o, d).  Reads fov_tan,
    aspect_ratio, focus_distance and view_matrix of `pass_params` (an ffi.PassParams)."""
    p = np.ascontiguousarray(xy, F).reshape(-1, 2)
    n = len(p)
    M = np.tile(np.array(pass_params.view_matrix[:], F).reshape(4, 4).T[None], (n, 1, 1))  # (the ABI is column-major; numpy holds m[row][col])
    fov, aspect, focus = F(pass_params.fov_tan), F(pass_params.aspect_ratio), F(pass_params.focus_distance)
    with np.errstate(all="ignore"):
        u, v = p[:, 0] / F(W), p[:, 1] / F(H)
        cx = ((F(2.0) * u - F(1.0)) * aspect) * fov
        cy = ((F(1.0) - F(2.0) * v) * fov) * F(-1.0)
        c = normalize(np.stack([cx, cy, np.full(n, -1.0, F)], axis=-1).astype(F))
        o = point(M, np.zeros((n, 3), F))
        d = normalize(direction(M, (focus * c).astype(F)))
    return np.concatenate([o, d], axis=1).astype(F)


def _unit_or_zero(x):
    with np.errstate(all="ignore"):
        ok = valid(dot(x, x))
        return np.where(ok[:, None], normalize(x), F(0.0)).astype(F)


def reference_surface(scene_meshes, geom_ids, hits, origins, dirs):
    """The surface records of closest hits.  scene_meshes: the committed meshes in the order they were added (objects with positions,
    normals, indices, uvs, mode, world, material_id, is_occluder and optionally front_face_cw, like scenes.MeshData; meshes without a
    triangle are skipped as the commit skips them), geom_ids: their hr_geom_ids; hits: what the query returned (prim < 0: a miss
    record); origins, dirs: the rays.  -> SURFACE_DTYPE array, byte for byte what the device writes."""
    o, d = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = len(hits)
    out = np.zeros(n, dtype=ffi.SURFACE_DTYPE)
    out["geom"] = -1
    first = 0
    for mesh, gid in zip(scene_meshes, geom_ids):
        tri = triangles(mesh.indices, mesh.mode)
        T = len(tri)
        if T == 0:
            continue
        sel = np.nonzero((hits["prim"] >= first) & (hits["prim"] < first + T))[0]
        lt = hits["prim"][sel] - first
        first += T
        if sel.size == 0:
            continue
        m = np.eye(4, dtype=F) if mesh.world is None else np.ascontiguousarray(mesh.world, F).reshape(4, 4)
        cw = getattr(mesh, "front_face_cw", None)
        cw = bool(np.linalg.det(m.astype(np.float64)) < 0) if cw is None else bool(cw)
        M = np.tile(m[None], (sel.size, 1, 1))
        ids = tri[lt]
        pos, nrm = np.ascontiguousarray(mesh.positions, F).reshape(-1, 3), np.ascontiguousarray(mesh.normals, F).reshape(-1, 3)
        ro, rd = o[sel], d[sel]
        t, u, v = hits["t"][sel], hits["u"][sel], hits["v"][sel]
        with np.errstate(all="ignore"):
            w = (F(1.0) - u) - v
            position = ro + rd * t[:, None]
            n0, n1, n2 = (direction(M, nrm[ids[:, k]]) for k in range(3))
            N = (n0 * w[:, None] + n1 * u[:, None]) + n2 * v[:, None]
            p0, p1, p2 = (point(M, pos[ids[:, k]]) for k in range(3))
            e1, e2 = p1 - p0, p2 - p0
            G = cross(e1, e2)
            # the winding the ray saw: the sign of the hit test's determinant dot(e1, cross(d, e2))
            ccw = dot(e1, cross(rd, e2)) > F(0.0)
        rec = out[sel]
        rec["geom"], rec["material"], rec["prim_in_geom"] = gid, mesh.material_id, lt
        rec["position"], rec["normal"], rec["geometric_normal"] = position, _unit_or_zero(N.astype(F)), _unit_or_zero(G.astype(F))
        flags = np.where(ccw != cw, ffi.HR_QUERY_SF_FRONT, 0).astype(np.uint32)
        if mesh.uvs is not None:
            uv = np.ascontiguousarray(mesh.uvs, F).reshape(-1, 2)
            with np.errstate(all="ignore"):
                rec["uv"] = (uv[ids[:, 0]] * w[:, None] + uv[ids[:, 1]] * u[:, None]) + uv[ids[:, 2]] * v[:, None]
            flags |= np.uint32(ffi.HR_QUERY_SF_HAS_UV)
        if not mesh.is_occluder:
            flags |= np.uint32(ffi.HR_QUERY_SF_NON_OCCLUDER)
        rec["flags"] = flags
        out[sel] = rec
    return out


def _pixel(engine, options, x, y, surface):
    xy = np.array([[x, y]], F)
    return engine.query_pixels(options.pass_params(0), xy, surface=surface)


def pick(engine, options, x, y):
    """What the point (x, y) of the frame shows (pixel units, row 0 at the bottom; options: a host.RenderOptions):
    {"geom", "prim_in_geom", "material", "position", "normal", "geometric_normal", "uv", "flags", "prim", "t"}, or None for a miss."""
    hits, surf = _pixel(engine, options, x, y, True)
    if hits["prim"][0] < 0:
        return None
    s = surf[0]
    out = {k: (s[k].copy() if s[k].ndim else s[k].item()) for k in ("geom", "prim_in_geom", "material", "position", "normal", "geometric_normal", "uv", "flags")}
    out["prim"], out["t"] = int(hits["prim"][0]), float(hits["t"][0])
    return out


def autofocus(engine, options, x, y):
    """The focus_distance that focuses the lens on what the point (x, y) of the frame shows, or None for a miss."""
    hits = _pixel(engine, options, x, y, False)
    return float(hits["t"][0]) if hits["prim"][0] >= 0 else None
