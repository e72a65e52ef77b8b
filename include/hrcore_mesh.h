/*
 * hrcore_mesh.h — mesh preparation on the device: smooth vertex normals and tangent frames for a mesh that comes without them.
 *
 * hr_geom_add refuses a mesh without normals, and a normal-mapped material reads per-vertex tangents and bitangents.  A loader built on
 * Assimp gets all three from its post-process steps (GenSmoothNormals, CalcTangentSpace, JoinIdenticalVertices); a caller that holds
 * positions and indices only (an STL, an OBJ without vn, a height field, a simulation's surface) gets them here:
 *
 *     hr_mesh_params p;  hr_mesh_default_params(&p);  p.want = HR_MESH_WANT_NORMALS | HR_MESH_WANT_TANGENTS;
 *     hr_mesh_prepare(ctx, &desc, &p, normals, tangents, bitangents, &r);      desc: positions, uvs, indices
 *     desc.normals = normals;  desc.tangents = tangents;  desc.bitangents = bitangents;
 *     hr_geom_add(ctx, &desc, &id);
 *
 * A pure side call: it builds no scene state (no geometry is added, nothing is marked for a commit), reads no frame and may be made at
 * any time, between passes included.  A context group is served (the call runs on its first member), and so is a tile-sharded context.
 * Without a call every bit of every frame, plane and counter is what it is in a library without this header.
 *
 * WHAT IS READ FROM desc: positions, indices, n_vertices, n_indices, mode and the strides exactly as hr_geom_add reads them (0 = tightly
 * packed; strides that are no multiple of four and interleaved buffers included); uvs when tangents are wanted; normals when tangents
 * are wanted and normals are not (the tangents are then built against the caller's normals).  world_from_entity is ignored: everything
 * is in object space, and the scene's assembly transforms later.  The other fields are not read.
 *
 * ARITHMETIC: the project's contract — one binary32 operation per written operation, in the order written, no contraction; sqrt_, abs_,
 * atan2_, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z and cross of hr_math.h; normalize(v) = v * (1.0f / sqrt_(dot(v, v)));
 * "valid(l2)" means l2 > 0 and l2 < +inf.  The per-element functions are heatray_amd/csrc/hr_mesh.h; heatray_amd/meshprep.py restates
 * them in numpy float32, bit for bit.  No float atomics anywhere: every sum below has ONE order, so a result is the same bits on every
 * run, context and device.
 *
 * TRIANGLES: the list hr_scene_commit makes of the same desc.  HR_TRIANGLES: triangle t is indices 3t, 3t + 1, 3t + 2 (n_indices / 3
 * triangles, trailing indices ignored).  HR_TRIANGLE_STRIP: triangle t is indices t, t + 1, t + 2, the first two swapped for odd t
 * (n_indices - 2 triangles, none below 3 indices).  Corner c = 3t + k is the triangle's k-th vertex p_k.
 *
 * FACE TERMS.  e1 = p1 - p0, e2 = p2 - p0, fn = cross(e1, e2), l2 = dot(fn, fn).  l2 not valid: the triangle is DEGENERATE, contributes
 * nothing and is counted.  len = sqrt_(l2), u = fn * (1.0f / len).  Corner weight w_k by hr_mesh_params::weight:
 *     ANGLE    atan2_(len, dot(a_k, b_k)), a_k and b_k the two edges leaving corner k: (e1, e2), (p2 - p1, p0 - p1), (p0 - p2, p1 - p2)
 *     AREA     len
 *     UNIFORM  1
 * The normal contribution of corner k is u * w_k.
 *
 * PER-VERTEX SUM.  S(v) = the contributions of v's corners in ascending corner index, added component-wise to +0 one after the other.
 *
 * WELD (weld = 1).  Vertices whose positions compare equal as floats (-0 == +0) form a group.  G = the sum of S(v) over the group's
 * members in ascending vertex index, added to +0 one after the other; every member uses G.  weld = 0: every vertex is its own group.
 * (The two-level order is the contract: one sort of the corners serves normals and tangents.)
 *
 * NORMAL.  dot(G, G) valid: normalize(G).  Otherwise a vertex whose group has no non-degenerate corner gets 0 0 0 and is counted
 * UNREFERENCED; any other gets the u of the lowest-index non-degenerate corner of its group and is counted CANCELLED (a fin whose two
 * faces cancel).
 *
 * TANGENTS, per vertex index and never welded (UV seams and mirrors must split them).  Per non-degenerate triangle:
 *     d1 = uv1 - uv0, d2 = uv2 - uv0, det = d1.x * d2.y - d2.x * d1.y
 *     T = e1 * d2.y - e2 * d1.y,  B = e2 * d1.x - e1 * d2.x,  both negated when det < 0
 * det zero or not finite, or dot(T, T) or dot(B, B) not valid: the triangle is DEGENERATE-UV, counted, and contributes no tangent terms.
 * Contributions: normalize(T) * w_k and normalize(B) * w_k; Ta(v) and Ba(v) are summed like S(v).  Finish, with N = the output normal,
 * or, when normals are not wanted, normalize(desc->normals[v]) if its dot with itself is valid, else 0 0 0:
 *     N = 0 0 0: tangent = bitangent = 0 0 0
 *     t = Ta - N * dot(N, Ta);  dot(t, t) valid: tangent = normalize(t)
 *     else the FALLBACK, counted: a = the unit axis of N's smallest abs_ component (ties: x, then y), tangent = normalize(a - N * dot(N, a))
 *     c = cross(N, tangent);  bitangent = dot(c, Ba) < 0 ? -c : c
 *
 * LIMITS.
 *   - Welding is exact: a seam whose two sides differ in the last bit is not welded (a lat/long sphere whose u = 0 and u = 1 columns
 *     come from cos(0) and cos(float(2 pi)) is such a seam).  There is no tolerance parameter.
 *   - No crease angle: hard edges need the caller's duplicated vertices and weld = 0.
 *   - One thread walks a vertex's corner list, and one a group's members, sequentially: a fan of many thousand triangles around one
 *     vertex, or many thousand coincident vertices, is slow but correct.
 *   - At most 2^32 - 1 corners (a strip of more than 1,431,655,767 indices is refused).
 *
 * MEMORY.  Scratch on the context's device sized by corners and vertices (about 52 bytes per corner and 135 per vertex with tangents
 * and weld; the four sort arrays among them hold max(corners, vertices) words each), kept on the context and grown only, freed by hr_ctx_destroy; not counted against hr_ctx_desc::memory_budget.  The
 * uploads go through the staging ring hr_geom_add uses.
 *
 * Not part of hrcore.h or any other header: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_MESH_H
#define HRCORE_MESH_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_MESH_API_VERSION 1u
uint32_t hr_mesh_api_version(void);

#define HR_MESH_WEIGHT_ANGLE 0
#define HR_MESH_WEIGHT_AREA 1
#define HR_MESH_WEIGHT_UNIFORM 2

#define HR_MESH_WANT_NORMALS 1
#define HR_MESH_WANT_TANGENTS 2

typedef struct hr_mesh_params {
    int32_t weight;      /* HR_MESH_WEIGHT_* */
    int32_t weld;        /* 0 / 1 */
    int32_t want;        /* HR_MESH_WANT_NORMALS | HR_MESH_WANT_TANGENTS, not 0 */
    int32_t reserved[5]; /* 0 */
} hr_mesh_params;

typedef struct hr_mesh_result {
    uint64_t triangles;               /* of the triangle list */
    uint64_t degenerate_triangles;
    uint64_t degenerate_uv_triangles; /* non-degenerate ones whose UVs give no tangent; 0 when tangents are not wanted */
    uint64_t weld_groups;             /* groups of vertices; n_vertices with weld = 0; 0 when normals are not wanted */
    uint64_t unreferenced_vertices;   /* 0 when normals are not wanted */
    uint64_t cancelled_vertices;      /* 0 when normals are not wanted */
    uint64_t fallback_tangents;       /* vertices whose tangent is the fallback */
    uint64_t max_valence;             /* the longest corner list of a vertex (degenerate triangles' corners included) */
} hr_mesh_result;

/* weight ANGLE, weld 1, want NORMALS; NULL is ignored */
void hr_mesh_default_params(hr_mesh_params *p);
/* desc -> normals_out, tangents_out, bitangents_out: the caller's host arrays, tightly packed, 3 floats per vertex; one that `want` does
 * not ask for may be NULL.  Synchronous.  params == NULL: the defaults; out may be NULL.  HR_ERR_INVALID (hr_last_error names the cause;
 * the context stays usable): NULL ctx, desc, positions, indices or a wanted output; n_vertices <= 0 or n_indices < 0; unknown mode,
 * weight or want, want == 0, weld not 0 or 1, non-zero reserved; an index >= n_vertices; a stride smaller than its attribute;
 * positions that are not finite (hr_geom_add's rule); tangents wanted without uvs; tangents wanted without normals and without
 * desc->normals; more than 2^32 - 1 corners. */
int hr_mesh_prepare(hr_ctx *ctx, const hr_mesh_desc *desc, const hr_mesh_params *params, float *normals_out, float *tangents_out, float *bitangents_out,
                    hr_mesh_result *out);
/* the result of the context's last successful hr_mesh_prepare (HR_ERR_INVALID before the first) */
int hr_mesh_last(hr_ctx *ctx, hr_mesh_result *out);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_MESH_H */
