/*
 * hrcore_query.h — ray queries: the caller's rays traced against the committed scene on the device, answered with the render's own hit
 * and, on request, a record of the surface that was hit.
 *
 * The tree, the triangles and the per-triangle attributes are resident after hr_scene_commit.  hr_debug_trace (hrcore.h) traces a
 * caller's rays against them for the parity tests: host arrays only, five allocations per call, a global triangle index nobody can map
 * back to a mesh.  Here:
 *
 *     hr_query_trace(ctx, &desc, stream);        rays and answers in DEVICE memory, asynchronous, on the caller's stream
 *     hr_query_trace_host(ctx, &desc);           the same desc with HOST arrays, synchronous
 *     hr_query_pixels(ctx, &camera, n, xy, hits, surfaces, rays);     the rays through points of the frame, made on the device
 *     hr_query_last(ctx, &result);               how many rays, hits and invalid rays the last call saw
 *
 * What they are for: picking (which mesh, which triangle of it, where on it), focusing the lens on what a pixel shows, visibility between
 * two points, and tracing a tensor of rays without a trip through the host.
 *
 * THE HIT is the render's: the triangle test of DESIGN.md §4 (Möller–Trumbore and the hit point inside the triangle's half-padded box),
 * the (t, prim) lexicographic minimum over t in (tmin, tmax).  It does not depend on the tree.  hits[i] = {prim, t, u, v} with the global
 * triangle index in submission order, exactly what hr_debug_trace reports for the same ray; -1 = miss (then t = u = v = 0).  Directions
 * are NOT normalised by the call: t is in units of |d|.  tmin < 0 means the scene's ray_epsilon (hr_scene_info), which is what the render
 * and hr_debug_trace use; tmin = 0 is allowed.  skip_prim[i] >= 0 excludes that triangle (a ray leaving a surface).  tmax <= tmin is an
 * ordinary miss.
 *
 * With HR_QUERY_ANY_HIT the query is an OCCLUSION query, answered by the first hit found: hits[i].prim = 0 blocked / -1 clear,
 * t = u = v = 0.  It sees the scene as a shadow ray of the render does: a non-occluder mesh whose PBR material is alpha-masked lets the
 * ray pass where the base colour texture's alpha is below 1 (physicallyBased.rlsl:57-91); every other primitive blocks.  A closest-hit
 * query reports such primitives like any other and flags them HR_QUERY_SF_NON_OCCLUDER.
 *
 * WHICH RAYS ARE TRACED.  A ray is INVALID if a component of its origin or of its direction is not finite, if its direction is 0 0 0, or
 * if its tmax (where tmax is given) is NaN or -inf; a tmax of +inf is the default "no limit".  An invalid ray is not traced: its
 * hits[i] is {HR_QUERY_INVALID_RAY, 0, 0, 0}, its surface record a miss (geom = -1), and it is counted in hr_query_result::invalid.  The
 * screen runs before the traversal starts, so the answer to every input is defined.
 *
 * THE SURFACE RECORD (closest-hit queries only).  ARITHMETIC: the project's contract — one binary32 operation per written operation, in
 * the order written, no contraction; dot, cross, normalize and valid as include/hrcore_mesh.h defines them.  i0 i1 i2: the triangle's
 * vertex indices (TRIANGLES: idx[3 lt .. 3 lt + 2]; TRIANGLE_STRIP: idx[lt], idx[lt + 1], idx[lt + 2] with the first two swapped for odd
 * lt); W: the mesh's world_from_entity; point(M, p).x = ((M[0]*p.x + M[4]*p.y) + M[8]*p.z) + M[12], dir(M, d).x = (M[0]*d.x + M[4]*d.y)
 * + M[8]*d.z (.y: 1 5 9 13, .z: 2 6 10 14); o, d, t, u, v: the ray and its hit.
 *
 *     w = (1 - u) - v
 *     position          = o + d * t                                  (component-wise: the product rounded, then the sum)
 *     n_k               = dir(W, normals[i_k]);   N = (n_0 * w + n_1 * u) + n_2 * v;   normal = valid(dot(N,N)) ? normalize(N) : 0 0 0
 *     p_k               = point(W, positions[i_k]);   e1 = p_1 - p_0;   e2 = p_2 - p_0;   G = cross(e1, e2)
 *     geometric_normal  = valid(dot(G,G)) ? normalize(G) : 0 0 0
 *     uv                = (uv_0 * w + uv_1 * u) + uv_2 * v            (0 0 and HR_QUERY_SF_HAS_UV clear for a mesh without uvs)
 *     FRONT             = the ray saw the triangle counter-clockwise (the hit test's determinant dot(e1, cross(d, e2)) > 0), inverted
 *                         for a front_face_cw mesh: rl_FrontFacing as the shaders see it
 *
 * geom is the hr_geom_id hr_geom_add returned (an id, not a position: it survives the removal of other meshes), prim_in_geom the
 * triangle's index lt within that mesh, material the mesh's material_id.  A miss and an invalid ray: geom = -1, every other byte 0.
 * heatray_amd/csrc/hr_query.h holds these lines; heatray_amd/query.py restates them in numpy float32, bit for bit.
 *
 * PIXEL QUERIES.  hr_query_pixels makes, for each (px, py) in pixel units (the centre of pixel x, y is x + 0.5, y + 0.5; row 0 is the
 * bottom row), the ray through that point of the image plane from the centre of the lens: the frame shader's camera ray
 * (perspective.rlsl:39-93) with the jitter and the aperture sample taken out.  Width and Height are the frame's (hr_frame_resize).
 *
 *     u = px / Width;  v = py / Height;  cx = ((2 * u - 1) * aspect_ratio) * fov_tan;  cy = ((1 - 2 * v) * fov_tan) * -1
 *     c = normalize(cx, cy, -1);   o = point(view_matrix, 0 0 0);   d = normalize(dir(view_matrix, focus_distance * c))
 *
 * Only fov_tan, aspect_ratio, focus_distance and view_matrix of `camera` are read.  The rays are made on the device, traced with tmin = 0
 * and no tmax, and resolved into hits and surface records as above; rays_out returns them (o then d, 6 floats per ray).  Because d is
 * unit length and o the centre of the lens, hits[i].t IS the value to write into hr_pass_params::focus_distance to focus the lens on what
 * that pixel shows.  A camera that is not finite makes invalid rays, answered as above.
 *
 * ORDERING.  hr_query_trace enqueues on `stream` (NULL: the context's stream) and returns; its inputs are read and its outputs written
 * when the stream gets there.  It runs behind the last hr_scene_commit (through an event where the streams differ), and the context's
 * next hr_scene_commit — and every other call that rewrites or frees what a query reads: materials, textures, lights, hr_ctx_destroy —
 * waits for the queries in flight (compare hr_aov_copy: "the ctx's next resolve waits for it").  The queries of one context run one
 * after the other in call order, whatever their streams.  Queries read only what a commit (and the scene block's upload) writes: they
 * neither wait for nor disturb passes in flight, and never change the frame, an AOV plane or a counter of hr_get_stats.  The one
 * exception is the first query after a commit or a change of materials, textures or lights: like the first pass, it uploads the scene
 * block, which completes the passes in flight.  hr_query_trace_host and hr_query_pixels return with their outputs filled.
 *
 * hr_query_last completes the queries in flight and returns the counters of the last successful call: rays = its n, hits = rays with
 * prim >= 0 (an occlusion query: blocked rays), invalid as above.
 *
 * DEVICE POINTERS (hr_query_trace).  Every pointer of the desc is device memory reachable from the context's device; hits and surfaces
 * must be 16-byte aligned (they are written with 16-byte stores), the inputs 4-byte aligned.  Strides are in bytes; 0 = tightly packed
 * (12, 12, 4, 4); otherwise a multiple of 4 that is at least the element.  Inputs and outputs must not overlap.
 *
 * MEMORY.  hr_query_trace allocates nothing per call.  hr_query_trace_host and hr_query_pixels stage rays and answers through one block
 * of scratch owned by the context, sized by the largest call so far and grown only; it is freed by hr_ctx_destroy and is not counted
 * against hr_ctx_desc::memory_budget.  A table of 8 bytes per mesh (first triangle, id) and 8 KB of counters go with it.
 *
 * LIMITS.  Rays are traced in the order given, one per lane, without sorting: neighbouring rays that walk different parts of the tree
 * (an incoherent batch) pay for it; DESIGN.md gives the measured cost.  One ray per call costs a launch.
 *
 * GROUPS AND SHARDS.  Every member of a context group holds the whole scene, so member 0 serves the call; for hr_query_trace the
 * device pointers must be reachable from member 0's device and `stream` must be a stream of that device.  hr_query_pixels takes Width
 * and Height from the group's frame.  A tile-sharded context is served (queries do not touch the frame).
 *
 * An uncommitted scene is HR_ERR_INVALID "scene not committed".  A committed scene without triangles answers every valid ray with a miss.
 *
 * Not part of hrcore.h or any other header: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_QUERY_H
#define HRCORE_QUERY_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_QUERY_API_VERSION 1u
uint32_t hr_query_api_version(void);

#define HR_QUERY_ANY_HIT 1u       /* occlusion query: hits[i].prim = 0 blocked / -1 clear, t = u = v = 0; surfaces must be NULL */
#define HR_QUERY_INVALID_RAY (-2) /* hits[i].prim of a ray that was not traced (above) */

#define HR_QUERY_SF_FRONT 1u /* rl_FrontFacing as the shaders see it */
#define HR_QUERY_SF_HAS_UV 2u
#define HR_QUERY_SF_NON_OCCLUDER 4u

typedef struct hr_query_surface { /* 64 bytes */
    int32_t geom;         /* hr_geom_id of the mesh, -1: miss or invalid ray (then every other field is 0) */
    int32_t material;     /* the mesh's material_id */
    int32_t prim_in_geom; /* triangle index within that mesh (strip: the lt-th triangle of the strip) */
    uint32_t flags;       /* HR_QUERY_SF_* */
    float position[3];
    float normal[3];           /* interpolated vertex normal, unit length or 0 0 0 */
    float geometric_normal[3]; /* of the world-space triangle as wound, unit length or 0 0 0 */
    float uv[2];
    float reserved; /* 0 */
} hr_query_surface;

typedef struct hr_query_desc {
    int32_t n;                /* rays; 0 is HR_OK and does nothing; < 0: HR_ERR_INVALID */
    uint32_t flags;           /* HR_QUERY_ANY_HIT; unknown bits: HR_ERR_INVALID */
    const float *origins;     /* 3 floats per ray, required */
    const float *directions;  /* 3 floats per ray, required; NOT normalised by the call: t is in units of |d| */
    const float *tmax;        /* NULL: +inf */
    const int32_t *skip_prim; /* NULL or a negative entry: none (global prim index, as hr_hit.prim reports it) */
    int32_t origin_stride, direction_stride, tmax_stride, skip_stride; /* bytes; 0 = tightly packed; else a multiple of 4 >= the element */
    float tmin;           /* a hit has t in (tmin, tmax); negative: the scene's ray_epsilon (what the render and hr_debug_trace use) */
    uint32_t reserved[3]; /* 0 */
    hr_hit *hits;               /* n records, or NULL */
    hr_query_surface *surfaces; /* n records, or NULL; at least one of the two outputs must be given */
} hr_query_desc;

typedef struct hr_query_result {
    uint64_t rays, hits, invalid;
    uint64_t reserved[5];
} hr_query_result;

/* Every pointer in desc is DEVICE memory; asynchronous on `stream` (a hipStream_t; NULL: the context's).  HR_ERR_INVALID (hr_last_error
 * names the cause; nothing is launched): "null desc"; "n = -1 is negative"; "unknown flags 2"; "reserved[0] must be 0"; "null origins";
 * "null directions"; "no output: hits and surfaces are both null"; "surfaces with HR_QUERY_ANY_HIT"; a stride that is no multiple of 4 or
 * smaller than its element ("origin_stride = 10 ..."); "tmin is NaN"; "hits must be 16-byte aligned" (surfaces likewise); "scene not
 * committed".  n = 0 is HR_OK after these checks and touches nothing. */
int hr_query_trace(hr_ctx *ctx, const hr_query_desc *desc, void *stream);
/* The same desc with every pointer in HOST memory (no alignment rule beyond the types'); synchronous. */
int hr_query_trace_host(hr_ctx *ctx, const hr_query_desc *desc);
/* n points of the frame -> camera rays, traced with tmin = 0 (PIXEL QUERIES above).  pixels_xy: host, 2 floats per ray; hits, surfaces,
 * rays_out (6 floats per ray: o, d): host, each may be NULL but not all three.  HR_ERR_INVALID: "null camera"; "n = -1 is negative";
 * "null pixels"; "no output"; "no frame" (before hr_frame_resize); "scene not committed". */
int hr_query_pixels(hr_ctx *ctx, const hr_pass_params *camera, int32_t n, const float *pixels_xy, hr_hit *hits, hr_query_surface *surfaces,
                    float *rays_out);
/* Completes the queries in flight; the last successful call's counters (HR_ERR_INVALID before the first, or "null output"). */
int hr_query_last(hr_ctx *ctx, hr_query_result *out);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_QUERY_H */
