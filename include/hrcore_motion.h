/*
 * hrcore_motion.h — motion reprojection: keep what a frame knew when meshes move or deform.
 *
 * hrcore_history.h carries a frame's mean, second moment and sample count across a CAMERA change: it finds the place to gather from
 * with the new view's depth plane, which is right only while the geometry stands still.  Here the place comes from the geometry itself.
 * A snapshot remembers the committed pose's world-space triangles; after the scene was edited and committed again, one pixel-centre
 * ray per pixel finds the surface point the pixel shows (the render's own hit: mesh, triangle within the mesh, barycentrics), the same
 * material point is interpolated over the snapshot's triangle, and the history is gathered where THAT point was seen.
 *
 *     ... render the frame ...
 *     hr_history_capture(ctx, &old_camera);          the history itself stays hrcore_history.h's: H0, H1, H2
 *     hr_motion_snapshot(ctx);                       remember the committed pose
 *     hr_geom_update / hr_deform_pose / hr_geom_set_transform / hr_geom_add / hr_geom_remove / another camera, in any mix
 *     hr_scene_commit(ctx);  hr_clear(ctx);
 *     hr_render_pass(ctx, &new_camera) ...           at least one pass
 *     hr_motion_merge(ctx, &new_camera, 0, &r);      hr_history_merge, gathering at the place the snapshot gives; once per hr_clear
 *     hr_motion_vectors(ctx, 0, device_out, 0);      the screen-space motion of every pixel, for an external temporal filter
 *
 * Opt-in, on the context's stream; it touches no kernel of the pass pipeline: without a call to it every bit of every frame, plane,
 * digest and counter is what it is in a library without this header.
 *
 * THE SNAPSHOT.  hr_motion_snapshot reads the committed scene: for every triangle, in submission (prim) order, the world-space
 * (p0, e1, e2) the commit stored (e1 = p1 - p0, e2 = p2 - p0, p_k = point(world_from_entity, positions[i_k]) as include/hrcore_query.h
 * writes them), padded to three float4 (48 bytes per triangle); and, on the host, (hr_geom_id, first triangle, triangle count) of every
 * committed mesh.  It survives hr_clear, later commits and hr_frame_resize; it goes with hr_motion_drop, a second snapshot and
 * hr_ctx_destroy; it is not counted against hr_ctx_desc::memory_budget.  It is enqueued on the context's stream behind the commit it
 * reads, and the context's next commit waits for it as it waits for queries in flight.
 *
 * ARITHMETIC.  The project's contract: one binary32 operation per written operation, in the order written (parentheses first, otherwise
 * left to right), no contraction; dot, cross, normalize and valid as include/hrcore_mesh.h defines them, dir as include/hrcore_query.h,
 * ray(x, y; aspect, fov), the two cameras (R, ax_old) and abs_ / floor_ / fmin_ as include/hrcore_history.h.  V = the new camera's
 * view_matrix, n_k = col_k(V), o = eye(V); V_old, o_k = col_k(V_old) likewise.  heatray_amd/csrc/hr_motion.h holds these lines;
 * heatray_amd/motion.py restates them in numpy float32, bit for bit.
 *
 * THE MOTION PLANES.  hr_motion_trace writes two planes of W x H float4, Mv0 and Mv1, per pixel (x, y), whether it has a sample or not:
 *
 *     c = ray(x, y; aspect_new, fov_new);   d = normalize(dir(V, c))
 *     hit = the render's closest hit of (o, d), tmin = 0, no tmax       (include/hrcore_query.h, THE HIT)
 *     miss:                     Mv0 = 0 0 0 0;             Mv1 = (0, 0, 0, +inf)
 *     hit (prim, t, u, v):      Pw = o + d * t;   depth = -dot(n_2, Pw - o)
 *       m = the mesh of prim, lt = prim - first(m)
 *       the snapshot holds a mesh with the hr_geom_id of m and the same triangle count -> (p0', e1', e2') of its lt-th triangle:
 *           Q  = (p0' + e1' * u) + e2' * v                               the same material point, previous pose, world space
 *           G  = cross(e1', e2');   Ng = valid(dot(G, G)) ? normalize(G) : 0 0 0
 *           Mv0 = (Q, 1);   Mv1 = (Ng, depth)
 *       otherwise (a mesh added since, or added again with another size): Mv0 = (Pw, -1);   Mv1 = (0, 0, 0, depth)
 *
 * The result counts surface (Mv0.w == 1), sky (0) and unmatched (-1) pixels.  The planes are allocated by the first trace and go with
 * the frame's size (hr_frame_resize) and hr_motion_drop.
 *
 * THE MERGE.  hr_motion_merge runs the trace for `camera`, then, per pixel with n = F.a > 0 (F, A, G, M: the frame and the planes
 * ALBEDO, NORMAL_DEPTH, MOMENTS as in include/hrcore_history.h), cov = A.a / n:
 *
 *     Mv0.w == 1 and cov >= 0.5:
 *         dmean = G.w / A.a;   not abs_(Mv1.w - dmean) <= plane_tol * dmean -> no history
 *                               (the centre ray and the pixel's samples disagree: a silhouette, a thin lens, a pass-through face)
 *         r = Q - eye(V_old);   q[i] = dot(o_i, r);   Nq[i] = dot(o_i, Ng)
 *         then exactly as hr_history_merge from "z = -q.z": the projection, the four taps, their weights, the sums, nh and the
 *         updates of F, M, A, G — except that a tap counts when  abs_(dot(Ng, H2(T).xyz)) >= normal_cos  in place of the normal
 *         test (the previous pose's geometric normal against the history's shading normal, either winding), and the plane test
 *         uses this Nq
 *     Mv0.w == 0 and cov < 0.5:   the sky branch of hr_history_merge, unchanged (q = rc)
 *     otherwise:                   no history
 *
 * The parameters are hr_history_params; hr_motion_default_params gives normal_cos = 0.8 and otherwise the history's defaults (a
 * geometric and an interpolated normal differ on a curved mesh).  One merge per hr_clear, of whatever kind: hr_motion_merge is refused
 * after hr_history_merge or hr_reproject_merge, and they are refused after it.
 *
 * MOTION VECTORS.  hr_motion_vectors writes one float4 per pixel from the planes of the last trace (or merge):
 *
 *     Mv0.w == 1:  r = Q - eye(V_old);  q[i] = dot(o_i, r)         Mv0.w == 0:  q = rc, the sky pixel's direction in the old camera
 *     z = -q.z;   sx, sy as the merge projects them
 *     out = (sx - (x + 0.5), sy - (y + 0.5), z, Mv0.w);   Mv0.w == -1 or not z > 0:  out = (0, 0, 0, Mv0.w)
 *
 * so (x + 0.5, y + 0.5) + out.xy is where the pixel's surface point was in the old camera's image, in pixels.
 *
 * LIMITS.
 *   - A pinhole at the lens centre: a thin-lens render is reprojected through the centre ray.
 *   - First surface only: what is seen behind glass or in a mirror moves with the glass or the mirror.
 *   - View-dependent shading is taken over as if it were diffuse.
 *   - Lighting that changed because the mover's shadow moved is taken over too; the bias is bounded by max_history.
 *   - Material and light edits still need hr_history_drop.
 *   - No progressive form: hr_reproject_* gathers with the depth plane only.
 *   - Context groups and tile-sharded contexts are refused, as hrcore_history.h refuses them.
 *
 * Not part of hrcore.h or any other header: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_MOTION_H
#define HRCORE_MOTION_H

#include "hrcore_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_MOTION_API_VERSION 1u
uint32_t hr_motion_api_version(void);

typedef struct hr_motion_trace_result {
    uint64_t surface_pixels;   /* Mv0.w == 1: the snapshot knows the surface point */
    uint64_t sky_pixels;       /* Mv0.w == 0: the centre ray hit nothing */
    uint64_t unmatched_pixels; /* Mv0.w == -1: a mesh the snapshot does not hold */
    uint64_t reserved;         /* 0 */
} hr_motion_trace_result;

typedef struct hr_motion_result {
    uint64_t reused_pixels;   /* as hr_history_result */
    uint64_t rejected_pixels;
    uint64_t history_samples;
    uint32_t history_passes;
    uint32_t passes;
    uint64_t surface_pixels;  /* as hr_motion_trace_result */
    uint64_t sky_pixels;
    uint64_t unmatched_pixels;
} hr_motion_result;

typedef struct hr_motion_info_t {
    int32_t snapshot;   /* 1: there is a snapshot */
    int32_t traced;     /* 1: the motion planes hold a trace at this frame size */
    uint32_t triangles; /* of the snapshot */
    uint32_t meshes;    /* of the snapshot */
    uint64_t bytes;     /* device memory of the snapshot and the planes */
} hr_motion_info_t;

/* hr_history_default_params with normal_cos = 0.8 */
void hr_motion_default_params(hr_history_params *p);

/* Every refusal below is HR_ERR_INVALID and hr_last_error names the cause. */

/* Remembers the committed pose (THE SNAPSHOT); a second snapshot replaces the first.  Refused: "scene not committed"; a context group;
 * a tile-sharded context. */
int hr_motion_snapshot(hr_ctx *ctx);
/* Writes the motion planes for `camera` (view_matrix, fov_tan and aspect_ratio are read); synchronous (the counters come back).  out may
 * be NULL.  Refused: a null or non-finite camera; a context group; a tile-sharded context; "no frame"; "scene not committed"; no
 * snapshot. */
int hr_motion_trace(hr_ctx *ctx, const hr_pass_params *camera, hr_motion_trace_result *out);
/* Completes the enqueued passes, runs the trace for `camera`, then adds the captured history to the frame and the planes (THE MERGE);
 * synchronous.  params == NULL: hr_motion_default_params.  out may be NULL.  Refused: what hr_motion_trace refuses; parameters out of
 * range or not finite; HR_AOV_SURFACE | HR_AOV_MOMENTS not both enabled, or enabled after the frame's first pass; an empty frame
 * (0 passes); no captured history; a second merge into the same frame, by this call, hr_history_merge or hr_reproject_merge. */
int hr_motion_merge(hr_ctx *ctx, const hr_pass_params *camera, const hr_history_params *params, hr_motion_result *out);
/* W x H float4 (MOTION VECTORS) from the planes of the last trace -> device_out, DEVICE memory reachable from the context's device and
 * 16-byte aligned, on `stream` (a hipStream_t; NULL: the context's) behind the trace; asynchronous.  old_camera == NULL: the captured
 * history's camera.  Refused: "null output"; a non-finite old_camera; NULL without a captured history; no trace at this frame size. */
int hr_motion_vectors(hr_ctx *ctx, const hr_pass_params *old_camera, float *device_out, void *stream);
/* The same image -> host_out (W x H x 4 floats of the caller's) through the feature's pinned buffer; synchronous. */
int hr_motion_vectors_readback(hr_ctx *ctx, const hr_pass_params *old_camera, float *host_out);
/* The two motion planes, for inspection and tests: Mv0 then Mv1 -> host_out (2 x W x H x 4 floats of the caller's); synchronous.
 * Refused: "null output"; no trace at this frame size. */
int hr_motion_readback(hr_ctx *ctx, float *host_out);
/* The snapshot's triangles, for inspection and tests: 12 floats per triangle in prim order (p0.xyz e1.x | e1.yz e2.xy | e2.z 0 0 0) ->
 * host_out; synchronous.  Refused: "null output"; no snapshot. */
int hr_motion_snapshot_readback(hr_ctx *ctx, float *host_out);
/* Frees the snapshot and the motion planes (no error when there are none). */
int hr_motion_drop(hr_ctx *ctx);
int hr_motion_info(hr_ctx *ctx, hr_motion_info_t *out);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_MOTION_H */
