/*
 * hrcore_deform.h — deformable meshes: new vertex data for a resident mesh without touching its topology, posed on the device from a
 * few matrices and weights where the caller has them, and read back.
 *
 * hr_geom_set_transform keeps the tree: the next hr_scene_commit re-assembles the triangles into their leaf slots and refits.  A mesh
 * whose VERTICES move while its indices stay (a simulation's surface, a skinned character, a morph, a height field being sculpted) had
 * only hr_geom_remove + hr_geom_add, which uploads every attribute and the indices again and rebuilds the tree.  Here:
 *
 *     hr_geom_update(ctx, id, &desc, &params, &r);        desc: the new positions (and any other attribute), host arrays
 *     hr_scene_commit(ctx);                                the refit branch, its box-area guard deciding as after a set_transform
 * or, with the data made on the device:
 *     hr_deform_bind(ctx, id, &rig);                       once: the rest pose is the mesh as it stands; morph deltas, joints, weights
 *     hr_deform_pose(ctx, id, morph_weights, joint_matrices, &params, &r);     per frame: 64 bytes per joint cross the bus
 *     hr_scene_commit(ctx);
 *
 * THE BLOCK.  A mesh lives in one device block with the layout it was added with (offsets, strides, interleaving); every call below
 * writes into or reads from that block and never changes the layout.  Attributes are numbered in the order of hr_mesh_desc
 * (HR_GEOM_*).
 *
 * hr_geom_update.  WHAT IS READ FROM desc: positions (required); each of normals, uvs, tangents, bitangents, colors that is not NULL
 * replaces that attribute, a NULL one is left as it is; the strides exactly as hr_geom_add reads them (0 = tightly packed; strides
 * that are no multiple of four and interleaved buffers included); n_vertices, which must be the mesh's.  indices, n_indices, mode,
 * world_from_entity and the remaining fields are NOT read: topology and transform stay.
 *
 * REGENERATION.  params->regenerate & HR_DEFORM_NORMALS: the mesh's normals are computed from the new positions, the mesh's own indices
 * and mode; with HR_DEFORM_TANGENTS also its tangents and bitangents, from the uvs the block holds after this call.  They are, byte for
 * byte, what hr_mesh_prepare returns for those arrays with {weight, weld, want = regenerate} (include/hrcore_mesh.h is that contract;
 * the same kernels run).  The weld is recomputed from the new positions on every regeneration.
 *
 * SCENE STATE changes exactly as for hr_geom_set_transform: the scene is no longer committed (hr_render_pass fails with "scene not
 * committed" until the next hr_scene_commit), topology is NOT dirty, the next commit refits and its guard decides whether the kept tree
 * has become too loose.  Only a commit reads a mesh block, and it runs behind these calls on the context's stream, so the calls do not
 * wait for passes in flight: those read the committed triangle arrays, which a commit alone rewrites.
 *
 * hr_geom_get_attribute is synchronous and returns one attribute tightly packed.
 *
 * hr_deform_bind snapshots the mesh's current positions and normals (and its tangents and bitangents when it has both) as the REST POSE
 * in tight device arrays, and uploads the rig.  A second bind replaces the first.  hr_geom_update on a bound mesh does not change the
 * rest pose.  The binding is freed by hr_deform_unbind, hr_geom_remove, hr_scene_clear and hr_ctx_destroy.
 *
 * hr_deform_pose, per vertex v.  ARITHMETIC: the project's contract — one binary32 operation per written operation, in the order
 * written, no contraction; normalize, dot and valid as include/hrcore_mesh.h defines them.  mw = morph_weights, M = one joint's 16
 * floats, column-major.
 *
 *     p = restP[v];  n = restN[v];  t = restT[v];  b = restB[v]
 *     for k = 0 .. n_morph-1:   p = p + dP[k][v] * mw[k]                    (component-wise)
 *                               n = n + dN[k][v] * mw[k]                    (only with morph_normals)
 *     if n_joints > 0:
 *         P = N = T = B = +0
 *         for i = 0 .. 3:  w = weights[v][i];  if w == 0: continue;  M = joint_matrices[joints[v][i]]
 *             P = P + point(M, p) * w     point(M,p).x = ((M[0]*p.x + M[4]*p.y) + M[8]*p.z) + M[12]   (.y: 1,5,9,13  .z: 2,6,10,14)
 *             N = N + dir(M, n) * w       dir(M,d).x   =  (M[0]*d.x + M[4]*d.y) + M[8]*d.z            (likewise; same for T, B)
 *         p = P;  n = N;  t = T;  b = B
 *     position:   every component finite and |.| <= 3e37 ? p : restP[v], counted rejected
 *     normal:     written only if morph_normals or n_joints > 0:  valid(dot(n,n)) ? normalize(n) : restN[v], counted kept
 *     tangent, bitangent: written only if n_joints > 0 and the mesh has both: likewise, each counted kept on its own
 *
 * An attribute that is not written keeps what the block holds.  params->regenerate then acts on the posed positions exactly as in
 * hr_geom_update; regenerated arrays replace the posed ones.  The scene-state rules are hr_geom_update's.  heatray_amd/csrc/hr_deform.h
 * holds these lines; heatray_amd/deform.py restates them in numpy float32, bit for bit.
 *
 * LIMITS.
 *   - Directions go through the joint's 3x3, not its inverse transpose: exact for rigid joints and uniform scale, an approximation
 *     under shear or non-uniform scale.
 *   - Weights are used as given: nothing is renormalised, four influences per vertex, a weight of 0 (or -0) skips its joint.
 *   - Every regeneration redoes the weld and the corner sort, although the sort depends on the indices alone.
 *
 * MEMORY.  A binding holds 12 bytes per vertex and rest array (2 or 4 arrays), 12 or 24 per vertex and morph, 32 per vertex with
 * joints, and 32 + 64 n_joints bytes for a pose's weights and matrices: sized by the mesh and the rig.  The calls' tight staging is the
 * context's mesh scratch (include/hrcore_mesh.h, MEMORY), grown only.  Neither is counted against hr_ctx_desc::memory_budget.
 *
 * GROUPS AND SHARDS.  Every call goes to every member of a context group, like hr_geom_add; the read-back and the result come from the
 * first member.  A tile-sharded context is served.  hr_mesh_last is not changed by any of these calls.  Without a call every bit of
 * every frame, plane, counter and hr_scene_info is what it is in a library without this header.
 *
 * Not part of hrcore.h or any other header: their versions do not change with these calls; this header has its own.
 */
#ifndef HRCORE_DEFORM_H
#define HRCORE_DEFORM_H

#include "hrcore_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_DEFORM_API_VERSION 1u
uint32_t hr_deform_api_version(void);

/* the attributes of a mesh, in the order of hr_mesh_desc */
#define HR_GEOM_POSITIONS 0
#define HR_GEOM_NORMALS 1
#define HR_GEOM_UVS 2
#define HR_GEOM_TANGENTS 3
#define HR_GEOM_BITANGENTS 4
#define HR_GEOM_COLORS 5

#define HR_DEFORM_NORMALS 1  /* regenerate: normals from the new positions, hr_mesh_prepare's arithmetic */
#define HR_DEFORM_TANGENTS 2 /* ... and tangent frames; only together with HR_DEFORM_NORMALS */
#define HR_DEFORM_MAX_MORPH 8
#define HR_DEFORM_MAX_JOINTS 1024

typedef struct hr_deform_params {
    int32_t regenerate;  /* 0 or HR_DEFORM_NORMALS [| HR_DEFORM_TANGENTS] */
    int32_t weight;      /* HR_MESH_WEIGHT_*, read with regenerate */
    int32_t weld;        /* 0 / 1, read with regenerate */
    int32_t reserved[5]; /* 0 */
} hr_deform_params;

typedef struct hr_deform_rig {
    const float *morph_positions; /* n_morph x n_vertices x 3 deltas, tightly packed; NULL iff n_morph == 0 */
    const float *morph_normals;   /* the same shape, or NULL: normals are not morphed */
    const uint32_t *joints;       /* n_vertices x 4; NULL iff n_joints == 0 */
    const float *weights;         /* n_vertices x 4; NULL iff n_joints == 0 */
    int32_t n_morph, n_joints, reserved[6];
} hr_deform_rig;

typedef struct hr_deform_result {
    uint64_t vertices, triangles;
    uint64_t rejected_vertices; /* pose: the posed position was not finite; the vertex kept its rest position */
    uint64_t kept_directions;   /* pose: directions whose posed length was not valid and that kept their rest value */
    uint32_t regenerated, posed; /* the regenerate mask that ran; 1 after hr_deform_pose */
    hr_mesh_result mesh;        /* the regeneration's counters, all 0 without one */
} hr_deform_result;

/* regenerate 0, weight ANGLE, weld 1; NULL is ignored */
void hr_deform_default_params(hr_deform_params *p);

/* New vertex data for a live mesh (above).  params == NULL: the defaults; out may be NULL.  HR_ERR_INVALID (hr_last_error names the
 * cause; the context stays usable and the block is untouched: every refusal is decided on the host before anything is launched): a bad
 * or dead id ("bad geom id"); "null desc"; "null positions"; another vertex count ("n_vertices = 5 but the mesh has 6"); an attribute
 * given that the mesh was added without ("the mesh has no tangents"); "attribute stride smaller than the attribute"; positions that are
 * not finite (hr_geom_add's rule: "vertex positions must be finite"); "unknown regenerate 4"; "regenerate TANGENTS needs NORMALS";
 * "unknown weight 3"; "weld = 2 is neither 0 nor 1"; "reserved[0] must be 0"; regenerate & NORMALS with desc->normals given
 * ("normals are both given and regenerated"); regenerate & TANGENTS with desc->tangents or desc->bitangents given ("tangents are both
 * given and regenerated"); regenerate & TANGENTS on a mesh that lacks uvs, tangents or bitangents ("regenerate TANGENTS needs a mesh
 * with uvs, tangents and bitangents"). */
int hr_geom_update(hr_ctx *ctx, hr_geom_id id, const hr_mesh_desc *desc, const hr_deform_params *params, hr_deform_result *out);

/* One attribute (HR_GEOM_*) of a live mesh -> out: the caller's host array, tightly packed, n_vertices x 3 floats (2 for uvs).
 * Synchronous.  HR_ERR_INVALID: "bad geom id", "unknown attribute 6", "the mesh has no colors", "null output". */
int hr_geom_get_attribute(hr_ctx *ctx, hr_geom_id id, int32_t attribute, float *out);

/* The mesh as it stands becomes the rest pose; the rig is copied.  HR_ERR_INVALID: "bad geom id"; "null rig"; n_morph outside
 * 0 .. HR_DEFORM_MAX_MORPH ("n_morph = 9"); n_joints outside 0 .. HR_DEFORM_MAX_JOINTS ("n_joints = 1025"); both 0 ("a rig needs
 * morphs or joints"); the pointer rules of hr_deform_rig ("null morph_positions", "morph_positions without morphs", "morph_normals
 * without morphs", "null joints", "null weights", "joints or weights without joints"); "joint index out of range"; a weight or a delta
 * that is not finite, |x| <= 3e37 ("weights must be finite", "morph deltas must be finite"); "reserved[0] must be 0". */
int hr_deform_bind(hr_ctx *ctx, hr_geom_id id, const hr_deform_rig *rig);

/* morph_weights: n_morph floats; joint_matrices: n_joints x 16 floats, column-major (NULL where the rig has none of the kind).
 * params == NULL: the defaults; out may be NULL.  HR_ERR_INVALID: "bad geom id"; "the mesh is not bound"; "null morph_weights"; "null
 * joint_matrices"; "morph weights must be finite"; "joint matrices must be finite" (|x| <= 3e37); and what hr_geom_update says about
 * params. */
int hr_deform_pose(hr_ctx *ctx, hr_geom_id id, const float *morph_weights, const float *joint_matrices, const hr_deform_params *params,
                   hr_deform_result *out);

/* HR_ERR_INVALID: "bad geom id", "the mesh is not bound" */
int hr_deform_unbind(hr_ctx *ctx, hr_geom_id id);

/* the result of the context's last successful hr_geom_update or hr_deform_pose (HR_ERR_INVALID before the first) */
int hr_deform_last(hr_ctx *ctx, hr_deform_result *out);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_DEFORM_H */
