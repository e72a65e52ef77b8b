/*
 * hrcore_tree.h — what the last build of the acceleration structure did to the radix tree's bottom subtrees.
 *
 * hr_scene_commit builds a radix tree over the Morton-sorted triangles (and a PLOC tree beside it: hr_scene_info's builder / cost_radix /
 * cost_ploc).  With HR_TUNE sahsub=T (default 64; 0: off) every subtree of 3 .. T triangles under a node of more than T is rebuilt
 * top-down by full-sweep SAH, and the rebuilt version is kept where its collapse cost is lower and it is not deeper than the radix
 * subtree it replaces.  cost_radix of hr_scene_info is the radix candidate's cost AFTER that step; this call reports the cost before
 * it and how many subtrees there were.  Hits do not depend on the tree: the step changes node visits, never a pixel.
 *
 * Since version 2 the committed tree can also be read back, array by array, as the traversal kernels see it: what tests/tree_audit.py
 * checks against float64 truth.  Plain copies after the commit; nothing on the render path reads them.
 *
 * Not part of hrcore.h: its version and hr_scene_info do not change with these calls; this header has its own version.
 */
#ifndef HRCORE_TREE_H
#define HRCORE_TREE_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_TREE_API_VERSION 2u /* 2: hr_scene_tree_layout, hr_scene_tree_read */
uint32_t hr_tree_api_version(void);

typedef struct hr_tree_info {
    float cost_before;          /* summed surface area of the 4-wide nodes / the root's, for the radix tree as k_karras made it ...        */
    float cost_after;           /* ... and with the kept subtrees in place (never larger).  Both 0: no rebuild ran (sahsub=0, a scene of at
                                 * most T triangles, a refit, a tree read from the cache file)                                               */
    uint32_t subtrees_found;    /* bottom subtrees of 3 .. T triangles                                                                      */
    uint32_t subtrees_replaced; /* ... whose full-sweep SAH version was kept                                                                */
    uint32_t max_triangles;     /* T of the build (0: off)                                                                                  */
    uint32_t reserved[3];       /* 0 */
} hr_tree_info;

/* the values of the last hr_scene_commit that built the tree (a refit keeps them); HR_ERR_INVALID before the first commit */
int hr_scene_get_tree_info(hr_ctx *ctx, hr_tree_info *out);

/* ---- the committed tree, read back (version 2).  The arrays, in the layouts of DESIGN.md "Data layout in HBM": */
#define HR_TREE_NODE4 0        /* n_nodes x 64 bytes: the 4-wide node of the packet kernel and the root cull                               */
#define HR_TREE_NODE32 1       /* n_nodes x 32 bytes: the same node as k_trace reads it, on the scene's grid                               */
#define HR_TREE_LEAF_KEYS 2    /* n_nodes x int32: the reference of a node's leaf child j is leaf_key + j = ~(its slot in HR_TREE_TRIS)     */
#define HR_TREE_TRIS 3         /* tri_slots x 48 bytes: (v0, e1, e2, prim id, flags, -) in leaf order                                      */
#define HR_TREE_NODE_BOX 4     /* n_nodes x 6 floats: lo.xyz, hi.xyz of every node, what a refit passes upwards                            */
#define HR_TREE_SLOT_OF_PRIM 5 /* n_triangles x uint32: prim id -> slot in HR_TREE_TRIS                                                    */
#define HR_TREE_ARRAYS 6

typedef struct hr_tree_layout {
    uint64_t n_nodes, n_triangles, tri_slots;
    uint32_t root_leaf_count;   /* > 0: the root is a leaf of that many triangles and there are no nodes                                   */
    uint32_t levels;            /* hr_scene_info's bvh_levels: the nodes of level L are [level_start[L], level_start[L + 1])               */
    uint32_t level_start[65];
    uint32_t grid_cell_exp[3];  /* biased exponent of grid_cell                                                                            */
    float pad, hit_pad;         /* the leaf padding (1e-5 |diagonal|) and the half of it the hit test grows a triangle's box by           */
    float ray_epsilon;
    float grid_lo[3], grid_cell[3]; /* the 32-byte node's frame origin is grid_lo + g * grid_cell                                          */
    float lo[3], hi[3];         /* the scene's bounds                                                                                      */
    uint32_t reserved;          /* 0 */
    uint64_t bytes[HR_TREE_ARRAYS]; /* size of each array above                                                                            */
} hr_tree_layout;

/* HR_ERR_INVALID before the first commit and for a null `out`; a context group is refused (its members hold a tree each), a tile-sharded
 * context answers */
int hr_scene_tree_layout(hr_ctx *ctx, hr_tree_layout *out);
/* copies array `what` into dst, of which `capacity` bytes may be written: refused when that is less than the layout's bytes[what] */
int hr_scene_tree_read(hr_ctx *ctx, int32_t what, void *dst, uint64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_TREE_H */
