/*
 * hrcore_tree.h — what the last build of the acceleration structure did to the radix tree's bottom subtrees.
 *
 * hr_scene_commit builds a radix tree over the Morton-sorted triangles (and a PLOC tree beside it: hr_scene_info's builder / cost_radix /
 * cost_ploc).  With HR_TUNE sahsub=T (default 64; 0: off) every subtree of 3 .. T triangles under a node of more than T is rebuilt
 * top-down by full-sweep SAH, and the rebuilt version is kept where its collapse cost is lower and it is not deeper than the radix
 * subtree it replaces.  cost_radix of hr_scene_info is the radix candidate's cost AFTER that step; this call reports the cost before
 * it and how many subtrees there were.  Hits do not depend on the tree: the step changes node visits, never a pixel.
 *
 * Not part of hrcore.h: its version and hr_scene_info do not change with this call; this header has its own version.
 */
#ifndef HRCORE_TREE_H
#define HRCORE_TREE_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_TREE_API_VERSION 1u
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

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_TREE_H */
