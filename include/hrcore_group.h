/*
 * hrcore_group.h — context groups of libhrcore: one frame rendered by N member contexts, driven through ONE hr_ctx handle.
 *
 * Member i is rank i of world N (it renders the pixel tiles t with t % N == i, see hr_ctx_desc) on device_ids[i]; the group
 * assembles the members' tiles into one full frame on device_ids[0].  The handle a group hands out is an ordinary hr_ctx*: every
 * hrcore.h call takes it.  Scene, texture, material, light and table calls go to every member (in parallel, the call returns when
 * all have finished; ids they return are the same on every member); hr_render_pass posts the pass to every member and returns;
 * hr_readback / hr_display / hr_frame_device_ptr complete the members' passes and assemble; the progressive read-backs assemble the
 * passes each member has resolved so far without completing the rest.  hr_get_kernel_times, hr_get_step_log,
 * hr_frame_bind_external, hr_frame_packed_slots, hr_frame_pack_owned and hr_frame_unpack return HR_ERR_UNSUPPORTED on a group
 * (per-member counters: hr_group_member_stats).  Member device ids may repeat: N members on one device are the one-device
 * emulation of an N-way split.
 *
 * Each member is driven by a host thread of its own (the library's); the caller's thread contract is that of a plain context.
 * An error of a member's asynchronous work is returned by the group's next call, as "member i (device d): ...".
 *
 * Not part of hrcore.h: that header's ABI version does not change with these calls; this one has its own.
 */
#ifndef HRCORE_GROUP_H
#define HRCORE_GROUP_H

#include "hrcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HR_GROUP_API_VERSION 1u
uint32_t hr_group_api_version(void);

#define HR_GROUP_MAX_MEMBERS 16

/* N member contexts behind one handle; member i = rank i of world n.  device_ids may repeat; NULL / n = 0: every visible device
 * once.  desc: tile_size, flags, memory_budget (per member) and stream (the assembly stream, on device_ids[0]) as for
 * hr_ctx_create; desc->device_id is ignored, desc->rank must be 0 and desc->world 1 (HR_ERR_INVALID otherwise, as for
 * n > HR_GROUP_MAX_MEMBERS or a bad device id).  The handle is used with every hrcore.h call; hr_ctx_destroy destroys the members. */
int hr_ctx_create_group(const hr_ctx_desc *desc, const int32_t *device_ids, int32_t n, hr_ctx **out);

typedef struct hr_group_info {
    int32_t n_members;
    int32_t device_ids[HR_GROUP_MAX_MEMBERS];
    uint64_t owned_pixels[HR_GROUP_MAX_MEMBERS]; /* pixels of the current frame member i renders (0 before hr_frame_resize) */
} hr_group_info;
/* HR_ERR_INVALID on a plain context */
int hr_group_get_info(hr_ctx *group, hr_group_info *out);

/* One member's counters (either pointer may be NULL); completes that member's enqueued passes first, like hr_get_stats. */
int hr_group_member_stats(hr_ctx *group, int32_t member, hr_pass_stats *stats, hr_kernel_times *times);

#ifdef __cplusplus
}
#endif
#endif /* HRCORE_GROUP_H */
