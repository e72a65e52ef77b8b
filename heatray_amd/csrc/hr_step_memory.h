// hr_step_memory.h — the bytes of a macro step's ray memory, stated ONCE: what a pass's table entry takes from its group's scratch region and from
// the step arena (hr_ctx::Group).  The step's need, the memory budget's per-stage record and the carve of hr_pipeline.inl all come from
// segmentBytes and queuePlaneBytes, and the budget's guarantee for stages not yet seen from the same per-ray constants: a need and a carve
// that disagree are a write past a region.  Host-only C++ without a HIP include, so that tests/host/step_memory_cpu.cpp checks it without a device.
#pragma once
#include <cstddef>
#include <cstdint>

static const size_t kQueuePlaneEntryBytes = 16; // a queue is planes of float4 / int4, one entry per ray and plane
static const size_t kRayQueuePlanes = 4, kShadowQueuePlanes = 3; // RayQueue A..D, ShadowQueue A..C (hr_kernels.h)
static const size_t kRayQueueBytesPerRay = kRayQueuePlanes * kQueuePlaneEntryBytes;       // closest-hit queue: 64 B
static const size_t kShadowQueueBytesPerRay = kShadowQueuePlanes * kQueuePlaneEntryBytes; // occlusion queue: 48 B
static const size_t kHitListEntryBytes = 4; // an index into the hit records

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline size_t queuePlaneBytes(size_t cap) { return align256(cap * kQueuePlaneEntryBytes); } // one plane of a queue of `cap` entries
static inline size_t rayQueueBytes(size_t cap) { return kRayQueuePlanes * queuePlaneBytes(cap); }
static inline size_t shadowQueueBytes(size_t cap) { return kShadowQueuePlanes * queuePlaneBytes(cap); }

struct SegmentBytes {
    size_t scratch, arena;
};
// One pass's entry of a step table.  In its first step the pass's P camera rays live in scratch; while it traces closest hits it takes
// hit records and a hit list of `bound` entries from scratch and, from the arena, the queues its shading emits into: `bound` rays and kS
// occlusion rays for each of them.
static inline SegmentBytes segmentBytes(uint32_t P, uint32_t bound, size_t kS, size_t hitRecordBytes, bool firstStep, bool closest)
{
    SegmentBytes b{0, 0};
    if (firstStep) b.scratch += rayQueueBytes(P);
    if (closest) {
        b.scratch += align256((size_t)bound * hitRecordBytes) + align256((size_t)bound * kHitListEntryBytes);
        b.arena += rayQueueBytes(bound) + shadowQueueBytes((size_t)bound * kS);
    }
    return b;
}

// The memory budget's guarantee for a stage no step has carved yet (budgetBytesPerPass): one ray per owned pixel, unaligned.
static inline double guaranteedArenaBytes(double P, double kS) { return P * ((double)kRayQueueBytesPerRay + (double)kShadowQueueBytesPerRay * kS); }
static inline double guaranteedScratchBytes(double P, size_t hitRecordBytes, bool firstStage)
{
    return P * (double)(hitRecordBytes + kHitListEntryBytes) + (firstStage ? P * (double)kRayQueueBytesPerRay : 0.0);
}
