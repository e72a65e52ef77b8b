// hr_features.h — the state of the optional post-process features, one struct per feature, each a member of hr_ctx (hr_ctx.h includes this
// file).  What a struct owns is a handle of hr_owned.h, so assigning it a default-constructed one frees everything and resets every flag:
// that is release().  The four lifetime functions of hr_postprocess.inl are the only callers (hr_history_drop and hr_motion_drop apart) and the only code
// that resets a feature's flags.  A read-back's pinned staging only grows (growPinned, hr_ctx.h): a shrinking frame keeps its buffer.
#pragma once
#include "hr_owned.h"

#include <vector>

// The result counters of a post-process feature: a few device words its kernel adds into and their pinned host copy.  A call runs
// ensure, zero, its launches and fetch (each under HIP_TRY), synchronises the stream and fills its result struct from `host`.
template <class Word> struct ResultCounters {
    DeviceBuf<Word> dev;
    PinnedBuf<Word> host;
    size_t words = 0;
    hipError_t ensure(size_t n) // both buffers of n words, made by the first call
    {
        words = n;
        const hipError_t e = dev ? hipSuccess : dev.alloc(n);
        return e == hipSuccess && !host ? host.alloc(n) : e;
    }
    hipError_t zero(hipStream_t st) { return hipMemsetAsync(dev, 0, words * sizeof(Word), st); }
    // enqueues dev -> host and does not wait: the caller synchronises `st`, once, with whatever else it copies back
    hipError_t fetch(hipStream_t st) { return hipMemcpyAsync(host, dev, words * sizeof(Word), hipMemcpyDeviceToHost, st); }
};

// AOVs (include/hrcore_aov.h): the frame's planes, summed by k_resolve_aov in pass order beside the frame.  With HR_AOV_SURFACE every
// pass slot also holds the pass's AOV record (PassSlot::aov) and the shading kernel variant with MODE & 4 writes it.
struct AovState {
    uint32_t mask = 0;
    DeviceBuf<float> plane[3];                     // W x H float4 each (HR_AOV_PLANE_*), null when not enabled
    PinnedBuf<float> pinned;                       // hr_aov_readback's host buffer
    unsigned long long zeroedAt = 0;               // value of nextResolveOrder when the planes were last zeroed
    size_t framesPerSlot() const { return (mask & HR_AOV_SURFACE) ? 2 : 0; }
    void freePlanes() { for (DeviceBuf<float> &p : plane) p.reset(); }
    void release() { *this = AovState(); }
};

// Denoiser (include/hrcore_denoise.h): working planes and result image, allocated by the first call, freed with the AOV planes
struct DenoiseState {
    DeviceBuf<float> work; // kDenoiseBytesPerPixel x W x H, cut into DenoiseBufs
    DeviceBuf<float> out;  // the result when it does not go straight to the caller's memory (W x H float4)
    PinnedBuf<float> pinned; // hr_denoise_readback's host buffer
    ResultCounters<unsigned long long> spatial; // kDenoiseSpatialResultWords (include/hrcore_denoise_spatial.h): made and freed with `work`
    void release() { *this = DenoiseState(); }
};

// Adaptive sampling (include/hrcore_adaptive.h).  frame.mask is maskWords while a mask is installed, null otherwise.  The buffers are made
// by the first call that needs them and go with the frame's size.
struct AdaptiveState {
    DeviceBuf<uint32_t> maskWords;  // the installed mask's words (sampleMaskWords)
    DeviceBuf<uint8_t> maskBytes;   // W x H bytes: staging of the byte form (hr_sample_mask_set / _get)
    DeviceBuf<float> error;         // W x H floats: the error map of the last hr_adaptive_update
    DeviceBuf<uint32_t> builtWords; // the mask that update built (copied to maskWords when it is installed)
    ResultCounters<uint32_t> result; // kAdaptiveResultWords
    bool errorValid = false;        // `error` holds an update's map at this frame size
    void release() { *this = AdaptiveState(); }
};

// History reprojection (include/hrcore_history.h).  The history survives hr_clear; it goes with the frame's size and with hr_history_drop.
struct HistoryState {
    DeviceBuf<float> hist;   // kHistoryBytesPerPixel x W x H: H0, H1, H2
    bool captured = false;   // `hist` holds a capture
    uint32_t passes = 0;     // complete passes of the frame it was captured from
    float view[16] = {0}, fovTan = 0.0f, aspect = 0.0f; // ... and its camera
    bool merged = false;     // the history has been merged into the frame since its last hr_clear
    ResultCounters<unsigned long long> result; // kHistoryResultWords
    void release() { *this = HistoryState(); }
};

// Progressive merge and preview (include/hrcore_reproject.h).  Everything here goes with the frame's size; hr_clear marks the examined bits
// stale and the next hr_reproject_merge zeroes them.
struct ReprojectState {
    DeviceBuf<unsigned long long> examined; // rpExaminedWords(W, H) words: one per 8 x 8 block of pixels
    bool stale = true;                      // the bits belong to an earlier frame (or were never zeroed): all pixels count as not examined
    bool merged = false;                    // hr_reproject_merge has merged into the frame since its last hr_clear (history.merged is set with it)
    ResultCounters<unsigned long long> result; // kReprojectResultWords (the preview uses the first three)
    DeviceBuf<float> out;                   // the preview when it does not go straight to the caller's memory (W x H float4)
    PinnedBuf<float> pinned;                // hr_reproject_preview_readback's host buffer
    void release() { *this = ReprojectState(); }
};

// Auto-exposure (include/hrcore_exposure.h).  Nothing here depends on the frame's size: hr_clear and hr_frame_resize leave it alone, it goes
// with the context.
struct ExposureState {
    ResultCounters<unsigned long long> bins; // kExWords of hr_exposure.h: the last metering's bins, class counters and reduced words
    DeviceBuf<uint32_t> state;               // {there is an adaptation state, its scale's bits} on the device: hr_exposure_reset zeroes it
    bool metered = false;                    // `bins` holds a metering (hr_exposure_last)
    void release() { *this = ExposureState(); }
};

// The convergence metric (include/hrcore_metric.h).  Nothing here depends on the frame's size: hr_clear and hr_frame_resize leave it alone,
// it goes with the context.
struct MetricState {
    ResultCounters<unsigned long long> bins; // kMtWords of hr_metric.h: the last measurement's bins, counters and max_abs bits
    uint32_t kind = 0, passes = 0;           // ... its kind (HR_METRIC_*) and the frame's passes in it
    bool measured = false;                   // `bins` holds a measurement (hr_metric_last)
    void release() { *this = MetricState(); }
};

// Firefly suppression (include/hrcore_despeckle.h).  The planes are made by the first call whose output does not go straight to the
// caller's memory and go with the denoiser's buffers: the denoiser can be run from them.
struct DespeckleState {
    DeviceBuf<float> planes;                   // 2 x W x H float4: the despeckled frame, then the despeckled moments
    PinnedBuf<float> pinned;                   // the read-backs' host buffer: the same two images
    ResultCounters<unsigned long long> result; // kDespeckleResultWords
    void release() { *this = DespeckleState(); }
};

// Mesh preparation (include/hrcore_mesh.h).  Nothing here depends on the frame or the scene: one block of scratch sized by the largest
// mesh prepared so far, grown only, not counted against memBudget; it goes with the context.  On a group's handle only `last` and
// `prepared` are used: the call itself runs on the first member.
struct MeshPrepState {
    DeviceBuf<char> scratch;                     // (its capacity: the bytes)
    ResultCounters<unsigned long long> counters; // kMsCounterWords
    hr_mesh_result last{};                       // the last successful hr_mesh_prepare's result
    bool prepared = false;                       // ... there has been one (hr_mesh_last)
    void release() { *this = MeshPrepState(); }
};

// Deformable meshes (include/hrcore_deform.h).  The bindings belong to their meshes (Geom::deform, hr_ctx.h); here are only the pose
// kernel's two counters and the last result.  On a group's handle only `last` and `done` are used.
struct DeformState {
    ResultCounters<unsigned long long> counters; // kDfCounterWords
    hr_deform_result last{};                     // the last successful hr_geom_update's or hr_deform_pose's result
    bool done = false;                           // ... there has been one (hr_deform_last)
    void release() { *this = DeformState(); }
};

// Ray queries (include/hrcore_query.h).  Nothing here depends on the frame: it goes with the context.  The scratch stages the host calls
// (rays in, answers out), grown only, not counted against memBudget.  `geoms` is the table from a committed mesh's first triangle to its
// hr_geom_id, uploaded by the first query after a commit (geomsStale).  evDone is recorded behind every query on the stream it ran on:
// wait() is what quiesce and hr_ctx_destroy call before anything a query reads is rewritten or freed, and what hr_query_last waits on.
// On a group's handle nothing is used: member 0 serves the calls.
struct QueryState {
    DeviceBuf<char> scratch;                     // (its capacity: the bytes)
    DeviceBuf<hr::QyGeom> geoms;
    int nGeoms = 0;
    bool geomsStale = true;
    ResultCounters<unsigned long long> counters; // kQyCounterWords; the copy to `host` is enqueued behind every query
    Event evOrder, evDone;            // made by the first query
    hipStream_t lastStream = nullptr; // the stream evDone was last recorded on (the caller's or the context's: not owned)
    bool inFlight = false;            // evDone has been recorded and not waited for
    uint64_t lastRays = 0;            // n of the last successful call
    bool done = false;                // ... there has been one (hr_query_last)
    hipError_t wait()
    {
        if (!inFlight) return hipSuccess;
        inFlight = false;
        return hipEventSynchronize(evDone);
    }
    void release() { wait(), *this = QueryState(); } // (nothing may read the memory or wait on evDone when the members go)
};

// Motion reprojection (include/hrcore_motion.h).  The snapshot (the committed pose's triangles and its table of meshes) does not depend on
// the frame: it survives hr_clear, commits and hr_frame_resize and goes with hr_motion_drop, a second snapshot and the context.  The
// motion planes and what hangs on them go with the frame's size (releaseFrame).  Nothing here is counted against memBudget.
struct MotionState {
    struct Mesh {
        int32_t id;            // hr_geom_id
        uint32_t first, count; // its triangles in `snap`
    };
    DeviceBuf<float> snap;   // kMotionSnapshotFloatsPerTri per triangle, prim order
    std::vector<Mesh> meshes; // the committed meshes that have triangles, in id order
    uint32_t nTris = 0;
    bool have = false;        // there is a snapshot (of a scene without triangles: `snap` is null)
    DeviceBuf<float> planes;  // kMotionPlaneBytesPerPixel x W x H: Mv0, Mv1
    bool traced = false;      // `planes` holds a trace
    float view[16] = {0}, fovTan = 0.0f, aspect = 0.0f; // ... and its camera
    DeviceBuf<int32_t> remap; // per committed mesh: its first triangle in `snap`, or -1 (rebuilt by every trace)
    DeviceBuf<float> out;     // the motion vectors on their way to the host (W x H float4)
    PinnedBuf<float> pinned;  // the read-backs' host buffer
    ResultCounters<unsigned long long> result; // kMotionTraceResultWords, then kMotionMergeResultWords
    void releaseFrame() // what was made for the frame's size
    {
        planes.reset(), out.reset();
        traced = false;
    }
    void release() { *this = MotionState(); }
};
