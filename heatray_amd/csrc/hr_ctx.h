// hr_ctx.h — the context behind the opaque hr_ctx handle of include/hrcore.h: everything one context owns on the device and the
// state of its pass pipeline, plus the error macros of the host side.  Included by hr_core.hip only (ONE translation unit: the
// host side's helpers keep internal linkage); hr_scene.inl and hr_pipeline.inl are that file's two large sections.  The state of the
// optional post-process features is one member each, of the structs of hr_features.h (with ResultCounters).
// Ownership: every device buffer, pinned buffer, event and stream the context holds is a handle of hr_owned.h, freed when the context
// (or the struct it is a member of) goes or is assigned a fresh one.  A raw pointer member owns nothing and says so: it aliases a
// handle's memory, is the caller's, or is one of the three kept raw on purpose (tree, Geom::dBlock, Geom::deform; DESIGN.md, "Ownership").
#pragma once
#include "hr_kernels.h"
#include "hr_trace.h"
#include "hr_tune.h"
#include "hr_step_memory.h"
#include "hr_owned.h"
#include "hr_features.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace hr;

namespace {

struct Texture {
    DeviceBuf<char> dpx;
    DeviceBuf<float> dmips; // levels >= 1 (HR_TEXTURE_LOD_CONE), built on first use
    TexDesc desc{};
    bool alive = false;
};

// What hr_deform_bind keeps for a mesh (include/hrcore_deform.h): ONE device allocation cut into the rest pose's tight arrays, the rig's
// arrays and a pose's weights and matrices.  Owned through Geom::deform, a plain pointer like Geom::chunk: a Geom is copied freely (the
// vector grows, hr_geom_remove assigns Geom()), so nothing is freed by a destructor; deformRelease (hr_deform.inl) is called wherever
// meshRelease or meshReleaseAll is, and by hr_deform_unbind and a second bind.
struct DeformBinding {
    char *dev = nullptr;
    float *restP = nullptr, *restN = nullptr, *restT = nullptr, *restB = nullptr; // V x 3 each; restT / restB null without tangent frames
    float *dP = nullptr, *dN = nullptr;                                         // nMorph x V x 3; dN null: normals are not morphed
    uint32_t *joints = nullptr;                                                 // V x 4
    float *weights = nullptr;                                                   // V x 4
    float *pose = nullptr; // HR_DEFORM_MAX_MORPH morph weights, then nJoints x 16 matrix words: uploaded by every hr_deform_pose
    int nMorph = 0, nJoints = 0;
};

// One submesh.  Its vertex attributes and indices live in ONE device block, uploaded when the mesh is added (straight from the
// caller's planar buffers through a pinned staging ring, with the caller's strides: nothing is de-interleaved or kept on the host).
struct Geom {
    bool alive = false;
    int nVerts = 0;
    uint32_t nIdx = 0;
    int mode = HR_TRIANGLES;
    float world[16];
    int frontFaceCW = 0, isOccluder = 1, material = 0;
    char *dBlock = nullptr;   // inside chunk `chunk` of the context's mesh arena, which owns it
    int chunk = -1;
    size_t blockBytes = 0;
    size_t off[7] = {0, 0, 0, 0, 0, 0, 0}; // byte offsets of pos, nrm, uv, tan, bit, col, idx in the block
    bool has[6] = {false, false, false, false, false, false};
    int stride[6] = {3, 3, 2, 3, 3, 3};     // floats between consecutive vertices
    DeformBinding *deform = nullptr;        // hr_deform_bind's (null: not bound); see DeformBinding for who frees it
    uint32_t nTris() const { return mode == HR_TRIANGLE_STRIP ? (nIdx >= 3 ? nIdx - 2 : 0u) : nIdx / 3; }
};

// frees the mesh's binding, if it has one (hipFree waits for the kernels that still read it)
inline void deformRelease(Geom &g)
{
    if (!g.deform) return;
    hipFree(g.deform->dev);
    delete g.deform;
    g.deform = nullptr;
}

} // namespace

struct GroupState; // hr_group.inl: what a context group owns beside its hr_ctx

static_assert(kMaxSlots == 2 * kMaxSegs, "hr_tune.h bounds depth= by the step table's size"); // (kMaxGroups, kMaxSlots: hr_tune.h)
#ifndef HR_BATCH_CAP
#define HR_BATCH_CAP 32 // most passes injected per macro step (small frames / tile shards reach it: 1/8 of a 1080p frame runs 6.6 % faster with 32 than with 12, profiles/r2p_shard_batch.txt)
#endif

struct hr_ctx {
    int device = 0;
    hipStream_t stream = nullptr; // the caller's (hr_ctx_desc::stream, hr_ctx_set_stream): not owned
    bool collectStats = false;
    bool textureLodUsed = false; // a pass has asked for HR_TEXTURE_LOD_CONE (kernel variant, see LaunchCfg)
    bool allLightsUsed = false;  // a pass has asked for HR_ESTIMATOR_ALL_LIGHTS: pass slots hold two occlusion rays per path and a second partial sum
    int rank = 0, world = 1, tile = 32;
    int numCUs = 256;
    std::string err;

    // frame
    int W = 0, H = 0;
    DeviceBuf<float> fbInternal;
    float *fbExternal = nullptr; // the caller's memory (hr_frame_bind_external): not owned
    PinnedBuf<float> pinned; // hr_readback's host buffer
    Event evPack; // made by the first call that needs it; orders hr_frame_pack_owned on a foreign stream against the resolves on the ctx stream
    Event evCopyOut; // made by the first call that needs it; orders a post-process feature's copy out on a foreign stream against the ctx stream (copyOutOnStream)
    DeviceBuf<char> dDisplay; // display resolve: device staging + pinned host copy, grown together (growDisplay)
    PinnedBuf<char> pinnedDisplay;
    // Progressive snapshots are handed out one call late from rotating buffers: the host then waits for a copy enqueued a
    // whole call ago instead of for everything it has just enqueued, so the GPU always has the next step queued
    // (waiting for the latest copy cost 0.8 ms of idle GPU per pass).
    struct Lagged {
        PinnedBuf<char> pinned[3];
        DeviceBuf<char> dev[3]; // device staging (display snapshots only)
        Event ev[3];
        uint32_t passes[3] = {0, 0, 0};
        unsigned long long epoch[3] = {0, 0, 0};
        int32_t format[3] = {-1, -1, -1};
        bool pending[3] = {false, false, false};
        size_t bytes = 0;
        int turn = 0;
    };
    Lagged progFrame, progDisplay;
    unsigned long long snapshotEpoch = 1; // bumped by clear / resize / bind: older snapshots are not handed out any more
    FrameDev frame{};
    unsigned long long frameZeroedAt = 0; // value of nextResolveOrder when the frame was last zeroed (hr_clear, hr_frame_resize): the AOV planes hold the frame's passes when aov.zeroedAt equals it
    uint32_t queueCapacity = 0;
    // Pipeline of in-flight passes (hr_trace.hip header): every slot owns the queues, hit records, counters and
    // the pass buffer of one pass.
    struct PassSlot {
        bool allocated = false, active = false;
        bool finished = false;   // every stage has been enqueued; the slot is held until its turn to resolve comes
        bool everResolved = false;
        unsigned long long resolvedAt = 0; // value of nextResolveOrder when this slot's last pass was resolved
        int group = 0;           // pipeline group (worker stream) the pass runs on
        Event evFinal;    // recorded on the worker stream after the pass's last stage
        Event evResolved; // recorded on the caller's stream after the pass buffer was added to the frame
        // Passes that finish in one macro step, and passes one k_resolve launch adds, share ONE recorded event (a record or a wait is a
        // packet of ~4-8 us on its stream: twelve of each per batch delayed the resolve of a batch by 0.1 ms and its next injection by as
        // much).  The slot that owns the recorded event may be reused later; whoever waits has enqueued the wait before that (same call).
        hipEvent_t finalEv = nullptr;    // the event to wait on for this pass's last stage (some slot's evFinal: not owned)
        hipEvent_t resolvedEv = nullptr; // ... for the launch that added this pass buffer to the frame (some slot's evResolved: not owned)
        int step = 0, nIter = 0;
        unsigned long long order = 0; // injection order (passes resolve in this order)
        hr_pass_params pp{};
        // The pass's rays live in its group's step arenas (Group::arena): what its last step's shading emitted, i.e. what its next
        // step traces.  Only the pass buffer belongs to the slot.
        RayQueue qcur{};       // closest-hit rays of the pass's next stage
        ShadowQueue scur{};    // occlusion rays of the pass's next stage
        uint32_t capCur = 0;   // rays qcur can hold (= upper bound of what it holds)
        uint32_t sCapCur = 0;  // occlusion rays scur can hold
        DeviceBuf<float> passbuf;
        float *passbufB = nullptr; // second partial sum (allLightsUsed): passbuf + W * H * 4, same allocation (not owned)
        float *aov = nullptr;      // HR_AOV_SURFACE: the pass's AOV record (two float4 per pixel) behind the partial sums, same allocation (not owned)
        Counters *ctr = nullptr;   // this slot's entry of dCounters (not owned)
    };
    PassSlot slots[kMaxSlots];
    int nSlotsAllocated = 0;
    int maxSlots = kMaxSlots; // bounded by device memory at resize
    // Pipeline groups: independent pass pipelines on their own HIP streams, stepped alternately, so that the tail of one
    // group's persistent trace kernel (waves running dry) is back-filled by the other group's kernels.  Resolves run on
    // the caller's stream, strictly in pass order.
    struct Group {
        Stream stream;
        DeviceBuf<StepTable> dTables;   // ring of device step tables
        PinnedBuf<StepTable> hTables;   // pinned staging ring
        StepTable *dTablesHost = nullptr; // ... as the device addresses it (not owned)
        Event tableCopied[4];
        bool tableUsed[4] = {false, false, false, false};
        unsigned long long stepCounter = 0;
        Event evUser;    // caller-stream state this group has to wait for
        bool needUserSync = true;
        // Pass-through scenes (single-sided / alpha-masked materials): a pass has no fixed number of stages, so after every
        // macro step the closest-queue lengths of all pass slots are copied to a pinned ring; the host reads the copy of TWO
        // steps ago (a step that has long finished while newer ones are still queued: it never waits for work it has just
        // enqueued) and retires the passes whose queue ran empty.
        PinnedBuf<uint32_t> hQCount;    // [kStatusRing][kMaxSlots][kMaxBounceSlots], pinned
        // Ray memory of the group (round 4).  A pass used to own two ray queues, an occlusion queue, hit records and a hit list, all
        // sized for EVERY owned pixel, for its whole life: 196 B x pixels x 120 slots = 53 GB for a 1080p render, while a pass past
        // its first bounce holds a few percent of the pixels.  Now every macro step carves what it needs out of three regions:
        //   arena[t & 1]  what step t's shading emits (closest-hit and occlusion rays of every in-flight pass), read by step t + 1;
        //   scratch       what lives inside one step: the injected passes' camera rays, hit records, hit lists.
        // A queue is sized by an upper bound of what can arrive in it: a ray emits at most one continuation ray and kS occlusion rays,
        // so the bound is the length of the pass's closest-hit queue ONE stage earlier — which k_trace itself reports: its first
        // workgroup writes, when it starts, the queue lengths of its step table to pinned host memory and then the step's number
        // (hCounts / hSeq; no packet on the stream).  Preparing step t the host waits for step t - 1's report (by then step t - 2 has
        // finished and all of step t - 1 is still queued: the device never runs dry); only a pass's FIRST stage is sized by pixels.
        // Regions grow on demand (a synchronisation of the group's stream, during the first passes of a render).
        struct Region {
            DeviceBuf<char> base;
            size_t cap = 0; // bytes handed out of `base` (growRegion may get more than it asked for)
        };
        Region arena[2], scratch;
        size_t arenaHighWater = 0; // most either half ever needed: both halves are kept that large (consecutive steps see the same load)
        PinnedBuf<uint32_t> hCounts;                   // [kTableRing][kMaxSegs], pinned: closest-hit queue length per table entry
        PinnedBuf<volatile unsigned long long> hSeq;   // [kTableRing], pinned: step number + 1 whose lengths the entry holds
        uint32_t *dCounts = nullptr;                   // the same two arrays as the device addresses them (not owned)
        unsigned long long *dSeq = nullptr;
        Stream streamB;                                // HR_TUNE corun=1: the fused packet kernel of a step runs here, beside k_trace (experiment)
        Event evFork, evJoin;
        PinnedBuf<volatile unsigned long long> hProbe; // [kTableRing][8] (five used), pinned: the packet probe's totals as of that step's k_trace (packet selector below)
        unsigned long long *dProbeHost = nullptr;      // ... as the device addresses it (not owned)
        int countN[4] = {0, 0, 0, 0};                  // entries of the step table that went with ring entry r
        int countSlot[4][HR_MAX_SEGS];                 // ... their pass slots
        unsigned long long countOrder[4][HR_MAX_SEGS]; // ... and passes (order + 1)
        Event statusEv[4];
        bool statusUsed[4] = {false, false, false, false};
        unsigned long long statusOrder[4][2 * HR_MAX_SEGS]; // pass (order + 1) a slot held when the snapshot was taken, 0 = none
    };
    Group groups[kMaxGroups];
    int nGroups = 2;      // groups in use: chosen per frame size in hr_frame_resize unless HR_TUNE fixes it
    int traceBlocks = 5;  // k_trace's workgroups per CU: tune.blocks where HR_TUNE gives it, else chosen with nGroups
    int nextGroup = 0;
    unsigned long long nextResolveOrder = 0;
    unsigned long long resolvedAtClear = 0; // value of nextResolveOrder at the last hr_clear
    // Passes requested but not yet injected: when a shard is small (multi-GPU tiles, small frames) several passes are
    // injected per macro step so that every launch still carries about a full 1080p pass worth of rays.
    std::deque<hr_pass_params> pendingInject;
    unsigned long long oldestWaitingNs = 0; // steady-clock time of the oldest pass request not yet completed by a drain (0: none)
    int injectBatch = 1;
    int lastDepth = -1;
    unsigned long long injected = 0;
    DeviceBuf<uint32_t> dZero;    // a zero word (occlusion count of a pass's first step)
    DeviceBuf<Counters> dCounters; // one per pass slot, contiguous (copied to the host in one piece in pass-through scenes)
    DeviceBuf<unsigned long long> dStepLog; // kStepLogCap records of three words (StepTable::stepLog)
    // Sticky report of a ray queue that turned out longer than its capacity (hr_wave.h: queueOverflow): four pinned, coherent words
    // the kernels write — kind of queue, step, table entry, count.  Checked wherever the caller learns about finished work.
    PinnedBuf<volatile uint32_t> hOverflow;
    uint32_t *dOverflowHost = nullptr; // ... as the device addresses them (not owned)
    // hr_ctx_desc::memory_budget: device bytes the pipeline may hold for rays and pass buffers (0: unlimited).  Bounds the passes
    // injected per step (budgetBatch): first by what a batch needs when every queue is as long as it can get, then — once a full
    // pipeline has shown the real lengths — by what it was seen to need (rayBytesSeen / batchSeen), with a fifth on top.
    unsigned long long memBudget = 0;
    // ray memory a pass needs at stage s of its life — what a step carves for it in the arena / in scratch —, the largest per-pass average
    // seen so far (not seen since the last resize / commit: the stage counts as long as it can possibly get, budgetBytesPerPass)
    struct BudgetSeen {
        double stageArenaSeen[kMaxBounceSlots] = {0}, stageScratchSeen[kMaxBounceSlots] = {0};
        bool stageSeen[kMaxBounceSlots] = {false};
        void forget() { std::memset(stageSeen, 0, sizeof(stageSeen)); } // back to the guarantee until the stages have been seen again
        void record(int st, double arena, double scratch)
        {
            stageArenaSeen[st] = (stageSeen[st] && stageArenaSeen[st] > arena) ? stageArenaSeen[st] : arena;
            stageScratchSeen[st] = (stageSeen[st] && stageScratchSeen[st] > scratch) ? stageScratchSeen[st] : scratch;
            stageSeen[st] = true;
        }
    };
    BudgetSeen budgetSeen;

    // Mesh blocks come out of an arena of 64 MB chunks (bump allocation inside a chunk): a hipMalloc per submesh is a device-wide
    // synchronisation of ~0.1 ms each, which adds up for the scenes the reference loads (hundreds of submeshes).  A chunk whose last
    // mesh has been removed is empty again: one such chunk is kept for the next add (a lone dynamic mesh that is removed and re-added
    // every frame costs no hipFree + hipMalloc), further ones are released, and their entries in the vector are reused.
    struct MeshChunk {
        DeviceBuf<char> base; // (its capacity: the chunk's bytes)
        size_t used = 0;
        int live = 0;
    };
    std::vector<MeshChunk> meshChunks;
    char *meshAlloc(size_t bytes, int *chunkOut)
    {
        const size_t need = (bytes + 255) & ~(size_t)255;
        // the newest chunk first (it is the one being filled), then any other with room (e.g. one that ran empty)
        for (int i = (int)meshChunks.size() - 1; i >= 0; --i) {
            MeshChunk &k = meshChunks[i];
            if (k.base && k.base.capacity() - k.used >= need) {
                char *p = k.base + k.used;
                k.used += need, k.live += 1;
                *chunkOut = i;
                return p;
            }
        }
        MeshChunk k;
        if (k.base.alloc(need > ((size_t)64 << 20) ? need : ((size_t)64 << 20)) != hipSuccess) return nullptr;
        k.used = need, k.live = 1;
        char *const p = k.base;
        for (size_t i = 0; i < meshChunks.size(); ++i)
            if (!meshChunks[i].base) { // a released chunk's entry (other meshes refer to chunks by index, so entries never move)
                meshChunks[i] = std::move(k);
                *chunkOut = (int)i;
                return p;
            }
        meshChunks.push_back(std::move(k));
        *chunkOut = (int)meshChunks.size() - 1;
        return p;
    }
    void meshRelease(int chunk)
    {
        if (chunk < 0 || chunk >= (int)meshChunks.size()) return;
        MeshChunk &k = meshChunks[chunk];
        if (!k.base || --k.live > 0) return;
        k.live = 0, k.used = 0; // empty: its space is handed out again
        int spare = 0;
        for (const MeshChunk &o : meshChunks) spare += (o.base && o.live == 0) ? 1 : 0;
        if (spare > 1 || k.base.capacity() > ((size_t)64 << 20)) k.base.reset(); // keep ONE empty default-sized chunk
    }
    void meshReleaseAll() { meshChunks.clear(); }
    // scene (host mirror)
    std::vector<Geom> geoms;
    std::vector<Texture> textures;
    std::vector<hr_material> materials;
    hr_lights lights{};
    int32_t blockNx = 0, blockNy = 0, blockCoords[32] = {0};
    // importance table of the environment map (HR_ESTIMATOR_ENV_MIS), built on the device when a pass first asks for it
    DeviceBuf<float> dEnvRowCdf, dEnvColCdf, dEnvProb;
    DeviceBuf<uint16_t> dEnvRowGuide, dEnvColGuide;
    int envW = 0, envH = 0, envTex = -2;
    float envMeanLum = 0.0f;
    bool committed = false, sceneDirty = true, hasPassthrough = false;
    bool hasGlass = false; // some material is glass (decides whether the glass shading kernel is launched)
    // What changed since the last commit decides what a commit does: a change of the set of geometries rebuilds the tree, a
    // change of transforms only (Scene::applyTransform while the user drags a slider) REFITS it — same topology, every box
    // recomputed bottom-up on the device, no allocation, one synchronisation at the end.
    bool topologyDirty = true, transformDirty = false;
    // pipeline diagnostics (HR_DEBUG_PIPE=1 prints them when the context is destroyed)
    unsigned long long dbgGrowths = 0, dbgGrowBytes = 0, dbgWaits = 0, dbgWaitNs = 0, dbgWaitSpun = 0;
    // ---- packet selector.  The camera rays of the passes injected together can be traced one ray per lane by k_trace, or 64 at a time as a
    // packet by k_raygen_packets (hr_raygen.hip): 2^k passes of 64 >> k neighbouring pixels per wave.  The packet walks the UNION of its
    // rays' node sets: it wins where that union is small against the sum — meshes, and since a pixel's rays in consecutive passes differ by
    // the jitter only, even the benchmark's triangle fog at 16 passes per packet (1.8 x; one pass of an 8x8 patch: 3.0 x, which loses).
    // Which it is depends on scene, camera and resolution, so it is measured: every kProbeEvery-th injecting step — and the first after a
    // commit, a resize or a change of camera — a probe kernel on a side stream makes the camera rays of every 32nd group of pixels of
    // one injected pass and its companions itself and walks them as packets of the shape in use, writing nothing but
    //     U = (children the packet entered x its rays) / (children the rays' own box tests entered)
    // and how many child boxes a ray enters.  Packets are used while U < tune.punion / 100 (profiles/r4u_packets.txt).  The totals come back
    // with the queue lengths k_trace reports (no synchronisation).  Either way the hits are the same bits (tune.packets = 0 | 1 pins the mode).
    // The packet kernel is VALU-bound and leaves the texture addressers idle (busy 1.0 / 0.16); k_trace without the camera rays is the
    // other way round (0.70 / 0.94).  So a step's packet kernel runs BESIDE its k_trace, on a second stream (fork after the table copy,
    // join before the shading kernels), and k_trace leaves it room: 3 workgroups per CU instead of 5 when the camera rays are a good part
    // of the step's work, 4 when they are little (a step that injects few passes beside many in flight); c3 2100 -> 2390 Mrays/s at 128
    // passes, 2025 -> 2150 at 20 (profiles/r4v_corun.txt).
    // Only where k_trace IS bound by the addressers, i.e. where rays walk far: the probe also reports how many child boxes a camera ray
    // enters (c3 76, c5 75, c3d 162: +8..13 %; c2 35: no difference; terrain 10, c1 5: k_trace is VALU-bound itself there and loses 6 %): tune.corun, tune.cmin.
    // The packet kernel tests a node's child boxes ONCE per packet against the packet's bounds (the interval step, hr_packet_interval.h,
    // DESIGN §2) instead of once per ray.  That walk enters a superset of the children; how much more is the scene's and the camera's:
    // the selector's probe walks both ways and reports F = children entered by the interval step / by the per-ray step (c3 1.05,
    // c3d 1.02, c2 1.01: +3..7 %; terrain 1.2, its short walks mostly leaves, where every extra child is a triangle test: -3.7 %): tune.pstep, tune.pstepf.
    struct PacketSelector {
        static const int kProbeEvery = 64; // injecting steps between two probes
        double lastLooseness = 0.0; // F of the last probe (0: none has reported)
        bool packetsOn = false;
        uint32_t lastCameraCount = 0; // camera rays per pass behind the root cull, as last reported
        int probeCountdown = 0;              // injecting steps until the next probe
        bool probePending = false;
        unsigned long long probeStep = 0;    // step (of group 0) that carried the pending probe
        unsigned long long probeSeen[5] = {0, 0, 0, 0, 0}; // totals of the report the last decision was taken on
        double lastOwnPerRay = 0.0;         // child boxes a probed camera ray entered: how long the scene's traversals are
        unsigned long long probeWaves = 0;   // waves of the pending probe: it is complete when the third total has grown by as many
        double lastUnion = 0.0;              // U of the last probe (HR_DEBUG_PIPE prints it)
        float probeCamera[21] = {0};         // fov, aspect, focus distance, aperture, view matrix, interactive mode of the probed pass
        DeviceBuf<unsigned long long> dProbe; // five device counters (of eight words) the probe launches add to (never reset)
        Stream probeStream;                  // the probe runs beside the pipeline: it makes its own camera rays and writes only the counters
        Event evProbeA, evProbeB; // scene and tables as the group's stream sees them -> probe may start; probe done
        bool probeGuard = false;             // evProbeB has not been waited for yet (drainPipeline does: the scene may change afterwards)

        void sceneOrSizeChanged() { probeCountdown = 0; } // another tree, another resolution: the next injecting step probes
        bool useIntervalStep(const Tune &tune) const { return tune.pstep != 0 && (tune.pstepf <= 0 || lastLooseness == 0.0 || lastLooseness * 100.0 < (double)tune.pstepf); }
        bool packetsInUse(const Tune &tune) const { return tune.packets == 1 || (tune.packets == 2 && packetsOn); }
        // Passes injected together when their camera rays travel as packets: a wave holds 2^k passes of 64 >> k pixels (hr_raygen.hip:
        // k_raygen_packets), so the batch is the power of two next to the usual one (12 -> 16, 3 -> 4, 5 -> 4), sixteen per launch at most.
        static int packetBatch(int injectBatch)
        {
            const int b = injectBatch < 1 ? 1 : injectBatch;
            int up = 1;
            while (up < b) up <<= 1;
            return (4 * b >= 3 * up) ? up : up / 2;
        }
        static int packetLog2(int injectBatch)
        {
            int k = 0;
            while ((2 << k) <= packetBatch(injectBatch) && k < 4) ++k;
            return k;
        }
        // The pending probe's totals as group 0's step `stepIdx` found them with the queue lengths (Group::hProbe; steps from the probe's own on
        // report them): complete once every wave of the probe has counted itself, and then the decision for the steps that follow.
        void takeReport(const volatile unsigned long long *totals, unsigned long long stepIdx, const Tune &tune)
        {
            if (!probePending || stepIdx <= probeStep) return;
            const unsigned long long pk = totals[0], ry = totals[1], done = totals[2], nr = totals[3], iv = totals[4];
            if (done - probeSeen[2] < probeWaves) return;
            const unsigned long long dPk = pk - probeSeen[0], dRy = ry - probeSeen[1], dNr = nr - probeSeen[3], dIv = iv - probeSeen[4];
            probePending = false, probeSeen[0] = pk, probeSeen[1] = ry, probeSeen[2] = done, probeSeen[3] = nr, probeSeen[4] = iv;
            if (dPk > 0) lastLooseness = (double)dIv / (double)dPk; // F: children entered, interval step / per-ray step
            if (dRy > 0) {
                lastUnion = (double)dPk / (double)dRy;
                packetsOn = lastUnion * 100.0 < (double)tune.punion;
                lastOwnPerRay = dNr ? (double)dRy / (double)dNr : 0.0;
            }
            if (tune.debugPipe) fprintf(stderr, "packet probe of step %llu (seen at step %llu): union %.3f, %.1f child boxes entered per ray -> packets %s; interval step F %.3f -> %s\n", probeStep, stepIdx, lastUnion, lastOwnPerRay, packetsOn ? "on" : "off", lastLooseness, useIntervalStep(tune) ? "on" : "off");
        }
        // Does group 0's step that injects passes with these parameters carry a probe?  (Counts the step, remembers the probed camera.)
        bool wantsProbe(const hr_pass_params &pp, const Tune &tune)
        {
            if (tune.packets != 2 || probePending || pp.interactive_mode != 0) return false;
            float cam[21] = {pp.fov_tan, pp.aspect_ratio, pp.focus_distance, pp.aperture_radius};
            std::memcpy(cam + 4, pp.view_matrix, sizeof(pp.view_matrix));
            cam[20] = (float)pp.interactive_mode;
            // another camera sees another part of the tree: probe again, but not more often than every eighth injecting step (a camera in motion)
            if (std::memcmp(cam, probeCamera, sizeof(cam)) != 0 && probeCountdown > 0 && probeCountdown <= kProbeEvery - 8) probeCountdown = 0;
            if (probeCountdown > 0) {
                probeCountdown--;
                return false;
            }
            std::memcpy(probeCamera, cam, sizeof(cam));
            return true;
        }
    };
    PacketSelector selector;
    // persistent device arrays of the committed scene (grow-only: reserve; reused across commits)
    DeviceBuf<GeomDev> dG;
    DeviceBuf<Tri> trisPrim;  // prim-order triangles (input of a full build)
    BuildResult tree{};       // nodes, leaf-order triangles, node boxes, prim -> slot map, level ranges: raw, shared with the build unit; freeTree frees it
    uint32_t treeTris = 0;
    DeviceBuf<SceneConsts> dConsts;
    PinnedBuf<SceneConsts> hConsts;
    float builtAreaSum = 0.0f; // (sum of the node boxes' areas) / (sum of the triangles' areas) right after the last full build (refit quality reference)
    std::string cachePath;          // hr_scene_cache
    // pinned staging ring for mesh uploads
    PinnedBuf<char> stage[2];
    Event stageEv[2];
    bool stageBusy[2] = {false, false};
    int stageTurn = 0;
    hr_scene_info info{};
    hr_tree_info treeInfo{}; // include/hrcore_tree.h: of the last commit that built the tree

    // scene (device); nodes / tris alias tree.nodes / tree.tris (not owned)
    Node4 *nodes = nullptr;
    Tri *tris = nullptr;
    DeviceBuf<TriAttr> attrs;
    DeviceBuf<TriAttrExt> attrsExt;
    DeviceBuf<hr_material> dMaterials;
    DeviceBuf<TexDesc> dTextures;
    DeviceBuf<float> dTexDensity; // HR_TEXTURE_LOD_CONE: per-triangle level offset, rebuilt after every commit once the mode was used
    bool texDensityStale = true;
    DeviceBuf<float2> dSeq, dAperture, dSeqOffsets;
    int nSeq = 0, seqLen = 0, nSeqOffsets = 0;
    SceneDev hScene{};
    DeviceBuf<SceneDev> dScene;
    DeviceBuf<Stats> dStats;
    DeviceBuf<uint32_t> dScratch; // 8 words: ordered bounds etc.

    // optional per-kernel timing (HR_CTX_TIME_KERNELS)
    bool timeKernels = false;
    struct Timed {
        int kind;
        hipEvent_t e0, e1; // entries of timingEvents (not owned)
        bool e0Shared; // e0 is the e1 of the entry before (timeNext): one record between two kernels enqueued back to back
    };
    std::vector<Timed> pending;
    std::vector<Event> timingEvents;    // every event getEvent has made
    std::vector<hipEvent_t> eventPool;  // ... those of them not in `pending` (not owned)
    float kernelMs[HR_KERNEL_COUNT] = {0, 0, 0, 0};
    uint32_t kernelLaunches[HR_KERNEL_COUNT] = {0, 0, 0, 0};
    hipEvent_t getEvent()
    {
        if (eventPool.empty()) {
            timingEvents.emplace_back();
            timingEvents.back().create();
            return timingEvents.back();
        }
        const hipEvent_t e = eventPool.back();
        eventPool.pop_back();
        return e;
    }
    void timeBegin(int kind, hipStream_t st)
    {
        if (!timeKernels) return;
        Timed t{kind, getEvent(), getEvent(), false};
        hipEventRecord(t.e0, st);
        pending.push_back(t);
    }
    // The kernel timed last ends and the next one begins at ONE event (a record is a packet of several microseconds between the two)
    void timeNext(int kind, hipStream_t st)
    {
        if (!timeKernels) return;
        const hipEvent_t mid = pending.back().e1;
        hipEventRecord(mid, st);
        pending.push_back(Timed{kind, mid, getEvent(), true});
    }
    void timeEnd(hipStream_t st)
    {
        if (!timeKernels) return;
        hipEventRecord(pending.back().e1, st);
    }
    void drainTimes()
    {
        if (pending.empty()) return;
        for (int g = 0; g < kMaxGroups; ++g)
            if (groups[g].stream) hipStreamSynchronize(groups[g].stream);
        hipStreamSynchronize(stream);
        for (Timed &t : pending) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, t.e0, t.e1) == hipSuccess) {
                kernelMs[t.kind] += ms;
                kernelLaunches[t.kind] += 1;
            }
            if (!t.e0Shared) eventPool.push_back(t.e0);
            eventPool.push_back(t.e1);
        }
        pending.clear();
    }

    float *fb() const { return fbExternal ? fbExternal : fbInternal; }
    Tune tune; // the HR_TUNE knobs (hr_tune.h), parsed by hr_ctx_create and never written afterwards
    // The optional post-process features (hr_features.h).  When each one's state goes: featuresPlanesGone, featuresFrameResized,
    // featuresFrameCleared and featuresDestroyed in hr_postprocess.inl.
    AovState aov;
    DenoiseState denoise;
    AdaptiveState adaptive;
    HistoryState history;
    ReprojectState reproject;
    ExposureState exposure;
    MetricState metric;
    DespeckleState despeckle;
    MeshPrepState meshPrep;
    DeformState deform;
    QueryState query;
    MotionState motion;
    // Context group (include/hrcore_group.h): non-null when this handle is a group.  Its own fields then describe the ASSEMBLED frame on the
    // group's first device (W, H, frame, fbInternal, the read-back buffers) and `stream` is the assembly stream; no pass pipeline runs on it.
    GroupState *grp = nullptr;
    LaunchCfg cfg(hipStream_t st) const
    {
        return LaunchCfg{st, numCUs, traceBlocks, tune.sblocks, collectStats, textureLodUsed, allLightsUsed, hasGlass, tune.pswz, selector.useIntervalStep(tune) ? 1 : 0, (aov.mask & HR_AOV_SURFACE) != 0};
    }
};

#define FAIL(ctx, code, msg)  \
    do {                      \
        (ctx)->err = (msg);   \
        return (code);        \
    } while (0)

#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
            return HR_ERR_DEVICE;                                                                 \
        }                                                                                         \
    } while (0)

#define ENTER(ctx)                                   \
    if (!(ctx)) return HR_ERR_INVALID;               \
    HIP_TRY(ctx, hipSetDevice((ctx)->device))


// a read-back's pinned staging: at least `needBytes`, grow-only (a shrinking frame keeps its buffer); reports through the context
template <class T> inline int growPinned(hr_ctx *c, PinnedBuf<T> &b, size_t needBytes)
{
    HIP_TRY(c, b.reserve((needBytes + sizeof(T) - 1) / sizeof(T)));
    return HR_OK;
}
