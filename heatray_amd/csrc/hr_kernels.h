// hr_kernels.h — host-visible declarations of the kernel launchers (the render stages hr_frame.hip, hr_raygen.hip, hr_trace.hip and hr_shade.hip; hr_build.hip and hr_tables.hip; the post-process units).
#pragma once

#include "hr_types.h"
#include "../../include/hrcore_group.h"
#include "../../include/hrcore_aov.h"
#include "../../include/hrcore_denoise.h"
#include "../../include/hrcore_denoise_spatial.h"
#include "../../include/hrcore_adaptive.h"
#include "../../include/hrcore_history.h"
#include "../../include/hrcore_reproject.h"
#include "../../include/hrcore_tree.h"
#include "../../include/hrcore_exposure.h"
#include "../../include/hrcore_metric.h"
#include "../../include/hrcore_despeckle.h"
#include "../../include/hrcore_mesh.h"
#include "../../include/hrcore_deform.h"
#include "../../include/hrcore_query.h"
#include "../../include/hrcore_motion.h"

#include <cstddef>

namespace hr {

struct FrameDev {
    float *fb; // RGBA32F accumulation buffer, row 0 = bottom
    int32_t W, H;
    int32_t rank, world, tile, tilesX, tilesY, nOwnedTiles;
    const uint32_t *mask; // the sample mask in force (include/hrcore_adaptive.h): row-major words, (W + 31) / 32 per row, bit (x & 31) of word (x >> 5) = pixel x; null: every pixel is sampled
};

struct HitRec; // hr_trace.h

// Device counters are kept in kStatSlots copies (a workgroup adds to slot blockIdx.x % kStatSlots) so that the adds of a
// launch spread over many addresses instead of serialising on one; hr_get_stats sums the copies.
static const int kStatSlots = 4096;
struct Stats {
    unsigned long long paths, raysClosest, raysAny, shadedHits, accumulates, nodeVisits, triTests, nodeVisitsAny, triTestsAny;
    unsigned long long traceTicks, traceLaunches; // k_trace by the 100 MHz device clock: first workgroup's start to last workgroup's end, summed over launches
};

struct LaunchCfg {
    hipStream_t stream;
    int numCUs;
    int traceBlocksPerCU;
    int shadeBlocksPerCU;
    bool collectStats;
    bool textureLod; // some pass has asked for HR_TEXTURE_LOD_CONE: launch the shading kernel that carries the trilinear sampler
    bool allLights;  // some pass has asked for HR_ESTIMATOR_ALL_LIGHTS: the shading kernel that can emit two occlusion rays per vertex
    bool hasGlass;   // some material of the scene is glass: the glass shading kernel is launched too
    int packetSwizzle = 0; // k_raygen_packets deals whole 32x32 tiles to the XCDs instead of consecutive 16-pixel patches (HR_TUNE pswz)
    int packetStep = 1;    // k_raygen_packets tests a node's children once per packet against the packet's bounds (hr_ctx::PacketSelector::useIntervalStep; hr_packet_interval.h)
    bool aovSurface = false; // HR_AOV_SURFACE is enabled: launch the shading kernel that records the first visible surface (include/hrcore_aov.h)
    bool packetLens = false; // (LAST: hr_ctx::cfg fills the fields above by position)  a pass injected this step has a lens: k_raygen_packets_rays<.., false>, and SegDev::listed stays 0 (hr_pipeline.inl)
};

// One in-flight pass as seen by the kernels of one macro step.
struct SegDev {
    RayQueue qin;        // closest-hit rays traced and shaded this step
    RayQueue qout;       // closest-hit rays emitted for the next step
    ShadowQueue sqIn;    // occlusion rays traced this step (emitted by the previous step's shade)
    ShadowQueue sqOut;   // occlusion rays this step's shade emits (traced by the next step)
    HitRec *hits;        // closest-hit records of qin
    float *passbuf;      // RGBA32F sample of this pass (full-frame indexing)
    float *passbufB;     // HR_ESTIMATOR_ALL_LIGHTS: the sample's second partial sum (analytic-light contributions), or null
    uint32_t *qCountIn;  // number of rays in qin
    uint32_t *sCountIn;  // number of occlusion rays to trace this step
    uint32_t *qCountOut; // counter shade appends qout with
    uint32_t *sCountOut; // counter shade appends sq with
    uint32_t *hitIdx;    // hit list of this step: indices into qin of the rays that hit a PBR material from the front, a glass material from the back
    uint32_t *pCount;    // entries at the front of hitIdx (k_shade_sort appends, k_shade_hit<.., 0> reads)
    uint32_t *gCount;    // entries at the back of hitIdx
    uint32_t hitCap;     // capacity of hitIdx (= of the ray queues)
    uint32_t packets;    // the entry's closest-hit queue (camera rays) is filled AND traced by k_raygen_packets this step: k_trace leaves it out; 2: that kernel runs beside k_trace (the queue's length is not final when k_trace starts)
    hr_pass_params pp;   // per-pass uniforms
    int32_t closestEnabled; // 0 in a pass's last step (only its occlusion rays remain)
    // Capacities of the queues beside hitCap (which also bounds hits / hitIdx / qout): every append compares its slot with them and every
    // reader clamps the counter it reads — a bound that turns out wrong drops rays and raises StepTable::hostOverflow instead of
    // writing past an arena (hr_wave.h: queueOverflow)
    uint32_t qinCap;  // rays qin can hold
    uint32_t sInCap;  // occlusion rays sqIn can hold
    uint32_t sOutCap; // occlusion rays sqOut can hold
    float *aov;       // HR_AOV_SURFACE: the pass's AOV record, two float4 per pixel (albedo + hit, normal + depth; full-frame indexing), or null
    uint32_t listed;  // the packet kernel lists this entry's hits itself: k_shade_sort leaves the entry out
};

#ifndef HR_MAX_SEGS
#define HR_MAX_SEGS 320
#endif
static const int kMaxSegs = HR_MAX_SEGS;
static const int kClkSlots = 16;
static const int kStepLogCap = 4096; // macro steps the step log keeps (a ring)
static const int kTraceHeadsMax = 64; // in-flight passes of one group: (passes injected per macro step) x (stages per pass)
struct StepTable {
    // read-mostly header: every wave of every kernel of the step reads it once
    int32_t nSeg;
    int32_t refillLanes;   // refill a wave from the work pool once this many lanes are idle
    int32_t triPhaseLanes; // run the triangle phase once this many lanes are blocked on a postponed leaf
    int32_t fetchMax;      // work items a wave reserves per global atomic while plenty of work is left ...
    int32_t fetchMin;      // ... shrinking to this near the end of the pool (guided self-scheduling: short tail)
    int32_t staticPerWave; // launches of at most this many rays per resident wave are dealt out statically (k_trace)
    int32_t hasGlass;      // some material of the scene is glass (else the glass hit list is never appended to)
    int32_t primaryFromSeg;  // passes [primaryFromSeg, nSeg) were injected this step: their closest-hit queues hold camera rays
    int32_t fetchMaxPrimary; // chunk size of the work fetch inside that (coherent) part of the index space: low 16 bits; high 16 bits: how many such chunks per resident wave the part must hold for it to be used
    uint32_t headsLog2;      // 2^headsLog2 ranges are in use (HR_TUNE heads=)
    // k_trace's first workgroup reports the closest-hit queue length of every entry to pinned HOST memory when it starts, then the
    // step's number (hr_core.hip, Group::hCounts): how the host sizes the next steps' queues without a packet on the stream
    uint32_t *hostCounts;
    unsigned long long *hostSeq;
    unsigned long long seqValue;
    // log of the k_trace launches since the last hr_clear (hr_get_step_log): k_shade_sort appends (first start, last end) by the device clock
    unsigned long long *stepLog; // kStepLogCap x {start tick, end tick, passes in the table | group << 16 | passes injected << 32}
    uint32_t nInjectedNow;
    uint32_t group; // pipeline group the step belongs to (goes into its log record)
    // k_packet_probe adds (children a packet entered x its rays, child boxes the rays themselves entered, 1 per finished wave) to
    // probe[0..2]; k_trace's first workgroup copies the totals to pinned host memory with the queue lengths (hr_core.hip: the packet selector)
    unsigned long long *probe;
    unsigned long long *hostProbe;
    // Sticky overflow report (pinned host memory, four words: queue kind, the step's number, table entry, count seen): set by the first
    // append or read that finds a queue longer than its capacity; hr_flush / hr_readback / hr_synchronize turn it into HR_ERR_DEVICE
    uint32_t *hostOverflow;
    uint32_t *hostCameraCount; // pinned: camera rays per pass behind the root cull, as the step's shading kernel last saw them in queues a packet kernel filled (a hint for the host's scheduling, no ordering)
    // The work cursors of k_trace: the index space of a launch is cut into 2^headsLog2 equal ranges (32 by default, at most
    // kTraceHeadsMax), each with a cursor on a cache line of its own — none of them shares its 128-byte line with the header above
    // or with seg[] below, which every wave reads while the cursors are hammered by atomics.  ONE cursor serialises at ~12 ns per atomic:
    // a launch of 25 M camera rays in 64-ray chunks needs 390 k of them, 4.7 ms of a 10 ms launch.  A workgroup starts on range
    // (blockIdx mod the number of ranges) — workgroups are dealt to the 8 XCDs round robin, so with 32 ranges an XCD starts on four of
    // them — and moves on to the next range when its own is used up.  Zeroed on the host with every table upload.
    alignas(128) uint32_t heads[kTraceHeadsMax * 32];
    // k_trace times itself with the device's constant 100 MHz clock: every workgroup folds its start and end into one of kClkSlots
    // (min, max) pairs, and the step's next kernel (k_shade_sort) adds (max end - min start) to the Stats counters.  No event packets
    // on the stream (a record costs a dependent chain of small launches 4-8 us each).  Initialised with every table upload.
    alignas(128) unsigned long long clkStart[kClkSlots];
    unsigned long long clkEnd[kClkSlots];
    alignas(128) SegDev seg[kMaxSegs];
};
static_assert(offsetof(StepTable, heads) % 128 == 0 && offsetof(StepTable, seg) % 128 == 0, "k_trace's work cursors own their cache lines");

// ---- the render stages (what their units share on the device: hr_wave.h)
// Several passes per launch (a small shard injects / resolves a batch of passes per macro step: one launch instead of 8 + 8)
static const int kMaxBatch = 16;
struct SegList {
    int32_t n;
    int32_t seg[kMaxBatch]; // indices into StepTable::seg, one per blockIdx.y
};

// ---- hr_frame.hip
struct PassBufList {
    int32_t n;
    const float *buf[kMaxBatch]; // pass samples, added to the frame in this order
    const float *bufB[kMaxBatch]; // second partial sum of a pass sample (HR_ESTIMATOR_ALL_LIGHTS), or null
};
// the per-stage counters of the passes injected by one macro step, cleared with ONE launch (a hipMemsetAsync per pass is a fill kernel
// and a kernel boundary each: 12 of them delayed a step's ray generation by ~0.1 ms)
struct CounterList {
    int32_t n;
    Counters *ctr[kMaxBatch];
};
void launchZeroCounters(const LaunchCfg &cfg, const CounterList &list);
void launchFetchTable(hipStream_t stream, const void *hostMapped, void *dst, size_t bytes);
void launchResolve(const LaunchCfg &cfg, const FrameDev &fr, const PassBufList &bufs);
// AOVs (include/hrcore_aov.h): the frame's planes (null when not enabled) and each pass's AOV planes (null without HR_AOV_SURFACE), in
// the order of PassBufList.  The resolve that adds the passes to the frame folds them into the planes and zeroes the passes' planes.
struct AovList {
    float *albedo, *normalDepth, *moments;
    float *pass[kMaxBatch];
};
void launchResolveAov(const LaunchCfg &cfg, const FrameDev &fr, const PassBufList &bufs, const AovList &aov);
void launchPackOwned(const LaunchCfg &cfg, const FrameDev &fr, const float *frame, float *packed, int unpack, float *full);
// Context groups (hr_group.inl): the packed pixels of every member (rank m of world n, ownedPixel order) -> their places in the full
// frame, ONE launch for all members.  Member m's slots are padded to whole workgroups: its workgroups are
// [blockStart[m], blockStart[m + 1]) (blockStart[n] = the grid), so a workgroup belongs to one member.
struct GatherList {
    int32_t n;
    uint32_t blockStart[HR_GROUP_MAX_MEMBERS + 1];
    const float *packed[HR_GROUP_MAX_MEMBERS]; // device memory on the frame's device (null for a member that owns no tiles)
};
int gatherBlock(); // workgroup size of k_gather_members (slots per padded workgroup)
void launchGatherMembers(const LaunchCfg &cfg, const FrameDev &fr, const GatherList &list, float *full);
void launchDisplay(const LaunchCfg &cfg, const FrameDev &fr, const hr_display_params &P, int format, void *out);

// ---- hr_raygen.hip
void launchRaygen(const LaunchCfg &cfg, const SceneDev *S, const StepTable *tbl, const SegList &segs, const FrameDev &fr, Stats *stats);
void launchRaygenPackets(const LaunchCfg &cfg, const SceneDev *S, const Node4 *nodes, const Tri *tris, const StepTable *tbl, const SegList &segs,
                         const FrameDev &fr, Stats *stats, bool uniformParams); // segs.n: a power of two; uniformParams: the passes differ in sample_index only
int launchPacketProbe(hipStream_t stream, const SceneDev *S, const Node4 *nodes, const Tri *tris, const hr_pass_params &pp, int passesLog2, const FrameDev &fr,
                      unsigned long long *probe, bool intervalStep);

// ---- hr_trace.hip
void launchTrace(const LaunchCfg &cfg, const SceneDev *S, const int *leafKeys, const Node32 *nodes32, const Tri *tris, StepTable *tbl, Stats *stats);
void launchDebugTrace(const LaunchCfg &cfg, const SceneDev *S, int n, const float *o, const float *d, const float *tmax, const int *skip,
                      int anyHit, hr_hit *out);
size_t hitRecordSize();

// ---- hr_shade.hip
void launchShade(const LaunchCfg &cfg, const SceneDev *S, const StepTable *tbl, Stats *stats);

// ---- hr_denoise.hip (include/hrcore_denoise.h)
// the working planes of the denoiser, W x H each: cv = demodulated colour + variance (ping-pong), nd = unit normal + depth,
// ac = effective albedo + coverage (float4 each), grad = depth gradient (float)
struct DenoiseBufs {
    float *cv[2], *nd, *ac, *grad;
};
static const size_t kDenoiseBytesPerPixel = 4 * 16 + 4;
void launchDenoisePrepare(hipStream_t st, int W, int H, const float *frame, const float *albedo, const float *normalDepth, const float *moments, const DenoiseBufs &b);
// one iteration from cv[src] to cv[src ^ 1] or, with finalOut, to the remodulated image there; tiled: the LDS kernel where it exists for the step
bool denoiseTiledHasStep(int step);
void launchDenoiseAtrous(hipStream_t st, int W, int H, const DenoiseBufs &b, int src, int step, const hr_denoise_params &p, bool tiled, float *finalOut);
void launchDenoiseFinish(hipStream_t st, int W, int H, const DenoiseBufs &b, float *out); // (no iteration: cv[0] remodulated)

// ---- hr_denoise_spatial.hip (include/hrcore_denoise_spatial.h)
// after launchDenoisePrepare: cv[1] = cv[0] with the variance after the spatial estimate (the iterations then start from src = 1);
// frame: the frame the planes were prepared from (its alpha is n); result = {spatial, estimated, starved pixels}, zeroed by the caller
static const size_t kDenoiseSpatialResultWords = 3;
void launchDenoiseSpatial(hipStream_t st, int W, int H, const float *frame, const DenoiseBufs &b, const hr_denoise_params &p, const hr_denoise_spatial_params &sp,
                          unsigned long long *result);

// ---- hr_adaptive.hip (include/hrcore_adaptive.h)
size_t sampleMaskWords(int W, int H); // 32-bit words of a frame's sample mask (FrameDev::mask)
void launchAdaptiveError(hipStream_t st, int W, int H, const float *frame, const float *moments, const hr_adaptive_params &p, float *err);
// err -> the mask words and result = {unconverged pixels, active pixels, bits of the largest finite error, unused} (four words, zeroed by the caller)
static const size_t kAdaptiveResultWords = 4;
void launchAdaptiveMask(hipStream_t st, int W, int H, const float *err, const hr_adaptive_params &p, uint32_t *words, uint32_t *result);
void launchMaskPack(hipStream_t st, int W, int H, const uint8_t *bytes, uint32_t *words);   // W x H bytes (non-zero = sampled) -> words
void launchMaskUnpack(hipStream_t st, int W, int H, const uint32_t *words, uint8_t *bytes); // words -> W x H bytes, 0 / 1

// ---- hr_history.hip (include/hrcore_history.h)
struct HsCam;    // hr_history.h: the two cameras of a merge
struct HsParams; // ... and its parameters as the kernel takes them
static const size_t kHistoryBytesPerPixel = 3 * 16; // H0, H1, H2: three planes of W x H float4 one after the other
void launchHistoryCapture(hipStream_t st, int W, int H, const float *frame, const float *albedo, const float *normalDepth, const float *moments, float *hist);
// the history -> the frame and the planes of the view being rendered; result = {reused pixels, rejected pixels, samples taken over}, zeroed by the caller
static const size_t kHistoryResultWords = 3;
void launchHistoryMerge(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, float *frame, float *albedo, float *normalDepth, float *moments,
                        unsigned long long *result);

// ---- hr_reproject.hip (include/hrcore_reproject.h)
// the history -> the sampled pixels of the frame and the planes that the examined bits (rpExaminedWords 64-bit words, hr_reproject.h) do not
// mark yet; result = {reused pixels, rejected pixels, samples taken over, pending pixels, examined pixels}, zeroed by the caller
static const size_t kReprojectResultWords = 5;
void launchReprojectMerge(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, float *frame, float *albedo, float *normalDepth, float *moments,
                          unsigned long long *examined, unsigned long long *result);
// a one-sample image (W x H float4) of the frame's own means and, where it has none, the history's colour behind a neighbour's guide;
// result = {own pixels, previewed pixels, empty pixels} in the first three of kReprojectResultWords words, zeroed by the caller
void launchReprojectPreview(hipStream_t st, int W, int H, const HsCam &cam, const HsParams &P, const float *hist, const float *frame, const float *albedo,
                            const float *normalDepth, float *out, unsigned long long *result);

// ---- hr_exposure.hip (include/hrcore_exposure.h)
struct ExParams; // hr_exposure.h: the reduce's parameters as the kernel takes them
struct ExWindow; // ... and the metered rectangle
// image (W x H float4, accumulation format) -> words: kExWords of hr_exposure.h (the 256 bins, the four class counters, what the reduce
// writes), zeroed by the caller; state: two 32-bit words {there is an adaptation state, its scale's bits}, read and written by the reduce
void launchExposureMeter(hipStream_t st, int numCUs, int W, int H, const float *image, const ExWindow &win, const ExParams &P, unsigned long long *words, uint32_t *state);
// launchDisplay of the image whose rgb is multiplied by the scale word of `words`
void launchExposureDisplay(hipStream_t st, const FrameDev &fr, const hr_display_params &P, int format, const unsigned long long *words, void *out);

// ---- hr_metric.hip (include/hrcore_metric.h)
struct MtWindow; // hr_metric.h: the measured rectangle
// kind 0 (compare): image against other = the reference; kind 1 (estimate): image = the frame, other = its MOMENTS plane; all W x H float4
// -> words: kMtWords of hr_metric.h (the 256 bins of NUM, those of DEN, the four counters, the bits of max_abs), zeroed by the caller
void launchMetricAccumulate(hipStream_t st, int numCUs, int W, int H, int kind, const float *image, const float *other, const MtWindow &win, unsigned long long *words);

// ---- hr_despeckle.hip (include/hrcore_despeckle.h)
// frame and moments (W x H float4 each) -> out and, where not null, momentsOut: the despeckled pair; no output is an input;
// result: kDespeckleSlots copies of {valid, clamped, kept, starved, nonfinite pixels}, each copy on a 128-byte line of its own, zeroed by
// the caller: a workgroup adds to copy blockIdx.x % kDespeckleSlots and the host sums the copies.  (Every workgroup of a frame adds to
// `valid`, and atomics on ONE word serialise at about 12 ns each: with one copy the 8100 workgroups of a 1080p frame took 104 us whatever
// else the kernel did or left out, profiles/despeckle_time.txt.)
static const int kDespeckleCounters = 5, kDespeckleSlots = 64, kDespeckleSlotStride = 16;
static const size_t kDespeckleResultWords = (size_t)kDespeckleSlots * kDespeckleSlotStride;
void launchDespeckle(hipStream_t st, int W, int H, const float *frame, const float *moments, const hr_despeckle_params &p, float *out, float *momentsOut,
                     unsigned long long *result);

// ---- hr_mesh.hip (include/hrcore_mesh.h)
// What one hr_mesh_prepare holds on the device, cut out of the context's scratch by hr_mesh.inl.  V vertices, T triangles, C = 3 T
// corners.  The four sort arrays hold max(C, V) words each (the corner sort, then the weld's sorts), blockHist 256 words per sort tile.
struct MsBufs {
    const float *pos, *uv, *nrmIn; // tightly packed: 3, 2, 3 floats per vertex (uv / nrmIn null unless read)
    const uint32_t *idx;
    uint32_t V, T, C;
    int32_t strip, weight, weld, want;
    uint8_t *tflag;                // per triangle: MS_FACE | MS_UV
    float *cN, *cT, *cB;           // per corner: the contributions (cT, cB with tangents only)
    uint32_t *keysA, *keysB, *valsA, *valsB, *blockHist;
    uint32_t *vBegin, *vEnd, *vFirst; // per vertex: its range in the sorted corners, its lowest non-degenerate corner
    float *vS, *vTa, *vBa;            // per vertex: the sums
    uint32_t *perm, *groupOf, *groupStart, *scan, *nGroups; // the weld: sorted vertex ids, vertex -> group, group -> first place in perm (V + 1), the heads' scan, one word
    float *gN;                     // per group: the normal
    uint8_t *gClass;               // ... and MS_NORMAL / MS_CANCELLED / MS_UNREFERENCED
    float *outN, *outT, *outB;     // per vertex: the outputs, 3 floats each
    unsigned long long *counters;  // kMsCounterWords, zeroed by the caller
};
enum { kMsDegenerate = 0, kMsDegenerateUv = 1, kMsUnreferenced = 2, kMsCancelled = 3, kMsFallback = 4, kMsMaxValence = 5, kMsGroups = 6 };
static const size_t kMsCounterWords = 8;
size_t meshSortBlocks(size_t n); // sort tiles of n keys
void launchMeshPrepare(hipStream_t st, const MsBufs &b);

// ---- hr_deform.hip (include/hrcore_deform.h)
// Up to four attributes of V vertices between a mesh block (`strided`: `stride` floats from vertex to vertex) and tight arrays (`comps`
// floats per vertex, 2 or 3): gather reads the strided side, scatter writes it.
struct DfCopy {
    float *strided[4], *tight[4];
    int32_t stride[4], comps[4];
    int32_t n; // attributes in use
    uint32_t V;
};
// One hr_deform_pose: the binding's tight arrays in, tight arrays out.  restT / restB null: the mesh has no tangent frames.  dN null:
// normals are not morphed.  pose: HR_DEFORM_MAX_MORPH morph weights, then nJoints x 16 matrix words.  outN / outT / outB null: not
// written (outT and outB go together).  counters: {rejected vertices, kept directions}, zeroed by the caller.
struct DfPoseArgs {
    const float *restP, *restN, *restT, *restB, *dP, *dN, *weights, *pose;
    const uint32_t *joints;
    float *outP, *outN, *outT, *outB;
    uint32_t V;
    int32_t nMorph, nJoints;
    unsigned long long *counters;
};
static const size_t kDfCounterWords = 2;
void launchDeformGather(hipStream_t st, const DfCopy &s);
void launchDeformScatter(hipStream_t st, const DfCopy &s);
void launchDeformPose(hipStream_t st, const DfPoseArgs &s);

// ---- hr_query.hip (include/hrcore_query.h)
// first triangle (prim id) of a committed mesh -> its hr_geom_id, in the order of the commit's GeomDev list (triOffset ascending)
struct QyGeom {
    uint32_t triOffset;
    int32_t id;
};
// One launch of ray queries; every pointer is device memory.  Rays are addressed in BYTES through the strides (never 0 here: the host
// has put in the tight ones); tmax / skip null: none.  hits / surfaces: either may be null.  slotOfPrim null: `tris` is in prim order.
// counters: kQySlots copies of one word (hits | invalid << 32), each on a 128-byte line of its own, zeroed by the caller: a wave adds to
// copy blockIdx.x % kQySlots with ONE atomic and the host sums the copies.
struct QyArgs {
    const SceneDev *scene;
    const char *origins, *directions, *tmax, *skip;
    int32_t oStride, dStride, tStride, sStride;
    int32_t n;
    float tmin; // negative: the scene's ray epsilon
    hr_hit *hits;
    hr_query_surface *surfaces;
    const uint32_t *slotOfPrim;
    const QyGeom *geoms;
    int32_t nGeoms;
    unsigned long long *counters;
};
static const int kQySlots = 64, kQySlotStride = 16;
static const size_t kQyCounterWords = (size_t)kQySlots * kQySlotStride;
void launchQueryTrace(hipStream_t st, const QyArgs &a, bool anyHit);
// the camera of hr_query_pixels as the kernel takes it; xy: n x 2 floats -> rays: n x 6 floats (o, d)
struct QyCamera {
    float view[16];
    float fovTan, aspect, focus, W, H;
};
void launchQueryCamera(hipStream_t st, const QyCamera &cam, int n, const float *xy, float *rays);

// ---- hr_motion.hip (include/hrcore_motion.h)
struct MvCam; // hr_motion.h: the two cameras of a merge or of the motion vectors
static const size_t kMotionSnapshotFloatsPerTri = 12; // (p0, e1, e2) padded to three float4
static const size_t kMotionPlaneBytesPerPixel = 2 * 16; // Mv0, Mv1: two planes of W x H float4 one after the other
// the committed triangles (leaf order, found through slotOfPrim) -> out: kMotionSnapshotFloatsPerTri floats per triangle in prim order
void launchMotionSnapshot(hipStream_t st, uint32_t nTris, const Tri *tris, const uint32_t *slotOfPrim, float *out);
// One trace of the pixel-centre rays of a W x H frame; every pointer is device memory.  geoms / nGeoms: the query's table of the committed
// meshes; remap[m]: the first triangle of mesh m in the snapshot `snap`, or -1 where the snapshot does not hold it with the same count.
// planes: Mv0 then Mv1.  result = {surface, sky, unmatched pixels}, zeroed by the caller.
struct MvTraceArgs {
    const SceneDev *scene;
    const QyGeom *geoms;
    const int32_t *remap;
    const float4 *snap;
    int32_t nGeoms, W, H;
    float view[16], aspect, fov; // the camera: view_matrix, aspect_ratio, fov_tan
    float *planes;
    unsigned long long *result;
};
static const size_t kMotionTraceResultWords = 3, kMotionMergeResultWords = 3;
void launchMotionTrace(hipStream_t st, const MvTraceArgs &a);
// launchHistoryMerge, gathering where the motion planes `mv` say; result as kHistoryResultWords, zeroed by the caller
void launchMotionMerge(hipStream_t st, int W, int H, const MvCam &cam, const HsParams &P, const float *mv, const float *hist, float *frame, float *albedo, float *normalDepth,
                       float *moments, unsigned long long *result);
void launchMotionVectors(hipStream_t st, int W, int H, const MvCam &cam, const float *mv, float *out); // out: W x H float4

// ---- hr_build.hip
// Per-geometry descriptor for the assemble kernel; all pointers are device pointers.  Attributes are addressed with a stride
// (in floats), exactly as the caller handed them over (rlVertexAttribBuffer's stride, Mesh.cpp:104-132): nothing is
// de-interleaved on the host.
struct GeomDev {
    const float *pos, *nrm, *uv, *tan, *bit, *col; // may be null (uv..col)
    int32_t posStride, nrmStride, uvStride, tanStride, bitStride, colStride; // floats between consecutive vertices
    const uint32_t *idx;
    uint32_t triOffset; // first global triangle (prim id) of this geometry
    uint32_t nTris;
    int32_t strip;
    uint32_t flags;    // TF_FRONT_CW | TF_NON_OCCLUDER | TF_HAS_*
    uint32_t material;
    float world[16];
};

static const int kBoundSlots = 64; // copies of the scene bounds the assemble kernel reduces into (6 ordered uints each)
struct Box6 {
    float lo[3], hi[3];
};

// Scene constants derived from the bounds on the device (so that a refit needs no host round trip before its kernels):
// diag = |hi - lo| with the contract's operation order, pad = 1e-5 diag (leaf boxes), eps = 1e-4 diag (ray epsilon)
struct SceneConsts {
    float lo[3], hi[3];
    float diag, pad, eps;
    float areaSum; // sum of the node boxes' surface areas after the last build / refit (tree-quality heuristic only)
    float triAreaSum; // sum of the triangles' areas (invariant under rigid motion, scales with the scene: what areaSum is compared with)
    uint32_t pad1;
};

static const int kMaxLevels = 64;
struct BuildResult {
    Node4 *nodes;
    Node32 *nodes32;      // the same nodes in 32 bytes (k_trace), made by encodeNodes32 after every build / refit
    int *leafKeys;        // Node4::c.w of every node, compact (k_trace finds a leaf child's triangle through it)
    Tri *tris;            // leaf order
    Box6 *nodeBox;        // float box of every node (a refit passes child boxes upwards through it)
    uint32_t *slotOfPrim; // prim id -> position in `tris`
    int32_t nNodes, rootLeafCount;
    int32_t levels; // levels of 4-wide inner nodes (the traversal stack holds at most 3 entries per level)
    uint32_t triSlots;    // entries of `tris` (32-byte nodes: 4 per node, some unused)
    uint32_t levelStart[kMaxLevels + 1]; // nodes of level L are [levelStart[L], levelStart[L + 1]) (breadth-first allocation)
    int32_t builder;            // which binary tree was collapsed: 0 the radix tree over Morton codes (LBVH), 1 PLOC
    float costRadix, costPloc;  // summed surface area of the 4-wide nodes over the root's, per candidate (0: not built)
    float sahCostBefore, sahCostAfter; // ... of the radix tree before and after its bottom subtrees were rebuilt (0: no rebuild ran)
    uint32_t sahFound, sahReplaced;    // bottom subtrees of 3..T triangles; those whose full-sweep SAH version was kept
};
struct BuildOptions {
    int ploc;       // 0: radix tree only; 1: build both, keep the cheaper collapse; 2: PLOC whenever it fits the traversal stack
    int plocRadius; // search radius of the nearest-neighbour step
    int maxLevels;  // levels of 4-wide nodes the traversal stack can hold (a PLOC tree deeper than that is not used)
    int sahSub;     // T: the radix tree's subtrees of at most T <= 64 triangles are rebuilt by full-sweep SAH (0: off)
};

// scene bounds as float-ordered uints: lo.xyz, hi.xyz.  slotOfPrim != null: triangles go to their leaf slot (refit), else prim order.
void launchAssemble(hipStream_t st, const GeomDev *geoms, int nGeoms, uint32_t nTris, Tri *tris, const uint32_t *slotOfPrim, TriAttr *attrs,
                    TriAttrExt *ext, uint32_t *boundsOrdered);
// bounds (ordered uints) -> SceneConsts, and the ray epsilon straight into the device scene block
void launchSceneConsts(hipStream_t st, const uint32_t *boundsOrdered, SceneConsts *out, SceneDev *scene);
// Full LBVH build from assembled triangles (prim order); allocates scratch internally; returns device arrays (hipMalloc).
int buildLBVH(hipStream_t st, const Tri *trisPrimOrder, uint32_t nTris, const float lo[3], const float hi[3], float pad,
              const SceneConsts *deviceConsts, BuildResult *out, const BuildOptions &opt);
// Refit: the tree keeps its topology; every node's child boxes are recomputed bottom-up from the triangles in `tree.tris`
// (already moved by launchAssemble) and re-quantised.  Level by level, no host synchronisation.
void refitLBVH(hipStream_t st, const BuildResult &tree, uint32_t nTris, SceneConsts *consts);
// Node32 of every node from its Node4 (children, counts), the node boxes and the triangles; also writes the grid into *scene (device) when given.
// The grid is a function of the scene bounds in *consts: gridOf() gives the host the same numbers.
void encodeNodes32(hipStream_t st, const BuildResult &tree, const SceneConsts *consts, SceneDev *scene);
void gridOf(const SceneConsts &k, float gridLo[3], float gridCell[3], uint32_t gridCellExp[3]);
// order-independent 64-bit digest of a device buffer, added to *out (device)
void launchHashWords(hipStream_t st, const void *words, size_t nWords, unsigned long long seed, unsigned long long *out);
void launchAreaSum(hipStream_t st, const Box6 *nodeBox, uint32_t n, SceneConsts *consts);
void launchTriAreaSum(hipStream_t st, const Tri *leafTris, uint32_t nSlots, SceneConsts *consts);

// ---- hr_tables.hip (the arithmetic of the sequential generators: hr_tables.h)
void launchMipChain(hipStream_t st, const TexDesc &t, int nLevels, float *mips);
void launchTexLodScale(hipStream_t st, TexDesc *table, int n);
void launchTexDensity(hipStream_t st, const Tri *leafTris, uint32_t nSlots, const TriAttr *attrs, float *out);

// environment importance table (HR_ESTIMATOR_ENV_MIS): scratch and outputs are caller-owned device arrays
void launchEnvGuides(hipStream_t st, const float *rowCdf, const float *colCdf, int w, int h, uint16_t *rowGuide, uint16_t *colGuide);
void launchEnvTable(hipStream_t st, const TexDesc &tex, float *lum, float *dil, uint32_t *wq, unsigned long long *rowSum, unsigned long long *total,
                    uint32_t *maxBits, float *rowCdf, float *colCdf, float *prob, float *meanLum);

void launchQmc(hipStream_t st, int mode, uint32_t sequenceIndex, uint32_t count, float2 *out);
// the sequential generators (hr_tables.h): nSeq tables of `count` points, table s at out + s * stride.  edges == 0: util::uniformRandomFloats
// with seed seed0 + s, else util::randomPolygonal over the polygon (vx, vy)[edges]; launchBlueNoise: util::blueNoise of sequence seq0 + s,
// cand = scratch of nSeq * (count - 1) * 30 points
void launchMtTables(hipStream_t st, uint32_t seed0, int nSeq, uint32_t count, uint32_t edges, const float *vx, const float *vy, float2 *out, size_t stride);
void launchBlueNoise(hipStream_t st, int32_t seq0, int nSeq, uint32_t count, float2 *out, size_t stride, float2 *cand);
void launchMultiscatterLUT(hipStream_t st, const float2 *sobol4096, float *out128x128);

} // namespace hr
