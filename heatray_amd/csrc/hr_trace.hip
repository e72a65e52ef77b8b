// hr_trace.hip — the per-pass wavefront pipeline's traversal stage: persistent-threads BVH traversal (closest hit + occlusion in
// ONE kernel, k_trace) and the debug trace.  Primary-ray generation is hr_raygen.hip, SoA shading with wave-level queue compaction
// hr_shade.hip, accumulation (resolve) hr_frame.hip; what they share is hr_wave.h.
//
// Replaces rlRenderFrame() (/root/reference/Source/HeatrayRenderer/PassGenerator.cpp:386) and the RLSL
// programs it runs (Resources/shaders/perspective.rlsl, physicallyBased.rlsl, glass.rlsl, *Light.rlsl,
// accumulator.rlsl).
//
// A pass needs depth+2 dependent stages (trace -> shade -> trace -> ...), and late stages hold few, long
// rays, so running one pass at a time leaves the chip idle in every stage's tail.  The host therefore
// keeps up to `depth+2` passes in flight, each at a different stage, and every "macro step" launches
//
//   raygen (the pass injected this step)  ->  k_trace (all in-flight passes: closest-hit rays of the
//   current stage + occlusion rays emitted by the previous stage)  ->  k_shade (all in-flight passes)
//   ->  k_resolve (passes that finished)
//
// so each launch carries about one whole pass worth of rays of every depth.  Each in-flight pass sums its
// sample into its own pass buffer (plain read-modify-write: a pixel has at most one live path and one
// live occlusion ray per pass, and the stages are stream-ordered), and k_resolve adds finished samples to
// the accumulation buffer in pass order — reproducible bit for bit.
#include "hr_kernels.h"
#include "hr_display.h"
#include "hr_shade.h"
#include "hr_trace.h"
#include "hr_packet_interval.h"
#include "hr_wave.h"

namespace hr {

#ifndef HR_NODE_STEPS
#define HR_NODE_STEPS 6 // inner-node steps per round of the trace loop
#endif
static const int kWavesPerBlock = kBlock / 64;
#ifndef HR_TRACE_BLOCK
#define HR_TRACE_BLOCK 256 // threads per workgroup of k_trace (an exited workgroup frees its CU slot only as a whole)
#endif
static const int kTraceBlock = HR_TRACE_BLOCK;
static const int kTraceWaves = kTraceBlock / 64;

// -------------------------------------------------------------------------------------------- trace
// Work items of one launch: for every in-flight pass k, its closest-hit queue followed by its occlusion
// queue.  segStart[2k] / segStart[2k+1] are the first global indices of the two.
HRD void buildSegStarts(const StepTable *tbl, uint32_t *segStart /* LDS, 2*kMaxSegs+1 */, bool closestOnly, bool skipPackets = false)
{
    // Queue lengths are read by one thread per queue, all at once (a serial loop over up to 96 passes, two dependent
    // global loads each, used to cost ~0.15 ms at the start of every launch on a small shard); then the first wave turns
    // the lengths into exclusive prefix sums, four entries per lane.
    const int n = tbl->nSeg;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const SegDev &sg = tbl->seg[k];
        segStart[2 * k] = (sg.closestEnabled && !(skipPackets && sg.packets)) ? closestCount(sg) : 0u;
        segStart[2 * k + 1] = closestOnly ? 0u : occlusionCount(sg);
        if (blockIdx.x == 0) { // (a queue longer than what the host provided for: its tail was dropped when it was written)
            if (sg.closestEnabled && sg.packets != 2u && *sg.qCountIn > closestCap(sg)) queueOverflow(tbl, OVF_CLOSEST_IN, (uint32_t)k, *sg.qCountIn);
            if (!closestOnly && *sg.sCountIn > sg.sInCap) queueOverflow(tbl, OVF_OCCLUSION_IN, (uint32_t)k, *sg.sCountIn);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int m = 2 * n; // entries to scan; entry m receives the total
        constexpr int kPer = (2 * kMaxSegs + 1 + 63) / 64; // entries per lane of the first wave
        const int first = (int)threadIdx.x * kPer;
        uint32_t v[kPer];
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            v[j] = (first + j < m) ? segStart[first + j] : 0u;
            sum += v[j];
        }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if ((int)threadIdx.x >= d) incl += up;
        }
        uint32_t acc = incl - sum;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (first + j <= m) segStart[first + j] = acc;
            acc += v[j];
        }
    }
    __syncthreads();
}


#ifndef HR_TAIL_ROUNDS
#define HR_TAIL_ROUNDS 3
#endif
static const unsigned long long kNoHitKey = ~0ull;

#ifdef HR_TAILPROF
// Experiment builds only: when does the work queue run dry, when does the launch end, how long is the longest ray?
__device__ unsigned long long g_tailprof[24]; // [0] min start clock, [1] min exhaustion clock, [2] max end clock, [3] max steps of a ray, [4] sum steps, [5] rays
#endif

// The host's view of the queue lengths (StepTable::hostCounts): the launch's first workgroup stores the closest-hit queue length of every
// table entry to pinned host memory (system scope), then the step's number.  Not inlined: k_trace sits exactly at the register count that
// gives five waves per SIMD, and this prologue must not move it (inlined it cost 4 VGPRs: four waves, -4.5 %).
__device__ __attribute__((noinline)) void reportQueueLengths(const StepTable *tbl, const uint32_t *segStart)
{
    if (!tbl->hostCounts) return;
    for (int k = (int)threadIdx.x; k < tbl->nSeg; k += kTraceBlock)
        __hip_atomic_store(&tbl->hostCounts[k], !tbl->seg[k].closestEnabled ? 0u : (tbl->seg[k].packets == 2u ? closestCap(tbl->seg[k]) : closestCount(tbl->seg[k])), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM); // (packets == 2: the packet kernel runs BESIDE this one and is still filling the queue: its capacity is the bound)
    if (threadIdx.x < 5 && tbl->hostProbe) // (the packet probe's totals so far)
        __hip_atomic_store(&tbl->hostProbe[threadIdx.x], __hip_atomic_load(&tbl->probe[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(tbl->hostSeq, tbl->seqValue, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the slab test's per-ray constants for the 32-byte nodes k_trace walks (the grid is folded into them: hr_trace.h)
HRD RayK traceFrame(const SceneDev &S, v3 o, v3 d)
{
    const float idx = safeInv(d.x), idy = safeInv(d.y), idz = safeInv(d.z);
    return rayFrame32(S, o, idx, idy, idz);
}

// An index whose address arithmetic is done where it is used (the ray-merge slots of the draining phase: their addresses, computed once
// ahead of the triangle loop, held two registers through it that the loop has not got)
HRD uint32_t hereOnly(uint32_t i)
{
    asm volatile("" : "+v"(i));
    return i;
}

template <bool STATS>
__global__ __launch_bounds__(kTraceBlock, 5) void k_trace(const SceneDev *__restrict__ Sp, const int *__restrict__ leafKeys, const Node32 *__restrict__ nodes32,
                                                  const Tri *__restrict__ tris, StepTable *__restrict__ tbl, Stats *stats)
{
    __shared__ int stack[kTraceWaves][kStackLDS][64];
    __shared__ uint32_t segStart[2 * kMaxSegs + 1];
    // merge slots of the drain phase (below): one per ray a wave held when the work queue ran dry
    __shared__ unsigned long long mKey[kTraceWaves][64]; // min over the ray's fragments of (t bits, prim, face bit); kNoHitKey: none
    __shared__ uint32_t mCount[kTraceWaves][64];         // fragments still traversing
    __shared__ float2 mUV[kTraceWaves][64];              // barycentrics that belong to mKey
    __shared__ uint32_t mDonor[kTraceWaves][64];         // k-th donating lane of this round
    const SceneDev &S = *Sp;
    stats += blockIdx.x & (kStatSlots - 1);
    const unsigned long long clk0 = wall_clock64();
    buildSegStarts(tbl, segStart, false, true); // (camera rays that travel as packets are k_raygen_packets' business)
    const int nSeg2 = 2 * tbl->nSeg;
    if (blockIdx.x == 0) reportQueueLengths(tbl, segStart);
    const uint32_t total = segStart[nSeg2];
    const uint32_t lane = laneId(), wave = threadIdx.x >> 6;
    int *stackLane = &stack[wave][0][lane];
    const unsigned long long ltMask = (1ull << lane) - 1ull;
    const int kRefill = tbl->refillLanes, kTriPhase = tbl->triPhaseLanes;
    const uint32_t fetchMax = (uint32_t)tbl->fetchMax, fetchMin = (uint32_t)tbl->fetchMin;
    // Camera rays are coherent: a wave that works through a LONGER run of consecutive pixels refills its idle lanes with neighbours of
    // the rays it still holds, so its lanes keep walking the same part of the tree (a launch of camera rays alone: 9.3 instead of 11.0 ms
    // with 256- instead of 64-ray chunks); the incoherent rays of later stages gain nothing from that and balance better in small chunks
    // (profiles/r3am_fetch_chunks.txt).  The passes injected this step are the last entries of the table.
    // (only when every resident wave gets at least eight such chunks: with fewer — a tile shard — the coarser grain costs more in balance
    // than the coherence brings)
    const uint32_t primaryStart = tbl->primaryFromSeg < tbl->nSeg ? segStart[2 * tbl->primaryFromSeg] : 0xFFFFFFFFu;
    const uint32_t fmPrimary = (uint32_t)tbl->fetchMaxPrimary & 0xFFFFu, fmGate = (uint32_t)tbl->fetchMaxPrimary >> 16;
    const bool longRuns = primaryStart < total && (unsigned long long)(total - primaryStart) >= (unsigned long long)fmGate * fmPrimary * gridDim.x * kTraceWaves;
    const uint32_t fetchMaxPrimary = (longRuns && fmPrimary > fetchMax) ? fmPrimary : fetchMax;
    const uint32_t headsLog2 = tbl->headsLog2, nHeads = 1u << headsLog2;
    const uint32_t wavesTimes2PerRange = ((2u * gridDim.x * kTraceWaves) >> headsLog2) + 1u;
    uint32_t home = blockIdx.x & (nHeads - 1u); // wave-uniform: the range of the index space this wave fetches from
    uint32_t lastBase = 0; // wave-uniform: where the global cursor stood at this wave's previous reservation

    // ---- per-lane traversal state (one ray per lane, refilled from the work pool when a lane finishes)
    int cur = kSentinel, sp = 0;
    uint32_t item = 0xFFFFFFFFu; // global work index of the ray this lane holds
    int segIdx = 0;              // 2k: closest-hit ray of pass k, 2k+1: occlusion ray of pass k
    uint32_t local = 0;          // index inside that queue
    v3 o(0.0f), d(0.0f);
    float idx = 0, idy = 0, idz = 0, oix = 0, oiy = 0, oiz = 0, tmax = 0, tlim = 0;
    uint32_t skipPrim = 0xFFFFFFFFu;
    HitRec best;
    best.prim = kMissPrim, best.t = 0, best.u = 0, best.v = 0;
    int ovf[kStackOvf];
    const float tmin = S.rayEps, hitPad = S.hitPad;
    const int rootRef = (S.nTris == 0) ? kSentinel : (S.rootLeafCount > 0 ? ~(0 | ((S.rootLeafCount - 1) << 28)) : 0);

    uint32_t poolLo = 0, poolHi = 0; // wave-uniform: indices this wave has reserved and not handed out yet
    bool exhausted = false;          // wave-uniform: the global cursor ran past the end
    // Small launches (the late stages of a pass hold a few hundred to a few thousand rays; a tile shard's stages even earlier): up to
    // tbl->staticPerWave rays per resident wave are dealt out statically — wave g takes items [g * per, (g + 1) * per) — instead of
    // through the global cursor.  No same-address atomics (5120 waves learning from one counter that nothing is left took ~60 us of
    // every such launch), every CU gets some of the rays instead of a few waves getting 64 each, and the lanes a wave has left over
    // take subtrees of its rays at once (the drain phase below): a late-stage launch went from ~210 to 50-80 us.  With only a few
    // 64-ray chunks per wave the cursor also balances badly (+-1 chunk is +-40 %): 865 k rays on 5120 waves take 0.80 ms dealt out
    // against 1.30 ms fetched; from ~500 rays per wave on the cursor wins (profiles/r3e_static_deal.txt).
    const uint32_t gridWaves = gridDim.x * kTraceWaves;
    const bool staticDeal = (unsigned long long)total <= (unsigned long long)gridWaves * (unsigned long long)(tbl->staticPerWave > 0 ? tbl->staticPerWave : 0);
    if (staticDeal) {
        const uint32_t per = (total + gridWaves - 1u) / gridWaves;
        const uint32_t gw = wave * gridDim.x + blockIdx.x; // the first gridDim.x chunks go to different workgroups
        const unsigned long long lo = (unsigned long long)gw * per;
        poolLo = lo < total ? (uint32_t)lo : total;
        poolHi = (lo + per < total) ? (uint32_t)(lo + per) : total;
        if (poolLo == poolHi) exhausted = true;
    }
    uint32_t nvC = 0, ntC = 0, nvA = 0, ntA = 0, nacc = 0;

    int pend = 0; // postponed leaf (a negative leaf reference) or 0: the lane keeps descending while a leaf waits
    uint32_t slot = lane;  // merge slot of the ray (fragment) this lane holds during the drain phase
    bool draining = false; // wave-uniform: the merge slots are initialised
#ifdef HR_TAILPROF
    const unsigned long long tStart = wall_clock64();
    const unsigned long long cStart = clock64(); // shader clock, against the 100 MHz wall clock: the frequency the kernel really ran at
    unsigned long long tExh = 0;
    uint32_t mySteps = 0, maxSteps = 0;
    unsigned long long sumSteps = 0, nRays = 0, nGiven = 0, drainIters = 0, drainLanes = 0;
    unsigned long long triPhases = 0, triLanes = 0, nodeRounds = 0, nodeLanes = 0; // (wave-level, counted by lane 0)
#endif
    for (;;) {
        // ---------------- refill idle lanes (persistent threads with dynamic fetch)
        bool idle = (item == 0xFFFFFFFFu);
        unsigned long long idleMask = __ballot(idle);
        int nIdle = __popcll(idleMask);
        if (!exhausted && (nIdle >= kRefill || nIdle == 64)) {
            for (int round = 0; round < 2 && nIdle > 0; ++round) {
                if (poolLo == poolHi) { // reserve another chunk of the global index space
                    if (staticDeal) { // (this wave's share of a small launch has been handed out)
                        exhausted = true;
#ifdef HR_TAILPROF
                        tExh = wall_clock64();
#endif
                        break;
                    }
                    // the next chunk of this wave's current range, or of the next range that still has work (hr_kernels.h: StepTable::heads)
                    bool got = false;
                    uint32_t base = 0, hi = 0;
                    for (uint32_t tries = 0; tries < nHeads; ++tries) {
                        const uint32_t rLo = (uint32_t)(((unsigned long long)total * home) >> headsLog2);
                        const uint32_t rHi = (uint32_t)(((unsigned long long)total * (home + 1u)) >> headsLog2);
                        // chunk ~ (work left in the range) / (2 x the waves that started on it), from the cursor value this wave saw last
                        const uint32_t left = (lastBase >= rLo && lastBase < rHi) ? rHi - lastBase : rHi - rLo;
                        uint32_t chunk = left / wavesTimes2PerRange;
                        const uint32_t fm = (tries == 0 && lastBase >= primaryStart) ? fetchMaxPrimary : fetchMax;
                        chunk = chunk > fm ? fm : (chunk < fetchMin ? fetchMin : chunk);
                        uint32_t off = 0;
                        if (lane == 0) off = atomicAdd(&tbl->heads[home * 32u], chunk);
                        off = __shfl(off, 0);
                        if (off < rHi - rLo) {
                            base = rLo + off;
                            hi = (off + chunk < rHi - rLo) ? base + chunk : rHi;
                            got = true;
                            break;
                        }
                        home = (home + 1u) & (nHeads - 1u);
                    }
                    if (!got) {
                        exhausted = true;
#ifdef HR_TAILPROF
                        tExh = wall_clock64();
#endif
                        break;
                    }
                    lastBase = base;
                    poolLo = base;
                    poolHi = hi;
                }
                const uint32_t avail = poolHi - poolLo;
                const uint32_t rank = (uint32_t)__popcll(idleMask & ltMask);
                if (idle && rank < avail) {
                    item = poolLo + rank;
                    // which queue does the item belong to (at most 2*kMaxSegs entries)
                    int sI = 0, sHiB = nSeg2 - 1; // last queue whose first index is <= item
                    while (sI < sHiB) {
                        const int mid = (sI + sHiB + 1) >> 1;
                        if (item >= segStart[mid])
                            sI = mid;
                        else
                            sHiB = mid - 1;
                    }
                    segIdx = sI;
                    local = item - segStart[sI];
                    const SegDev &sg = tbl->seg[sI >> 1];
                    float4 a, b;
                    if (sI & 1) { // occlusion ray
                        a = G(sg.sqIn.A)[local], b = G(sg.sqIn.B)[local];
                        skipPrim = __float_as_uint(b.w);
                    } else {
                        a = G(sg.qin.A)[local], b = G(sg.qin.B)[local];
                        skipPrim = (uint32_t)G(sg.qin.D)[local].z;
                    }
                    o = v3(a.x, a.y, a.z), d = v3(b.x, b.y, b.z);
                    tmax = a.w, tlim = a.w;
                    {
                        const RayK f = traceFrame(S, o, d);
                        idx = f.idx, idy = f.idy, idz = f.idz, oix = f.oix, oiy = f.oiy, oiz = f.oiz;
                    }
                    best.prim = kMissPrim, best.t = tmax, best.u = 0.0f, best.v = 0.0f;
                    sp = 0;
                    pend = 0;
                    cur = rootRef;
                    idle = false;
                }
                const uint32_t taken = avail < (uint32_t)nIdle ? avail : (uint32_t)nIdle;
                poolLo += taken;
                idleMask = __ballot(idle);
                nIdle = __popcll(idleMask);
            }
        }
        // ---------------- drain phase: the queue is empty, so a launch now lasts as long as its longest ray (0.5 ms for a ray of
        // ~400 node steps, against ~70 on average).  Idle lanes therefore take over pending subtrees of the rays still in
        // flight in their wave: the closest hit is the lexicographic minimum of (t, prim) over ALL triangles, so it does not
        // matter which lane visits which subtree; the fragments of a ray meet in its merge slot.
        if (exhausted) {
            if (!draining) {
                draining = true;
                slot = lane;
                mKey[wave][lane] = kNoHitKey;
                mCount[wave][lane] = (item != 0xFFFFFFFFu) ? 1u : 0u;
            }
            if (item != 0xFFFFFFFFu) { // what the other fragments of this ray have found so far bounds this one too
                const unsigned long long k = mKey[wave][slot];
                if (k != kNoHitKey) {
                    if (segIdx & 1) {
                        cur = kSentinel, sp = 0, pend = 0; // occluded: nothing left to find
                    } else {
                        const float ts = __uint_as_float((uint32_t)(k >> 32));
                        tlim = ts < tlim ? ts : tlim;
                    }
                }
            }
            for (int round = 0; round < HR_TAIL_ROUNDS; ++round) { // a lane gives one subtree per round
            const bool canGive = item != 0xFFFFFFFFu && sp >= 1 && sp <= kStackLDS; // (entries beyond kStackLDS are private)
            const unsigned long long giveMask = __ballot(canGive);
            if (nIdle == 0 || giveMask == 0ull) break;
            {
                const uint32_t nGive = (uint32_t)__popcll(giveMask);
                const uint32_t nMove = nGive < (uint32_t)nIdle ? nGive : (uint32_t)nIdle;
                const uint32_t giveRank = (uint32_t)__popcll(giveMask & ltMask), idleRank = (uint32_t)__popcll(idleMask & ltMask);
                // (LDS hand-offs between lanes of ONE wave: the hardware executes a wave's LDS instructions in order, and the wave barriers
                // keep the compiler from moving or caching the plain accesses across them)
                if (canGive && giveRank < nMove) mDonor[wave][giveRank] = lane;
                __builtin_amdgcn_wave_barrier();
                const bool takes = idle && idleRank < nMove;
                const uint32_t src = takes ? ((volatile uint32_t *)mDonor[wave])[idleRank] : lane;
                // the ray travels by cross-lane reads (every lane executes them), the subtree through the donor's stack column
                const float sox = __shfl(o.x, (int)src), soy = __shfl(o.y, (int)src), soz = __shfl(o.z, (int)src);
                const float sdx = __shfl(d.x, (int)src), sdy = __shfl(d.y, (int)src), sdz = __shfl(d.z, (int)src);
                const float sTmax = __shfl(tmax, (int)src), sTlim = __shfl(tlim, (int)src);
                const uint32_t sSkip = (uint32_t)__shfl((int)skipPrim, (int)src), sItem = (uint32_t)__shfl((int)item, (int)src);
                const uint32_t sLocal = (uint32_t)__shfl((int)local, (int)src), sSlot = (uint32_t)__shfl((int)slot, (int)src);
                const int sSeg = __shfl(segIdx, (int)src);
                const int given = ((volatile int *)stack[wave][0])[src]; // the donor's OLDEST entry: the farthest subtree, usually the largest
                __builtin_amdgcn_wave_barrier(); // (read by the taker before the donor compacts its stack)
                if (canGive && giveRank < nMove) {
                    sp -= 1;
                    if (sp > 0) stackLane[0] = stackLane[sp * 64];
                }
                if (takes) {
                    item = sItem, segIdx = sSeg, local = sLocal, slot = sSlot, skipPrim = sSkip;
                    o = v3(sox, soy, soz), d = v3(sdx, sdy, sdz);
                    tmax = sTmax, tlim = sTlim;
                    {
                        const RayK f = traceFrame(S, o, d);
                        idx = f.idx, idy = f.idy, idz = f.idz, oix = f.oix, oiy = f.oiy, oiz = f.oiz;
                    }
                    best.prim = kMissPrim, best.t = tmax, best.u = 0.0f, best.v = 0.0f;
                    sp = 0, pend = 0, cur = given;
                    atomicAdd(&mCount[wave][slot], 1u);
                    idle = false;
#ifdef HR_TAILPROF
                    nGiven += 1;
#endif
                }
                nIdle -= (int)nMove;
                idleMask = __ballot(idle);
            }
            }
        }
        if (nIdle == 64) { // nothing in flight (finished rays were retired at the end of the previous round)
            if (!exhausted) continue;
            break;
        }
#ifdef HR_TAILPROF
        if (exhausted) drainIters += 1, drainLanes += (unsigned long long)(64 - nIdle);
#endif

        const bool isAny = (segIdx & 1) != 0;
        // ---------------- inner-node steps for every lane that holds an inner node
#pragma unroll
        for (int rep = 0; rep < HR_NODE_STEPS; ++rep) {
#ifdef HR_TAILPROF
            {
                const unsigned long long m = __ballot(cur >= 0 && cur != kSentinel);
                if (m) nodeRounds += 1, nodeLanes += (unsigned long long)__popcll(m);
            }
#endif
            if (cur >= 0 && cur != kSentinel) {
                if (STATS) {
                    if (isAny)
                        ++nvA;
                    else
                        ++nvC;
                }
#ifdef HR_TAILPROF
                ++mySteps;
#endif
                const RayK rk{idx, idy, idz, oix, oiy, oiz};
                nodeStep32(nodes32, cur, sp, stackLane, ovf, rk, tmin, tlim); // (two loads per visit: hr_trace.h)
            }
            // a lane that reached a leaf postpones it and keeps descending (speculative traversal); with a leaf already
            // postponed it is blocked until the wave runs the triangle phase
            if (cur < 0 && pend == 0) {
                pend = cur;
                HR_POP();
            }
        }
        // ---------------- triangle phase: run it once enough lanes wait for it, or when nobody can descend any more
        const unsigned long long blockedMask = __ballot(pend != 0 && (cur < 0 || cur == kSentinel));
        const unsigned long long nodeMask = __ballot(cur >= 0 && cur != kSentinel);
        // (while draining, lane utilisation no longer matters: a waiting leaf is tested at once)
        if (blockedMask != 0ull && (__popcll(blockedMask) >= (exhausted ? 1 : kTriPhase) || nodeMask == 0ull)) {
#ifdef HR_TAILPROF
            triPhases += 1, triLanes += (unsigned long long)__popcll(__ballot(pend != 0));
#endif
            if (pend != 0) {
                const int enc = ~pend;
                // a leaf child of node `enc >> 2` in slot 3 - (enc & 3) (hr_trace.h: nodeStep32): its triangle's index is ~(leafKeys[node] + slot),
                // Node4::c.w of that node in a compact array that stays in L2 (a root leaf — a scene of at most four triangles, no nodes at
                // all — keeps the (first, count) form).  Read HERE, in front of the triangle's loads: reading it where the leaf is put aside
                // (six more load sites in the unrolled node steps) measured 2-5 % slower (profiles/r5_node32_ab.txt)
                int first = enc & 0x0FFFFFFF, count = (enc >> 28) + 1;
                if (rootRef >= 0) first = ~(leafKeys[enc >> 2] + (3 - (enc & 3))), count = 1;
                pend = 0;
                for (int k = 0; k < count; ++k) {
                    const Tri &tr = tris[first + k];
                    const float4 tp = tr.p, tq = tr.q, trr = tr.r;
                    if (STATS) {
                        if (isAny)
                            ++ntA;
                        else
                            ++ntC;
                    }
                    const uint32_t prim = __float_as_uint(trr.y);
                    if (prim == skipPrim) continue;
                    const v3 v0(tp.x, tp.y, tp.z), e1(tp.w, tq.x, tq.y), e2(tq.z, tq.w, trr.x);
                    // Möller–Trumbore; the operation order is part of the arithmetic contract
                    const v3 pvec = cross(d, e2);
                    const float det = dot(e1, pvec);
                    if (det == 0.0f) continue;
                    const float inv = 1.0f / det;
                    const v3 tvec = o - v0;
                    const float u = dot(tvec, pvec) * inv;
                    if (!(u >= 0.0f) || u > 1.0f) continue;
                    const v3 qvec = cross(tvec, e1);
                    const float v = dot(d, qvec) * inv;
                    if (!(v >= 0.0f) || u + v > 1.0f) continue;
                    float t = dot(e2, qvec) * inv;
                    if (!(t > tmin) || !(t < tmax)) continue;
                    // (the hit test's second half, hr_trace.h.  On the live triangle: re-reading it from L1 one axis at a time, to shorten
                    // the live ranges, measured 0.5-1.5 % slower — profiles/r5b_hitbox_ab.txt.  The kernel keeps its five waves per SIMD
                    // because its launch bounds say so: the compiler then allocates for 96 registers without spilling.)
                    if (!hitInTriBox(v0, e1, e2, o, d, t, hitPad) && !hitOnPlane<false>(tris, first + k, o, d, tmin, tmax, hitPad, t)) continue; // (the plane retry: cold)
                    if (isAny) {
                        if ((__float_as_uint(trr.z) & TF_NON_OCCLUDER) && alphaPasses(S, prim, u, v)) continue;
                        best.prim = 0u; // occluded (anything but kMissPrim)
                        cur = kSentinel;
                        sp = 0;
                        if (draining) atomicMin(&mKey[wave][hereOnly(slot)], 0ull); // the ray's other fragments stop at their next round
                        break;
                    }
                    const uint32_t bp = best.prim & 0x7FFFFFFFu;
                    if (best.prim == kMissPrim || t < best.t || (t == best.t && prim < bp)) {
                        best.prim = prim | ((det > 0.0f) ? 0x80000000u : 0u);
                        best.t = t, best.u = u, best.v = v;
                        tlim = t;
                        if (draining) { // publish at once: subtrees handed to other lanes are speculative until a hit bounds them
                            const unsigned long long kk = ((unsigned long long)__float_as_uint(t) << 32) | ((unsigned long long)prim << 1) |
                                                          (unsigned long long)(det > 0.0f ? 1u : 0u);
                            const uint32_t sl = hereOnly(slot);
                            atomicMin(&mKey[wave][sl], kk);
                            __builtin_amdgcn_wave_barrier();
                            if (((volatile unsigned long long *)mKey[wave])[sl] == kk) mUV[wave][sl] = make_float2(u, v);
                        }
                    }
                }
            }
        }
        // ---------------- retire finished rays
        if (draining && cur == kSentinel && pend == 0 && item != 0xFFFFFFFFu) {
            // a fragment is done: fold its result into the ray's slot; the last fragment writes the ray's result
            const bool hit = best.prim != kMissPrim;
            const unsigned long long myKey =
                !hit ? kNoHitKey
                     : (isAny ? 0ull
                              : (((unsigned long long)__float_as_uint(best.t) << 32) | ((unsigned long long)(best.prim & 0x7FFFFFFFu) << 1) |
                                 (unsigned long long)(best.prim >> 31)));
            if (hit) atomicMin(&mKey[wave][slot], myKey);
            __builtin_amdgcn_wave_barrier();
            if (hit && !isAny && ((volatile unsigned long long *)mKey[wave])[slot] == myKey) mUV[wave][slot] = make_float2(best.u, best.v);
            __builtin_amdgcn_wave_barrier();
            const uint32_t before = atomicSub(&mCount[wave][slot], 1u);
            if (before == 1u) {
                const unsigned long long k = ((volatile unsigned long long *)mKey[wave])[slot];
                const SegDev &sg = tbl->seg[segIdx >> 1];
                if (isAny) {
                    if (k == kNoHitKey) {
                        const float4 c = G(sg.sqIn.C)[local];
                        HR_GLOBAL float *px = G(sg.passbuf) + (size_t)__float_as_uint(c.w) * 4;
                        px[0] = px[0] + c.x;
                        px[1] = px[1] + c.y;
                        px[2] = px[2] + c.z;
                        ++nacc;
                    }
                } else {
                    HitRec h;
                    h.prim = kMissPrim, h.t = tmax, h.u = 0.0f, h.v = 0.0f;
                    if (k != kNoHitKey) {
                        const uint32_t lo = (uint32_t)k;
                        const float2 uv = make_float2(((volatile float *)&mUV[wave][slot])[0], ((volatile float *)&mUV[wave][slot])[1]);
                        h.prim = (lo >> 1) | (lo << 31), h.t = __uint_as_float((uint32_t)(k >> 32)), h.u = uv.x, h.v = uv.y;
                    }
                    G(sg.hits)[local] = h;
                }
            }
#ifdef HR_TAILPROF
            maxSteps = mySteps > maxSteps ? mySteps : maxSteps, sumSteps += mySteps, nRays += (before == 1u), mySteps = 0;
#endif
            item = 0xFFFFFFFFu;
        }
        if (cur == kSentinel && pend == 0 && item != 0xFFFFFFFFu) {
            const SegDev &sg = tbl->seg[segIdx >> 1];
            if (isAny) {
                if (best.prim == kMissPrim) { // unoccluded: the light's shader accumulates into the pass's sample
                    const float4 c = G(sg.sqIn.C)[local];
                    HR_GLOBAL float *px = G(sg.passbuf) + (size_t)__float_as_uint(c.w) * 4;
                    px[0] = px[0] + c.x;
                    px[1] = px[1] + c.y;
                    px[2] = px[2] + c.z;
                    ++nacc;
                }
            } else {
                G(sg.hits)[local] = best;
            }
#ifdef HR_TAILPROF
            maxSteps = mySteps > maxSteps ? mySteps : maxSteps, sumSteps += mySteps, nRays += 1, mySteps = 0;
#endif
            item = 0xFFFFFFFFu;
        }
    }
#ifdef HR_TAILPROF
    {
        const unsigned long long tEnd = wall_clock64();
        atomicMin(&g_tailprof[0], tStart);
        if (tExh) atomicMin(&g_tailprof[1], tExh);
        atomicMax(&g_tailprof[2], tEnd);
        atomicMax(&g_tailprof[3], (unsigned long long)maxSteps);
        atomicAdd(&g_tailprof[4], sumSteps);
        atomicAdd(&g_tailprof[5], nRays);
        atomicAdd(&g_tailprof[6], nGiven);
        if (blockIdx.x == 0 && threadIdx.x == 0) g_tailprof[18] = clock64() - cStart, g_tailprof[19] = tEnd - tStart;
        if (lane == 0) {
            atomicMax(&g_tailprof[7], drainIters);
            atomicAdd(&g_tailprof[16], drainLanes);
            atomicAdd(&g_tailprof[17], drainIters);
            atomicAdd(&g_tailprof[20], triPhases);
            atomicAdd(&g_tailprof[21], triLanes);
            atomicAdd(&g_tailprof[22], nodeRounds);
            atomicAdd(&g_tailprof[23], nodeLanes);
        }
        if (tExh && lane == 0) { // per-wave drain time in 0.05 ms buckets
            unsigned long long b = (tEnd - tExh) / 5000ull;
            atomicAdd(&g_tailprof[8 + (b > 15ull ? 15ull : b)], 1ull);
        }
    }
#endif

    nacc = waveSum(nacc);
    if (lane == 0 && nacc) atomicAdd(&stats->accumulates, (unsigned long long)nacc);
    if (STATS) {
        nvC = waveSum(nvC), ntC = waveSum(ntC), nvA = waveSum(nvA), ntA = waveSum(ntA);
        if (lane == 0) {
            atomicAdd(&stats->nodeVisits, (unsigned long long)nvC + nvA);
            atomicAdd(&stats->triTests, (unsigned long long)ntC + ntA);
            atomicAdd(&stats->nodeVisitsAny, (unsigned long long)nvA);
            atomicAdd(&stats->triTestsAny, (unsigned long long)ntA);
        }
    }
    // ---- the launch times itself (StepTable::clkStart): every workgroup folds its start and end into one of kClkSlots (min, max)
    // pairs — 80 atomics per address, spread over the launch; ONE counter of finished workgroups would put 1280 same-address
    // atomics (~12 ns each) into the tail of every launch.  The kernel behind this one (k_shade_sort) adds max - min to the counters.
    if (threadIdx.x == 0) {
        const uint32_t cs = blockIdx.x & (kClkSlots - 1);
        __hip_atomic_fetch_min(&tbl->clkStart[cs], clk0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&tbl->clkEnd[cs], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long nc = 0, na = 0;
        for (int k = 0; k < tbl->nSeg; ++k) {
            nc += segStart[2 * k + 1] - segStart[2 * k];
            na += segStart[2 * k + 2] - segStart[2 * k + 1];
        }
        atomicAdd(&stats->raysClosest, nc);
        atomicAdd(&stats->raysAny, na);
    }
}
// The product variant is instantiated first, here, ahead of launchTrace's two uses: of the two instantiations the compiler gives the one
// it creates first the code k_trace<false> had when all stages were one file (4712 instructions), and the other a different one; this way
// round it is the statistics variant that moves (tools/kernel_isa.py, profiles/render_split_isa.txt).
template __global__ void k_trace<false>(const SceneDev *__restrict__, const int *__restrict__, const Node32 *__restrict__, const Tri *__restrict__, StepTable *__restrict__, Stats *);

// ------------------------------------------------------------------------------------ debug trace
__global__ __launch_bounds__(kBlock) void k_debug_trace(const SceneDev *__restrict__ Sp, int n, const float *__restrict__ o,
                                                        const float *__restrict__ d, const float *__restrict__ tmax,
                                                        const int *__restrict__ skip, int anyHit, hr_hit *__restrict__ out)
{
    __shared__ int stack[kWavesPerBlock][kStackLDS][64];
    const SceneDev &S = *Sp;
    const uint32_t lane = laneId(), wave = threadIdx.x >> 6;
    int *stackLane = &stack[wave][0][lane];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const v3 ro(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    const float tm = tmax ? tmax[i] : __builtin_inff();
    const uint32_t sk = skip ? (uint32_t)skip[i] : 0xFFFFFFFFu;
    HitRec h;
    uint32_t nv = 0, nt = 0;
    hr_hit r;
    if (anyHit) {
        traverse<true, false>(S, ro, rd, S.rayEps, tm, sk, stackLane, h, nv, nt);
        r.prim = (h.prim == kMissPrim) ? -1 : 0;
        r.t = r.u = r.v = 0.0f;
    } else {
        traverse<false, false>(S, ro, rd, S.rayEps, tm, sk, stackLane, h, nv, nt);
        const bool hit = h.prim != kMissPrim;
        r.prim = hit ? (int)(h.prim & 0x7FFFFFFFu) : -1;
        r.t = hit ? h.t : 0.0f, r.u = hit ? h.u : 0.0f, r.v = hit ? h.v : 0.0f;
    }
    out[i] = r;
}

void launchTrace(const LaunchCfg &cfg, const SceneDev *S, const int *leafKeys, const Node32 *nodes32, const Tri *tris, StepTable *tbl, Stats *stats)
{
    const int grid = cfg.numCUs * cfg.traceBlocksPerCU * (kBlock / kTraceBlock); // traceBlocksPerCU counts 256-thread workgroups
    if (cfg.collectStats)
        hipLaunchKernelGGL(k_trace<true>, dim3(grid), dim3(kTraceBlock), 0, cfg.stream, S, leafKeys, nodes32, tris, tbl, stats);
    else
        hipLaunchKernelGGL(k_trace<false>, dim3(grid), dim3(kTraceBlock), 0, cfg.stream, S, leafKeys, nodes32, tris, tbl, stats);
}

void launchDebugTrace(const LaunchCfg &cfg, const SceneDev *S, int n, const float *o, const float *d, const float *tmax, const int *skip,
                      int anyHit, hr_hit *out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_debug_trace, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, cfg.stream, S, n, o, d, tmax, skip, anyHit, out);
}

size_t hitRecordSize() { return sizeof(HitRec); }

} // namespace hr

#ifdef HR_TAILPROF
extern "C" int hr_debug_tailprof(unsigned long long *out8, int reset)
{
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(hr::g_tailprof), sizeof(unsigned long long) * 24) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[24] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(hr::g_tailprof), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
