// hr_pipeline.inl — a section of hr_core.hip (included there, inside its extern "C" block): the pass pipeline — pass slots and ray memory,
// the macro step (tables, launches, the packet selector), batching, hr_render_pass / hr_flush, statistics of the pipeline itself.
// macroStep is its stages in order, handing on a StepPlan: 1 injectPasses (pickSlot) — 2 endDrainedPassthrough — 3 listInFlight —
// 4 boundQueues (waitCounts, PacketSelector::takeReport) — 5 sizeStepMemory (hr_step_memory.h, BudgetSeen::record, ensureRegion,
// takeBackInjection) — 6 buildTable (the carve and its check) — 7 decidePackets (PacketSelector::wantsProbe) — 8 launchStep
// (launchCameraRays, launchProbe, corunTraceBlocks) — 9 advancePasses; then resolveReady.
int hr_clear(hr_ctx *c)
{
    ENTER(c);
    if (c->grp) return groupClear(c);
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    int rc = drainPipeline(c);
    if (rc) return rc;
    if (c->hOverflow && c->hOverflow[0]) { // a dropped-rays report: the frame starts afresh and so does the report, once nothing that could repeat it is running
        QUIESCE(c);
        c->hOverflow[0] = c->hOverflow[1] = c->hOverflow[2] = c->hOverflow[3] = 0u;
    }
    HIP_TRY(c, hipMemsetAsync(c->fb(), 0, (size_t)c->W * c->H * 4 * sizeof(float), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dStats, 0, sizeof(Stats) * kStatSlots, c->stream));
    for (float *plane : c->aov.plane)
        if (plane) HIP_TRY(c, hipMemsetAsync(plane, 0, (size_t)c->W * c->H * 4 * sizeof(float), c->stream));
    c->resolvedAtClear = c->aov.zeroedAt = c->frameZeroedAt = c->nextResolveOrder;
    featuresFrameCleared(c);
    c->snapshotEpoch++;
    if (c->tune.debugPipe) fprintf(stderr, "hr_clear %p: ray-memory growths so far %llu, waits %llu (%.2f ms)\n", (void *)c, c->dbgGrowths, c->dbgWaits, (double)c->dbgWaitNs * 1e-6);
    c->drainTimes();
    for (int k = 0; k < HR_KERNEL_COUNT; ++k) c->kernelMs[k] = 0.0f, c->kernelLaunches[k] = 0;
    return HR_OK;
}

static int allocSlot(hr_ctx *c, hr_ctx::PassSlot &ps, hipStream_t st)
{
    const size_t fbBytes = (size_t)c->W * c->H * 4 * sizeof(float);
    const size_t sums = c->allLightsUsed ? 4 : 1;
    // (with HR_ESTIMATOR_ALL_LIGHTS the sample's further partial sums lie right behind the first: k_trace indexes one buffer; the AOV record
    // of HR_AOV_SURFACE behind them)
    const hipError_t e = ps.passbuf.alloc((size_t)c->W * c->H * 4 * (sums + c->aov.framesPerSlot()));
    if (e != hipSuccess) { // say what ran out: a pass slot is the unit the pipeline's memory grows in
        size_t freeB = 0, totalB = 0;
        hipMemGetInfo(&freeB, &totalB);
        c->err = "pass slot " + std::to_string(c->nSlotsAllocated + 1) + " (" + std::to_string(fbBytes >> 20) + " MiB pass buffer at " + std::to_string(c->W) + "x" +
                 std::to_string(c->H) + "): " + hipGetErrorString(e) + "; " + std::to_string(freeB >> 20) + " MiB of device memory free";
        return HR_ERR_DEVICE;
    }
    if (c->allLightsUsed) ps.passbufB = ps.passbuf + (size_t)c->W * c->H * 4;
    if (c->aov.framesPerSlot()) { // zeroed once here (complete before any stream uses the slot); from then on the resolve that reads a pass's record zeroes it
        ps.aov = ps.passbuf + sums * (size_t)c->W * c->H * 4;
        HIP_TRY(c, hipMemsetAsync(ps.aov, 0, fbBytes * c->aov.framesPerSlot(), st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    ps.ctr = c->dCounters + (&ps - c->slots);
    HIP_TRY(c, ps.evFinal.create(hipEventDisableTiming));
    HIP_TRY(c, ps.evResolved.create(hipEventDisableTiming));
    ps.allocated = true;
    c->nSlotsAllocated++;
    return HR_OK;
}

// ---- the groups' ray memory (hr_ctx::Group::arena / scratch); the sizes are hr_step_memory.h's
static RayQueue carveRayQueue(char *&p, size_t cap)
{
    RayQueue q;
    const size_t n = queuePlaneBytes(cap);
    q.A = (float4 *)p, q.B = (float4 *)(p + n), q.C = (float4 *)(p + 2 * n), q.D = (int4 *)(p + 3 * n);
    p += kRayQueuePlanes * n;
    return q;
}
static ShadowQueue carveShadowQueue(char *&p, size_t cap)
{
    ShadowQueue q;
    const size_t n = queuePlaneBytes(cap);
    q.A = (float4 *)p, q.B = (float4 *)(p + n), q.C = (float4 *)(p + 2 * n);
    p += kShadowQueuePlanes * n;
    return q;
}
// a region that is too small is replaced once everything the group has enqueued is done (what it held is dead by then: a step's
// scratch dies with the step, and arena[t & 1] holds the rays step t - 2 emitted, which step t - 1 consumed)
static int ensureRegion(hr_ctx *c, hr_ctx::Group &G, hr_ctx::Group::Region &r, size_t need, const char *what)
{
    if (need <= r.cap) return HR_OK;
    c->dbgGrowths++, c->dbgGrowBytes += need;
    if (c->tune.debugPipe) fprintf(stderr, "  grow %s: need %.1f MiB, had %.1f MiB (step %llu)\n", what, (double)need / 1048576.0, (double)r.cap / 1048576.0, G.stepCounter);
    HIP_TRY(c, hipStreamSynchronize(G.stream));
    const size_t hadCap = r.cap;
    r.base.reset(), r.cap = 0;
    // a third of headroom: counts vary from pass to pass, and while the pipeline fills (the first depth + 2 steps of a render) every
    // step carries one more generation of passes — for the benchmark soup the steady state needs 27 % more than the step that
    // triggered the last growth (profiles/r4m_mem.txt); a step that needs more regrows once more
    size_t want = need + need / 3;
    if (hadCap && !c->memBudget && want < hadCap + hadCap / 2) want = hadCap + hadCap / 2; // (a region that has to grow again grows by half at least: few events; under a memory budget only by what is needed)
    want = (want + ((size_t)2 << 20)) & ~(((size_t)2 << 20) - 1);
    hipError_t e = r.base.alloc(want);
    size_t got = want;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        got = align256(need);
        e = r.base.alloc(got);
    }
    if (e != hipSuccess) {
        size_t freeB = 0, totalB = 0;
        hipMemGetInfo(&freeB, &totalB);
        c->err = std::string("ray memory (") + what + ", " + std::to_string(need >> 20) + " MiB for one macro step at " + std::to_string(c->W) + "x" + std::to_string(c->H) +
                 "): " + hipGetErrorString(e) + "; " + std::to_string(freeB >> 20) + " MiB of device memory free";
        return HR_ERR_DEVICE;
    }
    r.cap = got;
    return HR_OK;
}

// passes that hold a slot: in flight, or finished and waiting for their turn to resolve
static int occupiedSlots(const hr_ctx *c, int group)
{
    int n = 0;
    for (const hr_ctx::PassSlot &ps : c->slots) n += ((ps.active || ps.finished) && (group < 0 || ps.group == group)) ? 1 : 0;
    return n;
}

static int slotLimit(const hr_ctx *c);
static int activePasses(const hr_ctx *c)
{
    int n = 0;
    for (const hr_ctx::PassSlot &ps : c->slots) n += ps.active ? 1 : 0;
    return n;
}

// Finished passes are added to the frame on the caller's stream, strictly in pass order (float addition order is
// part of the arithmetic contract), whatever order the groups finished them in.
static int resolveReady(hr_ctx *c)
{
    FrameDev fr = c->frame;
    fr.fb = c->fb();
    const LaunchCfg cfg = c->cfg(c->stream);
    for (;;) {
        // collect the passes whose turn it is (up to kMaxBatch) and add them with one launch
        PassBufList bufs{};
        hr_ctx::PassSlot *ready[kMaxBatch];
        while (bufs.n < kMaxBatch) {
            hr_ctx::PassSlot *next = nullptr;
            const unsigned long long want = c->nextResolveOrder + (unsigned long long)bufs.n;
            for (hr_ctx::PassSlot &ps : c->slots)
                if ((ps.active || ps.finished) && ps.order == want) next = &ps;
            if (!next || !next->finished) break;
            ready[bufs.n] = next;
            bufs.bufB[bufs.n] = next->pp.estimator == HR_ESTIMATOR_ALL_LIGHTS ? next->passbufB : nullptr;
            bufs.buf[bufs.n++] = next->passbuf;
        }
        if (bufs.n == 0) {
            // nothing requested is unfinished any more: the age of "the oldest waiting request" starts afresh with the next request
            // (stamped only in hr_render_pass, it used to survive every pass that completed the normal way, so that 4 ms after the
            // first request EVERY progressive read-back that found the streams idle drained a partly filled batch)
            if (c->pendingInject.empty() && occupiedSlots(c) == 0) c->oldestWaitingNs = 0;
            return HR_OK;
        }
        for (int k = 0; k < bufs.n; ++k) {
            bool seen = false;
            for (int j = 0; j < k; ++j) seen = seen || ready[j]->finalEv == ready[k]->finalEv;
            if (!seen) HIP_TRY(c, hipStreamWaitEvent(c->stream, ready[k]->finalEv, 0));
        }
        c->timeBegin(HR_KERNEL_RESOLVE, c->stream);
        if (c->aov.mask) {
            AovList aov{};
            aov.albedo = c->aov.plane[HR_AOV_PLANE_ALBEDO], aov.normalDepth = c->aov.plane[HR_AOV_PLANE_NORMAL_DEPTH], aov.moments = c->aov.plane[HR_AOV_PLANE_MOMENTS];
            for (int k = 0; k < bufs.n; ++k) aov.pass[k] = ready[k]->aov;
            launchResolveAov(cfg, fr, bufs, aov);
        } else {
            launchResolve(cfg, fr, bufs);
        }
        c->timeEnd(c->stream);
        HIP_TRY(c, hipEventRecord(ready[bufs.n - 1]->evResolved, c->stream));
        for (int k = 0; k < bufs.n; ++k) {
            ready[k]->resolvedEv = ready[bufs.n - 1]->evResolved;
            ready[k]->finished = false, ready[k]->everResolved = true;
            ready[k]->resolvedAt = c->nextResolveOrder;
            c->nextResolveOrder++;
        }
    }
}

// wait for the queue lengths step (want - 1) of this group reports when its k_trace starts (Group::hCounts)
static int waitCounts(hr_ctx *c, hr_ctx::Group &G, int ring, unsigned long long want)
{
    const auto t0 = std::chrono::steady_clock::now();
    c->dbgWaits++;
    for (unsigned spins = 0;; ++spins) {
        if (G.hSeq[ring] == want) {
            if (spins) c->dbgWaitSpun++, c->dbgWaitNs += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            break;
        }
        if ((spins & 255u) == 255u) {
            const hipError_t q = hipStreamQuery(G.stream);
            if (q == hipSuccess) { // everything enqueued has run: the report must have arrived
                if (G.hSeq[ring] == want) break;
                FAIL(c, HR_ERR_DEVICE, "internal: a step's queue lengths never arrived");
            }
            if (q != hipErrorNotReady) HIP_TRY(c, q);
            std::this_thread::yield();
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return HR_OK;
}

// ---- One macro step of pipeline group g: (raygen of the injected passes) -> trace of every in-flight pass of the group ->
// shade; passes whose last stage this was become `finished`.  macroStep (below) is the list of its stages; StepPlan is what they hand on.
static int stagesOf(const hr_ctx *c, const hr_pass_params &pp);
struct StepPlan {
    int g;
    hr_ctx::Group *G;
    LaunchCfg cfg; // as the step began: a probe report the step itself evaluates (boundQueues) bears on the launches of the steps after it
    FrameDev fr;
    unsigned long long stepIdx;
    int ring;   // the step's entry of the table ring
    uint32_t P; // camera rays an injected pass can have
    size_t kS;  // occlusion rays per closest-hit ray
    int order[kMaxSlots], n;    // the group's in-flight passes (their slots), oldest first: the step table's entries
    uint32_t boundIn[kMaxSegs]; // per entry, an upper bound of the closest-hit rays it traces in this step
    int injectedSlots[kMaxSegs], nInjected;
    int injectedSegs[kMaxSegs], nInjectedSegs; // ... and their entries of the table
    bool packetsNow, corunNow, anyLens;        // the selector's decision for this step (decidePackets)
    int probeSeg;                              // table entry whose pass the step's probe looks through, -1: no probe
    size_t needArena, needScratch;             // bytes the step carves
};
// HR_DEBUG_STEPTIMES: host time at the stages' borders
struct StepClock {
    bool on;
    double t[5];
    int n;
    static double nowUs() { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() * 1e-3; }
    void mark()
    {
        if (on && n < 5) t[n++] = nowUs();
    }
    void print(unsigned long long stepIdx, int nInject) const
    {
        if (on) fprintf(stderr, "step %llu (inject %d): begin %.1f us | injected +%.1f | counts known +%.1f | table built +%.1f | copy enqueued +%.1f | launched +%.1f\n", stepIdx, nInject, t[0], t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], nowUs() - t[4]);
    }
};
static bool tracesClosest(const hr_ctx *c, const hr_ctx::PassSlot &ps) { return c->hasPassthrough || ps.step < ps.nIter; }

// The slot an injected pass takes: the free one whose pass was resolved longest ago: the injection waits for that resolve, and a slot
// freed by the step just enqueued would chain this group's step behind the other group's (no overlap).  A slot resolved only recently
// is passed over for fresh memory while the slot budget allows.  -1: none is free.
static int pickSlot(const hr_ctx *c, int nInject)
{
    int slot = -1, fresh = -1;
    for (int i = 0; i < kMaxSlots; ++i) {
        const hr_ctx::PassSlot &cand = c->slots[i];
        if (cand.active || cand.finished) continue;
        if (!cand.allocated) {
            if (fresh < 0) fresh = i;
        } else if (slot < 0 || cand.resolvedAt < c->slots[slot].resolvedAt) {
            slot = i;
        }
    }
    const unsigned long long recent = 2ull * (unsigned long long)c->nGroups * (unsigned long long)(nInject > 0 ? nInject : 1);
    if (fresh >= 0 && c->nSlotsAllocated < slotLimit(c) && (slot < 0 || (c->nGroups > 1 && c->nextResolveOrder - c->slots[slot].resolvedAt < recent)))
        slot = fresh;
    return slot < 0 ? fresh : slot;
}

// stage 1: what the caller's stream set up becomes visible, the waiting passes take their slots, their counters go back to zero
static int injectPasses(hr_ctx *c, StepPlan &S, int nInject)
{
    hr_ctx::Group &G = *S.G;
    if (G.needUserSync) { // state set up on the caller's stream (scene, tables, cleared buffers) must be visible
        HIP_TRY(c, hipEventRecord(G.evUser, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(G.stream, G.evUser, 0));
        G.needUserSync = false;
    }
    hipEvent_t waited[kMaxSegs];
    S.nInjected = 0;
    for (int k = 0; k < nInject; ++k) {
        const hr_pass_params pp = c->pendingInject.front();
        c->pendingInject.pop_front();
        const int slot = pickSlot(c, nInject);
        if (slot < 0) FAIL(c, HR_ERR_INVALID, "internal: no free pass slot");
        hr_ctx::PassSlot &ps = c->slots[slot];
        if (!ps.allocated) {
            int rc = allocSlot(c, ps, G.stream);
            if (rc) return rc;
        }
        if (ps.everResolved) { // the pass buffer is free again once the launch that resolved it has run
            bool seen = false;
            for (int j = 0; j < S.nInjected; ++j) seen = seen || waited[j] == ps.resolvedEv;
            if (!seen) HIP_TRY(c, hipStreamWaitEvent(G.stream, ps.resolvedEv, 0));
        }
        waited[S.nInjected] = ps.everResolved ? ps.resolvedEv : nullptr;
        ps.active = true, ps.finished = false, ps.group = S.g, ps.step = 0, ps.nIter = pp.max_ray_depth + 1, ps.pp = pp;
        ps.qcur = RayQueue{}, ps.scur = ShadowQueue{}, ps.capCur = 0, ps.sCapCur = 0;
        ps.order = c->injected++;
        S.injectedSlots[S.nInjected++] = slot;
    }
    for (int j0 = 0; j0 < S.nInjected; j0 += kMaxBatch) { // the injected passes' counters back to zero, one launch
        CounterList cl{};
        for (int j = j0; j < S.nInjected && cl.n < kMaxBatch; ++j) cl.ctr[cl.n++] = c->slots[S.injectedSlots[j]].ctr;
        launchZeroCounters(S.cfg, cl);
    }
    return HR_OK;
}
// Nothing of the step has been enqueued except the counters' reset: the passes it was to inject go back to the head of the request queue
// (their slots are free again), so that a later call injects them properly instead of tracing queues no k_raygen ever filled.
static void takeBackInjection(hr_ctx *c, StepPlan &S)
{
    for (int j = S.nInjected - 1; j >= 0; --j) {
        hr_ctx::PassSlot &ps = c->slots[S.injectedSlots[j]];
        c->pendingInject.push_front(ps.pp);
        ps.active = false;
        c->injected--;
    }
    S.G->stepCounter--;
}

// stage 2.  Pass-through rays (back faces of single-sided materials, alpha masks: physicallyBased.rlsl:70-108) are not bounded by
// maxRayDepth, so in such scenes a pass runs until its closest-hit queue is empty.  The queue lengths come from the snapshot
// taken two macro steps ago (see Group::hQCount): a slot about to run stage `st` then knows the lengths of stages <= st - 1;
// if stage st - 1 had no rays, it emitted nothing and the pass was complete with the steps already enqueued.
static int endDrainedPassthrough(hr_ctx *c, StepPlan &S)
{
    hr_ctx::Group &G = *S.G;
    const unsigned long long N = G.stepCounter;
    if (!c->hasPassthrough || N < 2 || !G.statusUsed[(N - 2) % kTableRing]) return HR_OK;
    const int ring = (int)((N - 2) % kTableRing);
    HIP_TRY(c, hipEventSynchronize(G.statusEv[ring]));
    hr_ctx::PassSlot *endedEarly[kMaxSlots];
    int nEndedEarly = 0;
    const uint32_t *snap = G.hQCount + (size_t)ring * kMaxSlots * kMaxBounceSlots;
    for (int i = 0; i < kMaxSlots; ++i) {
        hr_ctx::PassSlot &ps = c->slots[i];
        if (!ps.active || ps.group != S.g || G.statusOrder[ring][i] != ps.order + 1ull) continue;
        const int st = ps.step;
        const bool empty = st >= 2 && snap[(size_t)i * kMaxBounceSlots + ((st - 1) % kMaxBounceSlots)] == 0u;
        if (empty) {
            ps.active = false, ps.finished = true;
            endedEarly[nEndedEarly++] = &ps;
        }
    }
    hr_ctx::PassSlot *owner = nullptr; // the newest of them: it is resolved last, so its event outlives the others' waits
    for (int k = 0; k < nEndedEarly; ++k)
        if (!owner || endedEarly[k]->order > owner->order) owner = endedEarly[k];
    if (owner) HIP_TRY(c, hipEventRecord(owner->evFinal, G.stream));
    for (int k = 0; k < nEndedEarly; ++k) endedEarly[k]->finalEv = owner->evFinal;
    return HR_OK;
}

// stage 3: the group's in-flight passes, oldest first
static void listInFlight(const hr_ctx *c, StepPlan &S)
{
    S.n = 0;
    for (int i = 0; i < kMaxSlots; ++i)
        if (c->slots[i].active && c->slots[i].group == S.g) S.order[S.n++] = i;
    for (int a = 1; a < S.n; ++a)
        for (int b = a; b > 0 && c->slots[S.order[b]].order < c->slots[S.order[b - 1]].order; --b) std::swap(S.order[b], S.order[b - 1]);
}

// stage 4: every queue of the step is sized by an upper bound of what can arrive in it (Group::arena): wait for the lengths the previous
// step's k_trace reported — the packet probe's totals come with them — and bound each pass's closest-hit queue
static int boundQueues(hr_ctx *c, StepPlan &S)
{
    hr_ctx::Group &G = *S.G;
    bool wanted = false;
    for (int k = 0; k < S.n; ++k) wanted = wanted || c->slots[S.order[k]].step > 0;
    int idxOfSlot[kMaxSlots];
    const int prev = (int)((S.stepIdx + kTableRing - 1) % kTableRing);
    if (wanted && S.stepIdx > 0) {
        int rc = waitCounts(c, G, prev, S.stepIdx); // (step stepIdx - 1 wrote stepIdx: its number + 1)
        if (rc) return rc;
        if (S.g == 0) c->selector.takeReport(G.hProbe + 8 * prev, S.stepIdx, c->tune);
        for (int i = 0; i < kMaxSlots; ++i) idxOfSlot[i] = -1;
        for (int j = 0; j < G.countN[prev]; ++j) idxOfSlot[G.countSlot[prev][j]] = j;
    }
    for (int k = 0; k < S.n; ++k) {
        const hr_ctx::PassSlot &ps = c->slots[S.order[k]];
        uint32_t b = S.P;
        if (ps.step > 0) {
            b = ps.capCur; // (what its queue can hold is a bound too: used when the pass was not in the previous step's table)
            const int j = (wanted && S.stepIdx > 0) ? idxOfSlot[S.order[k]] : -1;
            if (j >= 0 && G.countOrder[prev][j] == ps.order + 1ull) {
                const uint32_t seen = G.hCounts[(size_t)prev * kMaxSegs + j]; // length of its closest-hit queue one stage ago
                b = seen < b ? seen : b;
                if (ps.step == 1 && seen < S.P) c->selector.lastCameraCount = seen; // (camera rays that passed the root cull: what a packet kernel traces per pass)
            }
        }
        // TEST ONLY (HR_TUNE="ovf=": tests/test_gpu_parity.py forces every kind of overflow once): half of what the bound should be
        if (c->tune.ovf == 2 && ps.step == 1) b = b / 2u + 1u;
        S.boundIn[k] = b;
    }
    return HR_OK;
}

// what table entry k takes from scratch and from the arena (hr_step_memory.h): the need, the budget's record and the carve all ask here
static SegmentBytes segmentBytesOf(const hr_ctx *c, const StepPlan &S, int k)
{
    const hr_ctx::PassSlot &ps = c->slots[S.order[k]];
    return segmentBytes(S.P, S.boundIn[k], S.kS, hitRecordSize(), ps.step == 0, tracesClosest(c, ps));
}
// stage 5: the step's bytes, what the memory budget learns from them, and regions that hold them.  Out of device memory: the injection
// is taken back, so that a later call — after the caller has released memory — finds the pipeline as this one did.
static int sizeStepMemory(hr_ctx *c, StepPlan &S)
{
    hr_ctx::Group &G = *S.G;
    S.needArena = S.needScratch = 0;
    for (int k = 0; k < S.n; ++k) {
        const SegmentBytes b = segmentBytesOf(c, S, k);
        S.needScratch += b.scratch, S.needArena += b.arena;
    }
    if (c->memBudget) { // what this step carves per pass and stage (budgetBytesPerPass)
        double sumA[kMaxBounceSlots] = {0}, sumS[kMaxBounceSlots] = {0};
        int cnt[kMaxBounceSlots] = {0};
        for (int k = 0; k < S.n; ++k) {
            const int step = c->slots[S.order[k]].step, st = step < kMaxBounceSlots ? step : kMaxBounceSlots - 1;
            const SegmentBytes b = segmentBytesOf(c, S, k);
            cnt[st]++;
            sumS[st] += (double)b.scratch, sumA[st] += (double)b.arena;
        }
        for (int st = 0; st < kMaxBounceSlots; ++st)
            if (cnt[st]) c->budgetSeen.record(st, sumA[st] / cnt[st], sumS[st] / cnt[st]);
    }
    G.arenaHighWater = S.needArena > G.arenaHighWater ? S.needArena : G.arenaHighWater;
    int rc = ensureRegion(c, G, G.arena[S.stepIdx & 1ull], G.arenaHighWater, "rays emitted by a step");
    if (rc == HR_OK) rc = ensureRegion(c, G, G.scratch, S.needScratch, "camera rays and hit records of a step");
    if (rc) takeBackInjection(c, S);
    return rc;
}

// stage 6: the step table — every entry's queues carved out of the step's memory, its counters, its pass
static int buildTable(hr_ctx *c, StepPlan &S)
{
    hr_ctx::Group &G = *S.G;
    hr_ctx::Group::Region &arena = G.arena[S.stepIdx & 1ull];
    char *pArena = arena.base, *pScratch = G.scratch.base;
    StepTable &tbl = G.hTables[S.ring];
    const int n = S.n;
    std::memset(tbl.heads, 0, sizeof(tbl.heads));
    std::memset(tbl.clkStart, 0xFF, sizeof(tbl.clkStart)), std::memset(tbl.clkEnd, 0, sizeof(tbl.clkEnd));
    tbl.headsLog2 = (uint32_t)c->tune.heads;
    tbl.nSeg = n;
    tbl.refillLanes = c->tune.refill, tbl.triPhaseLanes = c->tune.tri;
    tbl.fetchMax = c->tune.fmax, tbl.fetchMin = c->tune.fmin;
    tbl.staticPerWave = c->tune.sdeal, tbl.hasGlass = c->hasGlass ? 1 : 0;
    tbl.primaryFromSeg = n, tbl.fetchMaxPrimary = (c->tune.fprim & 0xFFFF) | ((c->tune.fgate & 0xFFFF) << 16); // (primaryFromSeg is set below, once the injected passes' places in the table are known)
    for (int k = 0; k < n; ++k) { // the carve: nothing but the table is written yet
        const hr_ctx::PassSlot &ps = c->slots[S.order[k]];
        SegDev &sg = tbl.seg[k];
        const int st = ps.step;
        const uint32_t bound = S.boundIn[k];
        sg.qin = st == 0 ? carveRayQueue(pScratch, S.P) : ps.qcur; // (a new pass's camera rays live for this step only)
        sg.sqIn = ps.scur;                                         // (nothing to trace there in a pass's first step: sCountIn is the zero word)
        sg.qinCap = st == 0 ? S.P : ps.capCur, sg.sInCap = st == 0 ? 0u : ps.sCapCur, sg.sOutCap = 0u;
        sg.qout = RayQueue{}, sg.sqOut = ShadowQueue{}, sg.hits = nullptr, sg.hitIdx = nullptr;
        sg.closestEnabled = tracesClosest(c, ps) ? 1 : 0;
        if (sg.closestEnabled) {
            sg.hits = (HitRec *)pScratch, pScratch += align256((size_t)bound * hitRecordSize());
            sg.hitIdx = (uint32_t *)pScratch, pScratch += align256((size_t)bound * kHitListEntryBytes);
            sg.qout = carveRayQueue(pArena, bound);
            sg.sqOut = carveShadowQueue(pArena, (size_t)bound * S.kS);
            sg.sOutCap = (uint32_t)((size_t)bound * S.kS);
            if (c->tune.ovf == 3 && st == 0) sg.sOutCap = sg.sOutCap / 8u + 1u; // TEST ONLY: the first hits' occlusion rays do not fit
        }
        sg.hitCap = sg.closestEnabled ? bound : 0u; // (capacity of hits, the hit list and qout: what was carved above)
    }
    // both cursors advanced by what sizeStepMemory provided for, or a kernel of this step would write past a region
    const size_t carved[2] = {(size_t)(pArena - arena.base), (size_t)(pScratch - G.scratch.base)}, sized[2] = {S.needArena, S.needScratch};
    for (int r = 0; r < 2; ++r)
        if (carved[r] != sized[r]) {
            takeBackInjection(c, S);
            FAIL(c, HR_ERR_DEVICE, "internal: a step carved " + std::to_string(carved[r]) + " bytes of " + (r ? "scratch" : "the step arena") + " but sized " + std::to_string(sized[r]));
        }
    S.nInjectedSegs = 0;
    for (int k = 0; k < n; ++k) {
        hr_ctx::PassSlot &ps = c->slots[S.order[k]];
        SegDev &sg = tbl.seg[k];
        const int st = ps.step;
        if (sg.closestEnabled) ps.qcur = sg.qout, ps.scur = sg.sqOut, ps.capCur = S.boundIn[k], ps.sCapCur = sg.sOutCap;
        sg.passbuf = ps.passbuf;
        sg.passbufB = ps.pp.estimator == HR_ESTIMATOR_ALL_LIGHTS ? ps.passbufB : nullptr;
        sg.aov = ps.aov;
        // The per-stage counters are a ring: a chain of pass-through rays (stacked single-sided sheets seen from behind, alpha holes:
        // physicallyBased.rlsl:70-108 re-emits without a depth bound) can outlive any fixed number of stages, so from stage
        // kMaxBounceSlots - 1 on the entries this step appends to are cleared first (their previous use lies a whole ring back).
        const int R = kMaxBounceSlots;
        if (st + 1 >= R) {
            HIP_TRY(c, hipMemsetAsync(&ps.ctr->qCount[(st + 1) % R], 0, sizeof(uint32_t), G.stream));
            if (st >= R) {
                HIP_TRY(c, hipMemsetAsync(&ps.ctr->sCount[st % R], 0, sizeof(uint32_t), G.stream));
                HIP_TRY(c, hipMemsetAsync(&ps.ctr->pCount[st % R], 0, sizeof(uint32_t), G.stream));
                HIP_TRY(c, hipMemsetAsync(&ps.ctr->gCount[st % R], 0, sizeof(uint32_t), G.stream));
            }
        }
        sg.qCountIn = &ps.ctr->qCount[st % R];
        sg.sCountIn = st > 0 ? &ps.ctr->sCount[(st - 1) % R] : c->dZero;
        sg.qCountOut = &ps.ctr->qCount[(st + 1) % R];
        sg.sCountOut = &ps.ctr->sCount[st % R];
        sg.pCount = &ps.ctr->pCount[st % R], sg.gCount = &ps.ctr->gCount[st % R];
        sg.listed = 0, sg.packets = 0;
        sg.pp = ps.pp;
        G.countSlot[S.ring][k] = S.order[k], G.countOrder[S.ring][k] = ps.order + 1ull;
        for (int j = 0; j < S.nInjected; ++j)
            if (S.order[k] == S.injectedSlots[j]) S.injectedSegs[S.nInjectedSegs++] = k;
    }
    if (S.nInjectedSegs > 0) tbl.primaryFromSeg = S.injectedSegs[0]; // (the table is in pass order: the passes injected now are its last entries)
    G.countN[S.ring] = n;
    tbl.hostCounts = G.dCounts + (size_t)S.ring * kMaxSegs, tbl.hostSeq = G.dSeq + S.ring, tbl.seqValue = S.stepIdx + 1ull;
    tbl.stepLog = c->dStepLog, tbl.nInjectedNow = (uint32_t)S.nInjected, tbl.group = (uint32_t)S.g;
    tbl.hostOverflow = c->dOverflowHost;
    return HR_OK;
}

// stage 7, the packet selector (hr_ctx::PacketSelector): do the injected passes' camera rays travel as packets (k_raygen_packets), beside
// k_trace or in front of it, and does this step carry a probe?  One decision per step: the table is copied before the launches are put together.
static void decidePackets(hr_ctx *c, StepPlan &S)
{
    hr_ctx::PacketSelector &sel = c->selector;
    StepTable &tbl = S.G->hTables[S.ring];
    const hr_pass_params *first = S.nInjectedSegs > 0 ? &tbl.seg[S.injectedSegs[0]].pp : nullptr;
    S.packetsNow = sel.packetsInUse(c->tune) && first && first->interactive_mode == 0; // (interactive sub-passes of one sample share no pixels)
    S.probeSeg = (S.g == 0 && first && sel.wantsProbe(*first, c->tune)) ? S.injectedSegs[0] : -1;
    S.corunNow = S.packetsNow && (c->tune.corun == 2 || (c->tune.corun == 1 && sel.lastOwnPerRay >= (double)c->tune.cmin));
    S.anyLens = false;
    for (int j = 0; j < S.nInjectedSegs; ++j) S.anyLens = S.anyLens || tbl.seg[S.injectedSegs[j]].pp.aperture_radius > 1e-30f;
    for (int j = 0; j < S.nInjectedSegs && S.packetsNow; ++j) {
        SegDev &sg = tbl.seg[S.injectedSegs[j]];
        sg.packets = S.corunNow ? 2 : 1;
        if (!S.anyLens || S.cfg.collectStats) sg.listed = 1; // (the kernels with the endings: hr_raygen.hip, launchRaygenPackets)
    }
    tbl.hostCameraCount = S.corunNow ? S.G->dCounts + (size_t)kTableRing * kMaxSegs : nullptr;
    tbl.probe = sel.dProbe, tbl.hostProbe = (S.g == 0 && (sel.probePending || S.probeSeg >= 0)) ? S.G->dProbeHost + 8 * S.ring : nullptr; // (reported only while a probe is awaited)
}

// stage 8a: one launch for the passes injected this step
// (as packets: ray generation and the camera rays' traversal in one launch per group of 16, 8, 4, 2, 1 passes — the bucket
// HR_KERNEL_RAYGEN then holds both, HR_KERNEL_TRACE and the step's device clock stay k_trace's own)
static int launchCameraRays(hr_ctx *c, const StepPlan &S, bool &timing, bool &forked)
{
    hr_ctx::Group &G = *S.G;
    const StepTable &tbl = G.hTables[S.ring];
    StepTable *dTbl = G.dTables + S.ring;
    for (int j0 = 0; j0 < S.nInjectedSegs;) {
        int take = 1;
        if (S.packetsNow)
            while (2 * take <= S.nInjectedSegs - j0 && 2 * take <= kMaxBatch) take *= 2;
        else
            take = S.nInjectedSegs - j0 < kMaxBatch ? S.nInjectedSegs - j0 : kMaxBatch;
        SegList segs{};
        for (int j = j0; j < j0 + take; ++j) segs.seg[segs.n++] = S.injectedSegs[j];
        j0 += take;
        bool uniformParams = S.packetsNow;
        for (int j = 1; j < segs.n && uniformParams; ++j) { // (the usual batch: one camera, one set of options, consecutive sample indices)
            hr_pass_params a = tbl.seg[segs.seg[0]].pp, b = tbl.seg[segs.seg[j]].pp;
            a.sample_index = b.sample_index = 0;
            uniformParams = std::memcmp(&a, &b, sizeof(a)) == 0;
        }
        LaunchCfg cfgP = S.cfg; // (a step with a lens: none of its packets has one origin, none can take the interval step)
        if (S.anyLens) cfgP.packetStep = 0, cfgP.packetLens = true; // (k_raygen_packets_rays<.., false>, whose hits k_shade_sort lists: `listed` above)
        if (S.corunNow) { // beside k_trace: fork after the table copy, join before the shading kernels
            LaunchCfg cb = cfgP;
            cb.stream = G.streamB;
            if (!forked) {
                HIP_TRY(c, hipEventRecord(G.evFork, G.stream));
                HIP_TRY(c, hipStreamWaitEvent(G.streamB, G.evFork, 0));
                forked = true;
            }
            launchRaygenPackets(cb, c->dScene, c->nodes, c->tris, dTbl, segs, S.fr, c->dStats, uniformParams);
            continue;
        }
        if (timing)
            c->timeNext(HR_KERNEL_RAYGEN, G.stream);
        else
            c->timeBegin(HR_KERNEL_RAYGEN, G.stream);
        timing = true;
        if (S.packetsNow)
            launchRaygenPackets(cfgP, c->dScene, c->nodes, c->tris, dTbl, segs, S.fr, c->dStats, uniformParams);
        else
            launchRaygen(S.cfg, c->dScene, dTbl, segs, S.fr, c->dStats);
    }
    if (forked) HIP_TRY(c, hipEventRecord(G.evJoin, G.streamB));
    return HR_OK;
}
// stage 8b: the step's probe, on the selector's side stream
static int launchProbe(hr_ctx *c, const StepPlan &S)
{
    hr_ctx::PacketSelector &sel = c->selector;
    // (probeSeen holds the totals of the report the previous decision was taken on: probes never overlap, that probe was complete)
    HIP_TRY(c, hipEventRecord(sel.evProbeA, S.G->stream));
    HIP_TRY(c, hipStreamWaitEvent(sel.probeStream, sel.evProbeA, 0));
    sel.probeWaves = (unsigned long long)launchPacketProbe(sel.probeStream, c->dScene, c->nodes, c->tris, S.G->hTables[S.ring].seg[S.probeSeg].pp, c->tune.plog >= 0 ? c->tune.plog : hr_ctx::PacketSelector::packetLog2(c->injectBatch), S.fr, sel.dProbe, c->tune.pprobe != 0);
    HIP_TRY(c, hipEventRecord(sel.evProbeB, sel.probeStream));
    sel.probeGuard = true, sel.probePending = true, sel.probeStep = S.stepIdx, sel.probeCountdown = hr_ctx::PacketSelector::kProbeEvery;
    return HR_OK;
}
// k_trace's workgroups per CU while the step's packet kernel runs beside it: the camera rays of this step (what the passes injected before
// sent through the root cull, or half the pixels while unknown) against the rays k_trace carries (two per entry of the closest-hit
// queues' bounds: the ray and its occlusion ray)
static int corunTraceBlocks(hr_ctx *c, const StepPlan &S)
{
    uint32_t &lastCameraCount = c->selector.lastCameraCount;
    double others = 0.0;
    for (int k = 0; k < S.n; ++k)
        if (c->slots[S.order[k]].step > 0) others += 2.0 * (double)((c->slots[S.order[k]].step == 1 && lastCameraCount && S.boundIn[k] > lastCameraCount) ? lastCameraCount : S.boundIn[k]);
    const uint32_t late = ((volatile uint32_t *)S.G->hCounts)[(size_t)kTableRing * kMaxSegs]; // (k_shade_sort's hint: camera rays per pass behind the root cull)
    if (late) lastCameraCount = late;
    const double cam = (double)S.nInjectedSegs * (double)(lastCameraCount ? lastCameraCount : S.P / 2u);
    const int blocks = cam > 0.2 * others ? 3 : 4;
    return c->tune.cblocks > 0 ? c->tune.cblocks : blocks;
}
// stage 8: the launches — table fetch, camera rays, probe, k_trace, shading — and their timing buckets
static int launchStep(hr_ctx *c, const StepPlan &S, StepClock &clk)
{
    hr_ctx::Group &G = *S.G;
    StepTable *dTbl = G.dTables + S.ring;
    const size_t tblBytes = offsetof(StepTable, seg) + (size_t)S.n * sizeof(SegDev);
    launchFetchTable(G.stream, G.dTablesHost + S.ring, dTbl, (tblBytes + 15) & ~(size_t)15);
    clk.mark();
    HIP_TRY(c, hipEventRecord(G.tableCopied[S.ring], G.stream));
    G.tableUsed[S.ring] = true;
    if (c->pending.size() > 8192) c->drainTimes();
    bool timing = false; // (the kernels of a step are enqueued back to back: n + 1 timing events for n kernels)
    bool forked = false;
    int rc = launchCameraRays(c, S, timing, forked);
    if (rc) return rc;
    if (timing)
        c->timeNext(HR_KERNEL_TRACE, G.stream);
    else
        c->timeBegin(HR_KERNEL_TRACE, G.stream);
    if (S.probeSeg >= 0) {
        rc = launchProbe(c, S);
        if (rc) return rc;
    }
    LaunchCfg ct = S.cfg;
    if (forked) {
        const int blocks = corunTraceBlocks(c, S);
        if (blocks < ct.traceBlocksPerCU) ct.traceBlocksPerCU = blocks;
    }
    launchTrace(ct, c->dScene, c->tree.leafKeys, c->tree.nodes32, c->tris, dTbl, c->dStats);
    if (forked) { // (the bucket HR_KERNEL_TRACE stays k_trace's own launch; what the packet kernel beside it runs longer is booked as ray generation)
        c->timeNext(HR_KERNEL_RAYGEN, G.stream);
        HIP_TRY(c, hipStreamWaitEvent(G.stream, G.evJoin, 0));
    }
    c->timeNext(HR_KERNEL_SHADE, G.stream);
    launchShade(S.cfg, c->dScene, dTbl, c->dStats);
    c->timeEnd(G.stream);
    return HR_OK;
}

// stage 9: every pass is a stage further or, past its last, finished; in pass-through scenes the snapshot endDrainedPassthrough reads
static int advancePasses(hr_ctx *c, const StepPlan &S)
{
    hr_ctx::Group &G = *S.G;
    hr_ctx::PassSlot *ended[kMaxSegs];
    int nEnded = 0;
    for (int k = 0; k < S.n; ++k) {
        hr_ctx::PassSlot &ps = c->slots[S.order[k]];
        if (!c->hasPassthrough && ps.step >= ps.nIter) {
            ps.active = false, ps.finished = true;
            ended[nEnded++] = &ps;
        } else {
            ps.step++;
        }
    }
    if (nEnded > 0) HIP_TRY(c, hipEventRecord(ended[nEnded - 1]->evFinal, G.stream)); // one event for the passes whose last stage this step was
    for (int k = 0; k < nEnded; ++k) ended[k]->finalEv = ended[nEnded - 1]->evFinal;
    if (c->hasPassthrough) { // snapshot of the queue lengths after this step, read two steps from now
        uint32_t *dst = G.hQCount + (size_t)S.ring * kMaxSlots * kMaxBounceSlots;
        HIP_TRY(c, hipMemcpy2DAsync(dst, sizeof(uint32_t) * kMaxBounceSlots, &c->dCounters[0].qCount[0], sizeof(Counters),
                                    sizeof(uint32_t) * kMaxBounceSlots, kMaxSlots, hipMemcpyDeviceToHost, G.stream));
        HIP_TRY(c, hipEventRecord(G.statusEv[S.ring], G.stream));
        G.statusUsed[S.ring] = true;
        for (int i = 0; i < kMaxSlots; ++i)
            G.statusOrder[S.ring][i] = (c->slots[i].active && c->slots[i].group == S.g) ? c->slots[i].order + 1ull : 0ull;
    }
    return HR_OK;
}

static int macroStep(hr_ctx *c, int g, int nInject)
{
    StepClock clk{c->tune.debugStepTimes, {0, 0, 0, 0, 0}, 0};
    clk.mark();
    StepPlan S;
    hr_ctx::Group &G = c->groups[g];
    S.g = g, S.G = &G;
    S.cfg = c->cfg(G.stream);
    S.fr = c->frame, S.fr.fb = c->fb();
    int rc = injectPasses(c, S, nInject);
    if (rc == HR_OK) rc = endDrainedPassthrough(c, S);
    if (rc) return rc;
    clk.mark();
    listInFlight(c, S);
    if (S.n == 0) return resolveReady(c);
    if (S.n > kMaxSegs) FAIL(c, HR_ERR_INVALID, "internal: too many passes in one group");
    S.stepIdx = G.stepCounter++;
    S.ring = (int)(S.stepIdx % kTableRing);
    if (G.tableUsed[S.ring]) HIP_TRY(c, hipEventSynchronize(G.tableCopied[S.ring])); // staging entry free again (4 steps old)
    S.P = c->tune.ovf == 1 ? c->queueCapacity / 8u + 1u : (c->queueCapacity ? c->queueCapacity : 1u); // (ovf=1, TEST ONLY: camera rays do not fit)
    S.kS = c->allLightsUsed ? 4 : 1;
    rc = boundQueues(c, S);
    if (rc) return rc;
    clk.mark();
    rc = sizeStepMemory(c, S);
    if (rc == HR_OK) rc = buildTable(c, S);
    if (rc) return rc;
    decidePackets(c, S);
    clk.mark();
    rc = launchStep(c, S, clk);
    if (rc == HR_OK) rc = advancePasses(c, S);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    clk.print(S.stepIdx, nInject);
    return resolveReady(c);
}

// Stages a pass occupies in the pipeline (depth+1 shaded stages + the last occlusion stage; in pass-through scenes two more
// until the host has seen that its queue ran empty — longer only for rays that really pass through surfaces).
static int stagesOf(const hr_ctx *c, const hr_pass_params &pp) { return pp.max_ray_depth + 2 + (c->hasPassthrough ? 2 : 0); }

// Advance the group that holds the oldest in-flight pass by one macro step (keeps passes finishing in order).
static int stepOldest(hr_ctx *c)
{
    const hr_ctx::PassSlot *oldest = nullptr;
    for (const hr_ctx::PassSlot &ps : c->slots)
        if (ps.active && (!oldest || ps.order < oldest->order)) oldest = &ps;
    if (!oldest) return resolveReady(c);
    return macroStep(c, oldest->group, 0);
}

static int slotLimit(const hr_ctx *c) { return c->maxSlots < c->tune.depth ? c->maxSlots : c->tune.depth; } // passes in flight, all groups (both within 1..kMaxSlots)

// Inject n pending passes into the next group (round robin), first making room for them.
static int injectBatch(hr_ctx *c, int n, int perGroupLimit)
{
    const int g = c->nextGroup;
    c->nextGroup = (g + 1) % c->nGroups;
    int guard = 0;
    while ((occupiedSlots(c, g) + n > perGroupLimit || occupiedSlots(c) + n > slotLimit(c)) && occupiedSlots(c) > 0) {
        int rc = stepOldest(c);
        if (rc) return rc;
        if (++guard > 64 * kMaxBounceSlots) FAIL(c, HR_ERR_DEVICE, "internal: pass pipeline did not make room");
    }
    return macroStep(c, g, n);
}

// hr_ctx_desc::memory_budget: how many passes per step fit.  A pass of the batch holds, over the `stages` steps of its life, a pass buffer
// (S + 2 of them per batch pass are kept: the pipeline's depth and the resolve lag), its camera rays and hit records (scratch), and
// what each of its closest-hit stages emits (arena: two halves, each with a third of headroom).  A stage that has not been seen yet
// counts as long as it can possibly get (one ray per owned pixel: the guarantee); a stage that has, by the largest per-pass average a
// step carved for it, plus a tenth.  All stages of a batch are in flight at once (one generation per stage), so the sum over the
// stages is what one more pass per step costs.
static double budgetBytesPerPass(const hr_ctx *c, int stages)
{
    const double P = (double)(c->queueCapacity ? c->queueCapacity : 1u), kS = c->allLightsUsed ? 4.0 : 1.0;
    const double fb = (double)c->W * c->H * 16.0 * ((c->allLightsUsed ? 4.0 : 1.0) + (double)c->aov.framesPerSlot());
    double arena = 0.0, scratch = 0.0;
    for (int st = 0; st + 1 < stages && st < kMaxBounceSlots; ++st) { // (the last stage traces occlusion rays only)
        const hr_ctx::BudgetSeen &seen = c->budgetSeen; // (the guarantee: unaligned and in double, hr_step_memory.h)
        arena += seen.stageSeen[st] ? 1.1 * seen.stageArenaSeen[st] : guaranteedArenaBytes(P, kS);
        scratch += seen.stageSeen[st] ? 1.1 * seen.stageScratchSeen[st] : guaranteedScratchBytes(P, hitRecordSize(), st == 0);
    }
    return (double)c->nGroups * ((double)(stages + 2) * fb + (4.0 / 3.0) * (2.0 * arena + scratch));
}
static int budgetBatch(const hr_ctx *c, int stages)
{
    if (!c->memBudget) return 1 << 20;
    const double fit = (double)c->memBudget / budgetBytesPerPass(c, stages);
    return fit < 1.0 ? 1 : (fit > 1e6 ? 1 << 20 : (int)fit);
}

static int batchFor(const hr_ctx *c, int stages)
{
    int batch = c->selector.packetsInUse(c->tune) ? hr_ctx::PacketSelector::packetBatch(c->injectBatch) : c->injectBatch;
    const int fit = budgetBatch(c, stages);
    if (batch > fit) {
        batch = fit;
        if (c->selector.packetsInUse(c->tune)) // (a packet holds a power of two of passes)
            while (batch & (batch - 1)) batch &= batch - 1;
    }
    int perGroup = slotLimit(c) / c->nGroups;
    if (perGroup > kMaxSegs) perGroup = kMaxSegs;
    if (batch * stages > perGroup) batch = perGroup / stages;
    return batch < 1 ? 1 : batch;
}

static int drainPipeline(hr_ctx *c)
{
    while (!c->pendingInject.empty()) {
        const int stages = stagesOf(c, c->pendingInject.front());
        const int batch = batchFor(c, stages);
        int n = (int)c->pendingInject.size() < batch ? (int)c->pendingInject.size() : batch;
        // the last, partly filled batch of a run on several pipeline groups is dealt out over the groups (each group's dependent
        // chain of stages then carries a share of it, and the chains overlap on the device) instead of going to one of them whole
        if (c->nGroups > 1 && (int)c->pendingInject.size() <= batch) {
            const int idleGroups = c->nGroups - (c->nextGroup % c->nGroups);
            const int share = ((int)c->pendingInject.size() + idleGroups - 1) / (idleGroups > 0 ? idleGroups : 1);
            n = share < 1 ? 1 : share;
        }
        // With the camera rays as packets a step injects WHOLE launches of kMaxBatch passes where it can: a remainder goes in one step later,
        // where its (smaller, less coherent) packets run beside the k_trace that carries the first launches' first bounce instead of
        // lengthening the step that has nothing beside it.  A 1/8 shard's 20 passes as 16, then 4: 0.304 -> 0.294 ms/step; as 12 + 8,
        // 10 + 10, 8 + 8 + 4 (each of them smaller packets all round): 0.307 - 0.323 (profiles/r5g_burst_pmin.txt).
        if (c->selector.packetsInUse(c->tune) && n > kMaxBatch && n % kMaxBatch) n -= n % kMaxBatch;
        int perGroup = batch * stages;
        int rc = injectBatch(c, n, perGroup);
        if (rc) return rc;
    }
    int guard = 0;
    while (activePasses(c) > 0) {
        int rc = stepOldest(c);
        if (rc) return rc;
        if (++guard > 64 * kMaxBounceSlots) FAIL(c, HR_ERR_DEVICE, "internal: pass pipeline did not drain");
    }
    int rc = resolveReady(c);
    if (rc) return rc;
    if (occupiedSlots(c) > 0) FAIL(c, HR_ERR_DEVICE, "internal: finished passes left unresolved");
    c->oldestWaitingNs = 0;
    if (c->selector.probeGuard) { // (a probe nobody has waited for: whatever follows on the caller's stream — frees after a synchronise included — comes after it)
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->selector.evProbeB, 0));
        c->selector.probeGuard = false;
    }
    // whatever the caller does next on its stream (clear, scene edits, new tables) has to be seen by the groups
    for (int g = 0; g < kMaxGroups; ++g) c->groups[g].needUserSync = true;
    return HR_OK;
}

int hr_render_pass(hr_ctx *c, const hr_pass_params *pp)
{
    ENTER(c);
    if (c->grp) return groupRenderPass(c, pp);
    if (!pp) FAIL(c, HR_ERR_INVALID, "null params");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    if (!c->committed) FAIL(c, HR_ERR_INVALID, "scene not committed");
    if (c->nSeq <= 0 || c->nSeqOffsets <= 0) FAIL(c, HR_ERR_INVALID, "sample tables not set");
    if (pp->max_ray_depth < 0 || pp->max_ray_depth + 2 >= kMaxBounceSlots - 8) FAIL(c, HR_ERR_INVALID, "max_ray_depth out of range");
    if (pp->interactive_mode && (pp->block_size[0] <= 0 || pp->block_size[1] <= 0)) FAIL(c, HR_ERR_INVALID, "bad block size");
    int rc = HR_OK;
    if (pp->estimator == HR_ESTIMATOR_ENV_MIS || pp->estimator == HR_ESTIMATOR_ALL_LIGHTS) {
        rc = ensureEnvTable(c);
        if (rc) return rc;
        if (pp->estimator == HR_ESTIMATOR_ALL_LIGHTS && !c->allLightsUsed) {
            // pass slots grow (a second occlusion ray per path, a second partial sum per pass): the existing ones are released and
            // re-allocated below with the new sizes
            rc = drainPipeline(c);
            if (rc) return rc;
            QUIESCE(c);
            const uint32_t keepCap = c->queueCapacity;
            freeQueues(c);
            c->queueCapacity = keepCap;
            c->allLightsUsed = true;
            slotBudget(c);
        }
    } else if (pp->estimator != HR_ESTIMATOR_REFERENCE) {
        FAIL(c, HR_ERR_INVALID, "unknown estimator");
    }
    if (pp->texture_lod == HR_TEXTURE_LOD_CONE) {
        rc = ensureTextureLod(c);
        if (rc) return rc;
        c->textureLodUsed = true;
    } else if (pp->texture_lod != HR_TEXTURE_LOD_BASE) {
        FAIL(c, HR_ERR_INVALID, "unknown texture_lod mode");
    }
    rc = uploadScene(c); // drains the pipeline first when the scene constants changed
    if (rc) return rc;
    if (c->frame.nOwnedTiles == 0) return HR_OK;
    // only passes of equal depth overlap (keeps the groups in lockstep; order is enforced by resolveReady regardless)
    if (pp->max_ray_depth != c->lastDepth && (occupiedSlots(c) > 0 || !c->pendingInject.empty())) {
        rc = drainPipeline(c);
        if (rc) return rc;
    }
    c->lastDepth = pp->max_ray_depth;
    if (c->memBudget && (double)c->memBudget < budgetBytesPerPass(c, stagesOf(c, *pp))) {
        c->err = "hr_ctx_desc.memory_budget (" + std::to_string(c->memBudget >> 20) + " MiB) is less than one pass per pipeline step needs at " + std::to_string(c->W) + "x" +
                 std::to_string(c->H) + ", depth " + std::to_string(pp->max_ray_depth) + ": " + std::to_string((unsigned long long)budgetBytesPerPass(c, stagesOf(c, *pp)) >> 20) + " MiB";
        return HR_ERR_INVALID;
    }
    {
        // All pass slots this depth needs are allocated up front, on the first pass (hipMalloc synchronises the device and
        // takes ~0.1 ms per buffer: allocating slot by slot as the pipeline filled stalled the first 20-odd passes of a render)
        const int stagesNow = stagesOf(c, *pp);
        const int batchNow = batchFor(c, stagesNow);
        int want = c->nGroups * batchNow * stagesNow + 2 * c->nGroups * batchNow;
        if (want > slotLimit(c)) want = slotLimit(c);
        for (int i = 0; i < kMaxSlots && c->nSlotsAllocated < want; ++i)
            if (!c->slots[i].allocated) {
                rc = allocSlot(c, c->slots[i], c->stream);
                if (rc) return rc;
            }
    }
    c->pendingInject.push_back(*pp);
    if (c->oldestWaitingNs == 0)
        c->oldestWaitingNs = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    // a macro step is launched once enough passes are waiting to fill it; each group holds batch x stages passes
    const int stages = stagesOf(c, *pp);
    const int batch = batchFor(c, stages);
    if ((int)c->pendingInject.size() < batch) return HR_OK;
    return injectBatch(c, batch, batch * stages);
}

int hr_frame_pass_batch(hr_ctx *c, int32_t max_ray_depth, int32_t *batch)
{
    ENTER(c);
    if (c->grp) return groupOne(c, 0, [&](hr_ctx *m) { return hr_frame_pass_batch(m, max_ray_depth, batch); });
    if (!batch || max_ray_depth < 0) FAIL(c, HR_ERR_INVALID, "bad arguments");
    if (c->W <= 0) FAIL(c, HR_ERR_INVALID, "no frame");
    hr_pass_params pp{};
    pp.max_ray_depth = max_ray_depth;
    *batch = batchFor(c, stagesOf(c, pp));
    return HR_OK;
}

int hr_flush(hr_ctx *c)
{
    ENTER(c);
    if (c->grp) return groupSync(c, false);
    const int rc = drainPipeline(c);
    return rc ? rc : overflowCheck(c); // (no wait here: what the kernels have reported so far)
}

int hr_get_stats(hr_ctx *c, hr_pass_stats *out)
{
    ENTER(c);
    if (c->grp) return groupStats(c, out);
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    {
        int rc = drainPipeline(c);
        if (rc) return rc;
    }
    std::vector<Stats> parts(kStatSlots);
    HIP_TRY(c, hipMemcpyAsync(parts.data(), c->dStats, sizeof(Stats) * kStatSlots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    {
        const int rc = overflowCheck(c);
        if (rc) return rc;
    }
    Stats s{};
    for (const Stats &p : parts) {
        s.paths += p.paths, s.raysClosest += p.raysClosest, s.raysAny += p.raysAny, s.shadedHits += p.shadedHits;
        s.accumulates += p.accumulates, s.nodeVisits += p.nodeVisits, s.triTests += p.triTests;
        s.nodeVisitsAny += p.nodeVisitsAny, s.triTestsAny += p.triTestsAny;
    }
    std::memset(out, 0, sizeof(*out));
    out->paths = s.paths, out->rays_closest = s.raysClosest, out->rays_any = s.raysAny, out->shaded_hits = s.shadedHits;
    out->accumulates = s.accumulates, out->node_visits = s.nodeVisits, out->tri_tests = s.triTests;
    out->node_visits_any = s.nodeVisitsAny, out->tri_tests_any = s.triTestsAny;
    return HR_OK;
}

int hr_get_kernel_times(hr_ctx *c, hr_kernel_times *out)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_get_kernel_times");
    if (!out) FAIL(c, HR_ERR_INVALID, "null output");
    {
        int rc = drainPipeline(c);
        if (rc) return rc;
    }
    c->drainTimes();
    for (int k = 0; k < HR_KERNEL_COUNT; ++k) out->ms[k] = c->kernelMs[k], out->launches[k] = c->kernelLaunches[k];
    std::vector<Stats> parts(kStatSlots);
    HIP_TRY(c, hipMemcpyAsync(parts.data(), c->dStats, sizeof(Stats) * kStatSlots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long ticks = 0, launches = 0;
    for (const Stats &p : parts) ticks += p.traceTicks, launches += p.traceLaunches;
    out->trace_clock_ms = (float)((double)ticks * 1e-5); // 100 MHz: 10 ns per tick
    out->trace_clock_launches = (uint32_t)launches;
    out->camera_packets = c->selector.packetsInUse(c->tune) ? (uint32_t)hr_ctx::PacketSelector::packetBatch(c->injectBatch) : 0u;
    out->packet_union = (float)c->selector.lastUnion;
    return HR_OK;
}

int hr_get_step_log(hr_ctx *c, hr_step_record *out, int32_t capacity, int32_t *n_records)
{
    ENTER(c);
    if (c->grp) return groupUnsupported(c, "hr_get_step_log");
    if (!out || !n_records || capacity <= 0) FAIL(c, HR_ERR_INVALID, "bad arguments");
    {
        int rc = drainPipeline(c);
        if (rc) return rc;
    }
    std::vector<Stats> parts(1);
    std::vector<unsigned long long> log(3 * (size_t)kStepLogCap);
    HIP_TRY(c, hipMemcpyAsync(parts.data(), c->dStats, sizeof(Stats), hipMemcpyDeviceToHost, c->stream)); // (k_shade_sort's first thread counts in the first copy)
    HIP_TRY(c, hipMemcpyAsync(log.data(), c->dStepLog, log.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long total = parts[0].traceLaunches;
    const unsigned long long first = total > (unsigned long long)kStepLogCap ? total - (unsigned long long)kStepLogCap : 0ull;
    // Records are appended when a step's k_trace has ENDED (k_shade_sort writes them), so with several pipeline groups they arrive out of
    // start order: they are handed out sorted by start, each with its group.
    std::vector<const unsigned long long *> recs;
    for (unsigned long long i = first; i < total; ++i) recs.push_back(&log[3 * (size_t)(i % (unsigned long long)kStepLogCap)]);
    std::stable_sort(recs.begin(), recs.end(), [](const unsigned long long *a, const unsigned long long *b) { return a[0] < b[0]; });
    int32_t n = 0;
    for (const unsigned long long *rec : recs) {
        if (n >= capacity) break;
        out[n].start_ms = (double)(rec[0] - recs[0][0]) * 1e-5; // 100 MHz device clock
        out[n].trace_ms = (float)((double)(rec[1] - rec[0]) * 1e-5);
        out[n].passes_in_flight = (int32_t)(rec[2] & 0xFFFFull), out[n].group = (int32_t)((rec[2] >> 16) & 0xFFull), out[n].passes_injected = (int32_t)(rec[2] >> 32);
        ++n;
    }
    *n_records = n;
    return HR_OK;
}

