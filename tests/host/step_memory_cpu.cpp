// heatray_amd/csrc/hr_step_memory.h on the CPU (tests/test_step_memory.py builds this with -fsanitize=address,undefined and runs it): the
// bytes a macro step takes from scratch and from the step arena, against the expressions the pipeline held before the header existed
// (restated literally below), against a walk of two cursors, and the memory budget's guarantee against its former constants.
// No input; prints "step memory cpu: ok" and returns 0 when every check holds.
#include "hr_step_memory.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

// the pipeline's own helpers and its need sum, as they stood
static size_t oldAlign256(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t oldRayQueueBytes(size_t cap) { return 4 * oldAlign256(cap * 16); }
static size_t oldShadowQueueBytes(size_t cap) { return 3 * oldAlign256(cap * 16); }
static void oldNeed(uint32_t P, uint32_t bound, size_t kS, size_t hitRecordSize, bool firstStep, bool closest, size_t &needScratch, size_t &needArena)
{
    if (firstStep) needScratch += oldRayQueueBytes(P);
    if (closest) {
        needScratch += oldAlign256((size_t)bound * hitRecordSize) + oldAlign256((size_t)bound * 4);
        needArena += oldRayQueueBytes(bound) + oldShadowQueueBytes((size_t)bound * kS);
    }
}

// the carve, plane by plane, as carveRayQueue / carveShadowQueue and the table loop of hr_pipeline.inl advance their cursors (offsets only)
static void walkQueue(size_t &p, size_t cap, size_t planes)
{
    for (size_t k = 0; k < planes; ++k) {
        CHECK(p % 256 == 0); // every plane starts aligned
        p += queuePlaneBytes(cap);
    }
}
static void walkSegment(size_t &pScratch, size_t &pArena, uint32_t P, uint32_t bound, size_t kS, size_t hitRecordSize, bool firstStep, bool closest)
{
    if (firstStep) walkQueue(pScratch, P, 4);
    if (closest) {
        pScratch += align256((size_t)bound * hitRecordSize);
        pScratch += align256((size_t)bound * 4);
        walkQueue(pArena, bound, 4);
        walkQueue(pArena, (size_t)bound * kS, 3);
    }
}

int main()
{
    const uint32_t bounds[] = {0u, 1u, 15u, 16u, 17u, 4095u, 4096u, 4097u, (1u << 20) + 1u};
    const uint32_t Ps[] = {1u, 16u, 2073600u};
    const size_t kSs[] = {1, 4};
    const size_t hitRec = 16;

    CHECK(kRayQueueBytesPerRay == 64 && kShadowQueueBytesPerRay == 48 && kHitListEntryBytes == 4);
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
    CHECK(queuePlaneBytes(16) == 256 && queuePlaneBytes(17) == 512);

    for (uint32_t P : Ps)
        for (size_t kS : kSs) {
            // one step table of every case of the grid: the sum of its entries against the walk of the two cursors
            size_t sumScratch = 0, sumArena = 0, pScratch = 0, pArena = 0;
            for (uint32_t bound : bounds)
                for (int first = 0; first < 2; ++first)
                    for (int closest = 0; closest < 2; ++closest) {
                        const SegmentBytes b = segmentBytes(P, bound, kS, hitRec, first != 0, closest != 0);
                        size_t oldScratch = 0, oldArena = 0;
                        oldNeed(P, bound, kS, hitRec, first != 0, closest != 0, oldScratch, oldArena);
                        if (b.scratch != oldScratch || b.arena != oldArena)
                            printf("P %u bound %u kS %zu first %d closest %d: (%zu, %zu), was (%zu, %zu)\n", P, bound, kS, first, closest, b.scratch, b.arena, oldScratch, oldArena), ++failures;
                        CHECK(b.scratch % 256 == 0 && b.arena % 256 == 0);
                        CHECK(rayQueueBytes(bound) == oldRayQueueBytes(bound) && shadowQueueBytes((size_t)bound * kS) == oldShadowQueueBytes((size_t)bound * kS));
                        sumScratch += b.scratch, sumArena += b.arena;
                        walkSegment(pScratch, pArena, P, bound, kS, hitRec, first != 0, closest != 0);
                    }
            CHECK(sumScratch == pScratch && sumArena == pArena && sumArena > 0);

            // the budget's guarantee for a stage not yet seen: the former constants, as doubles, exactly
            const double Pd = (double)P, kSd = kS == 4 ? 4.0 : 1.0;
            CHECK(guaranteedArenaBytes(Pd, kSd) == Pd * (64.0 + 48.0 * kSd));
            CHECK(guaranteedScratchBytes(Pd, hitRec, false) == Pd * 20.0);
            CHECK(guaranteedScratchBytes(Pd, hitRec, true) == Pd * 20.0 + Pd * 64.0);
        }
    if (failures) return printf("step memory cpu: %d checks failed\n", failures), 1;
    printf("step memory cpu: ok\n");
    return 0;
}
