// The owning handles of heatray_amd/csrc/hr_owned.h against a counting fake of the HIP calls they make (tests/host/fake_hip, first on
// the include path): every handle frees once, moves without copying, survives a self-move, guards the null handle; reserve is grow-only
// and leaves no size behind a failed allocation; an aggregate shaped like hr_ctx::Group leaks nothing whichever creation call fails.
// Built with AddressSanitizer and UBSan by tests/test_owned.py; ends with "owned cpu: ok".
#include "hr_owned.h"

#include <cstdint>
#include <cstdio>
#include <utility>

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static FakeHip &F = fakeHip();
static long liveOf(FakeHip::Kind k) { return (long)F.live[k].size(); }

// create / destroy / move / self-move / reset of one handle type; `make` creates into its argument
template <class H, class Make> static int lifeCycle(FakeHip::Kind kind, Make make)
{
    const long frees0 = F.frees[kind];
    {
        H a;
        CHECK(!a.get() && liveOf(kind) == 0);
        CHECK(make(a) == hipSuccess && a.get() && liveOf(kind) == 1);
    }
    CHECK(liveOf(kind) == 0 && F.frees[kind] == frees0 + 1); // create, then destroy
    {
        H a;
        CHECK(make(a) == hipSuccess);
        const auto raw = a.get();
        H b(std::move(a)); // move-construct: the resource changes owner, nothing is made or freed
        CHECK(!a.get() && b.get() == raw && liveOf(kind) == 1 && F.frees[kind] == frees0 + 1);
        H c;
        CHECK(make(c) == hipSuccess && liveOf(kind) == 2);
        const auto old = c.get();
        c = std::move(b); // move-assign over a live handle: the old resource is freed, exactly once and then
        CHECK(F.frees[kind] == frees0 + 2 && liveOf(kind) == 1 && !F.live[kind].count((void *)old));
        CHECK(c.get() == raw && !b.get());
        H &self = c;
        c = std::move(self); // self-move-assign
        CHECK(c.get() == raw && liveOf(kind) == 1 && F.frees[kind] == frees0 + 2);
        c.reset();
        CHECK(!c.get() && liveOf(kind) == 0 && F.frees[kind] == frees0 + 3);
        c.reset(); // ... of an empty handle: nothing
        CHECK(F.frees[kind] == frees0 + 3);
    }
    CHECK(liveOf(kind) == 0 && F.frees[kind] == frees0 + 3);
    {
        const long calls = F.calls;
        {
            H empty, other;
            other = std::move(empty);
            H third(std::move(other));
        }
        CHECK(F.calls == calls); // empty handles make no call at all (the fake aborts on a null host-free, event- or stream-destroy)
    }
    return 0;
}

static int handles()
{
    if (lifeCycle<DeviceBuf<float>>(FakeHip::Device, [](DeviceBuf<float> &b) { return b.alloc(16); })) return 1;
    if (lifeCycle<PinnedBuf<float>>(FakeHip::Host, [](PinnedBuf<float> &b) { return b.alloc(16); })) return 1;
    if (lifeCycle<PinnedBuf<volatile uint32_t>>(FakeHip::Host, [](PinnedBuf<volatile uint32_t> &b) { return b.alloc(4, hipHostMallocCoherent | hipHostMallocMapped); })) return 1;
    if (lifeCycle<Event>(FakeHip::Ev, [](Event &e) { return e.create(hipEventDisableTiming); })) return 1;
    if (lifeCycle<Stream>(FakeHip::St, [](Stream &s) { return s.create(hipStreamNonBlocking); })) return 1;

    // capacity and flags travel with a move; alloc over a live buffer frees it first
    DeviceBuf<float> d;
    CHECK(d.alloc(10) == hipSuccess && d.capacity() == 10);
    DeviceBuf<float> d2(std::move(d));
    CHECK(d.capacity() == 0 && d2.capacity() == 10);
    d = std::move(d2);
    CHECK(d.capacity() == 10 && d2.capacity() == 0 && !d2.get());
    CHECK(d.alloc(20) == hipSuccess && d.capacity() == 20 && liveOf(FakeHip::Device) == 1);
    // release(): the pointer is handed out and still live; the handle is empty and frees nothing
    float *raw = d.release();
    CHECK(raw && !d.get() && d.capacity() == 0 && liveOf(FakeHip::Device) == 1);
    d.reset();
    CHECK(liveOf(FakeHip::Device) == 1);
    CHECK(hipFree(raw) == hipSuccess && liveOf(FakeHip::Device) == 0);

    const unsigned spun = hipHostMallocCoherent | hipHostMallocMapped;
    PinnedBuf<volatile unsigned long long> p;
    CHECK(p.alloc(4, spun) == hipSuccess && p.flags() == spun && F.lastHostFlags == spun && p.capacity() == 4);
    unsigned long long *dev = nullptr;
    CHECK(p.devicePointer(&dev) == hipSuccess && (volatile unsigned long long *)dev == p.get());
    p[1] = 7ull; // the host writes and polls it through the handle
    CHECK(p[1] == 7ull);
    PinnedBuf<volatile unsigned long long> q;
    q = std::move(p);
    CHECK(q.flags() == spun && q.capacity() == 4 && p.capacity() == 0);
    CHECK(q.reserve(8) == hipSuccess && q.capacity() == 8 && F.lastHostFlags == spun && liveOf(FakeHip::Host) == 1); // grows with its flags
    PinnedBuf<float> plain;
    CHECK(plain.alloc(3) == hipSuccess && plain.flags() == hipHostMallocDefault && F.lastHostFlags == hipHostMallocDefault);

    Event e;
    CHECK(e.create() == hipSuccess && F.lastEventFlags == hipEventDefault);
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && F.lastEventFlags == hipEventDisableTiming && liveOf(FakeHip::Ev) == 1);
    Stream s;
    CHECK(s.createWithPriority(hipStreamNonBlocking, -1) == hipSuccess && F.lastStreamFlags == hipStreamNonBlocking && F.lastPriority == -1);
    hipStream_t asRaw = s; // a handle reads as its raw value
    CHECK(asRaw == s.get());
    return 0;
}

template <class Buf> static int reserveOf(FakeHip::Kind kind)
{
    Buf b;
    CHECK(b.reserve(100) == hipSuccess && b.capacity() == 100 && liveOf(kind) == 1);
    const auto raw = b.get();
    long calls = F.calls;
    CHECK(b.reserve(100) == hipSuccess && b.reserve(1) == hipSuccess && b.reserve(0) == hipSuccess);
    CHECK(F.calls == calls && b.get() == raw && b.capacity() == 100); // the capacity suffices: no HIP call
    const long frees = F.frees[kind];
    CHECK(b.reserve(101) == hipSuccess && b.capacity() == 101);
    CHECK(F.calls == calls + 2 && F.frees[kind] == frees + 1 && liveOf(kind) == 1); // a larger request: free, then allocate
    F.failAt = F.created + 1;
    CHECK(b.reserve(200) != hipSuccess);
    CHECK(!b.get() && b.capacity() == 0 && liveOf(kind) == 0); // a failed allocation leaves no pointer and no size behind
    F.failAt = 0;
    calls = F.calls;
    CHECK(b.reserve(50) == hipSuccess && b.get() && b.capacity() == 50 && F.calls == calls + 1); // ... and the next one starts over
    return 0;
}

// hr_ctx::Group's resources, created in hr_ctx_create's order by a function that returns on the first failure
struct GroupLike {
    Stream stream, streamB;
    Event evFork, evJoin, evUser, tableCopied[4], statusEv[4];
    DeviceBuf<char> dTables;
    PinnedBuf<char> hTables;
    PinnedBuf<uint32_t> hQCount, hCounts;
    PinnedBuf<volatile unsigned long long> hSeq, hProbe;
    char *dTablesHost = nullptr; // aliases: the device's addresses of the mapped blocks
    uint32_t *dCounts = nullptr;
    unsigned long long *dSeq = nullptr, *dProbeHost = nullptr;
};
#define TRY(expr)                          \
    do {                                   \
        if ((expr) != hipSuccess) return false; \
    } while (0)
static bool createGroupLike(GroupLike &G)
{
    const unsigned spun = hipHostMallocCoherent | hipHostMallocMapped;
    TRY(G.stream.createWithPriority(hipStreamNonBlocking, -1));
    TRY(G.streamB.createWithPriority(hipStreamNonBlocking, -1));
    TRY(G.evFork.create(hipEventDisableTiming));
    TRY(G.evJoin.create(hipEventDisableTiming));
    TRY(G.dTables.alloc(4 * 512));
    TRY(G.hTables.alloc(4 * 512));
    TRY(G.hTables.devicePointer(&G.dTablesHost));
    TRY(G.evUser.create(hipEventDisableTiming));
    for (Event &e : G.tableCopied) TRY(e.create(hipEventDisableTiming));
    for (Event &e : G.statusEv) TRY(e.create(hipEventDisableTiming));
    TRY(G.hQCount.alloc(4 * 64));
    TRY(G.hCounts.alloc(4 * 16 + 1, spun));
    TRY(G.hSeq.alloc(4, spun));
    TRY(G.hCounts.devicePointer(&G.dCounts));
    TRY(G.hSeq.devicePointer(&G.dSeq));
    TRY(G.hProbe.alloc(4 * 8, spun));
    TRY(G.hProbe.devicePointer(&G.dProbeHost));
    return true;
}

static int aggregate()
{
    long nCalls = 0;
    {
        const long created = F.created;
        GroupLike G;
        CHECK(createGroupLike(G) && (void *)G.dSeq == (void *)G.hSeq.get());
        nCalls = F.created - created;
        CHECK(nCalls == 19 && liveOf(FakeHip::St) == 2 && liveOf(FakeHip::Ev) == 11 && liveOf(FakeHip::Device) == 1 && liveOf(FakeHip::Host) == 5);
    }
    CHECK(F.liveTotal() == 0);
    for (long k = 1; k <= nCalls; ++k) { // creation call k fails: what was made so far goes with the aggregate
        {
            GroupLike G;
            F.failAt = F.created + k;
            CHECK(!createGroupLike(G));
            F.failAt = 0;
            CHECK(F.liveTotal() == k - 1);
        }
        for (int kind = 0; kind < FakeHip::Kinds; ++kind) CHECK(liveOf((FakeHip::Kind)kind) == 0);
    }
    return 0;
}

// a feature's state: release() is `*this = State()`
struct StateLike {
    DeviceBuf<float> work, out;
    PinnedBuf<float> pinned;
    Event evDone;
    int flag = 0;
};
static int assignedDefault()
{
    StateLike s;
    CHECK(s.work.alloc(8) == hipSuccess && s.out.alloc(8) == hipSuccess && s.pinned.alloc(8) == hipSuccess && s.evDone.create(hipEventDisableTiming) == hipSuccess);
    s.flag = 3;
    const long d = F.frees[FakeHip::Device], h = F.frees[FakeHip::Host], e = F.frees[FakeHip::Ev];
    s = StateLike();
    CHECK(F.frees[FakeHip::Device] == d + 2 && F.frees[FakeHip::Host] == h + 1 && F.frees[FakeHip::Ev] == e + 1); // each member once
    CHECK(F.liveTotal() == 0 && !s.work.get() && !s.pinned.get() && !s.evDone.get() && s.flag == 0 && s.work.capacity() == 0);
    return 0;
}

int main()
{
    if (handles()) return 1;
    CHECK(F.liveTotal() == 0);
    if (reserveOf<DeviceBuf<float>>(FakeHip::Device) || reserveOf<PinnedBuf<float>>(FakeHip::Host)) return 1;
    if (aggregate() || assignedDefault()) return 1;
    CHECK(F.liveTotal() == 0);
    printf("owned cpu: ok\n");
    return 0;
}
