// A fake of the HIP calls heatray_amd/csrc/hr_owned.h uses, for tests/host/owned_cpu.cpp (put first on the include path): it counts the
// live objects of each kind, aborts on a double free, an unknown pointer or a null passed to the host-free, event-destroy or
// stream-destroy call, and can be told to fail the k-th creation call.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <set>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct fakeEvent *hipEvent_t;
typedef struct fakeStream *hipStream_t;
enum { hipHostMallocDefault = 0u, hipHostMallocMapped = 2u, hipHostMallocCoherent = 0x40000000u };
enum { hipEventDefault = 0u, hipEventDisableTiming = 2u };
enum { hipStreamDefault = 0u, hipStreamNonBlocking = 1u };

struct FakeHip {
    enum Kind { Device, Host, Ev, St, Kinds };
    std::set<void *> live[Kinds];
    long created = 0;    // creation calls so far (failed ones included)
    long failAt = 0;     // the creation call with this number fails (0: none)
    long calls = 0;      // every call of the fake, creation or destruction
    long frees[Kinds] = {0, 0, 0, 0};
    unsigned lastHostFlags = 0, lastEventFlags = 0, lastStreamFlags = 0;
    int lastPriority = 0;
    long liveTotal() const { return (long)(live[Device].size() + live[Host].size() + live[Ev].size() + live[St].size()); }
    static void die(const char *what)
    {
        fprintf(stderr, "fake hip: %s\n", what);
        abort();
    }
    hipError_t make(Kind k, void **out, size_t bytes = 1)
    {
        ++calls;
        if (++created == failAt) return hipErrorOutOfMemory; // (*out is left as it was, like a failed call may)
        *out = malloc(bytes ? bytes : 1);
        live[k].insert(*out);
        return hipSuccess;
    }
    hipError_t drop(Kind k, void *p, bool nullAllowed)
    {
        ++calls;
        if (!p) {
            if (!nullAllowed) die("null handle passed to a destruction call");
            return hipSuccess;
        }
        if (!live[k].erase(p)) die("double free, or a pointer of another kind");
        ++frees[k];
        free(p);
        return hipSuccess;
    }
};
inline FakeHip &fakeHip()
{
    static FakeHip f;
    return f;
}

inline hipError_t hipMalloc(void **p, size_t bytes) { return fakeHip().make(FakeHip::Device, p, bytes); }
inline hipError_t hipFree(void *p) { return fakeHip().drop(FakeHip::Device, p, true); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags)
{
    fakeHip().lastHostFlags = flags;
    return fakeHip().make(FakeHip::Host, p, bytes);
}
inline hipError_t hipHostFree(void *p) { return fakeHip().drop(FakeHip::Host, p, false); }
inline hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned)
{
    ++fakeHip().calls;
    if (!fakeHip().live[FakeHip::Host].count(host)) FakeHip::die("device address asked of memory that is not pinned");
    *dev = host;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    fakeHip().lastEventFlags = flags;
    return fakeHip().make(FakeHip::Ev, (void **)e);
}
inline hipError_t hipEventDestroy(hipEvent_t e) { return fakeHip().drop(FakeHip::Ev, e, false); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
    fakeHip().lastStreamFlags = flags;
    return fakeHip().make(FakeHip::St, (void **)s);
}
inline hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority)
{
    fakeHip().lastStreamFlags = flags, fakeHip().lastPriority = priority;
    return fakeHip().make(FakeHip::St, (void **)s);
}
inline hipError_t hipStreamDestroy(hipStream_t s) { return fakeHip().drop(FakeHip::St, s, false); }
