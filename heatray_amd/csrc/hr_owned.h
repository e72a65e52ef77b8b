// hr_owned.h — the host side's four owning handles: a device buffer, a pinned host buffer, an event and a stream.  Host-only, like
// hr_tune.h and hr_step_memory.h; included by hr_features.h and hr_ctx.h only.  The four destruction calls of the host side (hipFree,
// hipHostFree, hipEventDestroy, hipStreamDestroy) live here: a resource is freed because its owner went away (a member of a struct that
// is destroyed or assigned a fresh one, a local at the end of its scope), once, and a null handle is never passed to a destruction call.
// The handles move and do not copy; creation returns hipError_t (HIP_TRY at the call site) and an owner that fails is left empty.
// A handle reads as its raw pointer wherever one is expected (a launch argument, a copy, an index); never hand that to a free call.
// tests/host/owned_cpu.cpp compiles this file against a counting fake of the HIP calls below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace hr_owned_detail {
// what the four share: one raw value, emptied by a move, destroyed once by `Free` when it is set
template <class Raw, class Free> class Handle {
  public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = Raw(); }
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o) reset(), h_ = o.h_, o.h_ = Raw();
        return *this;
    }
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ~Handle() { reset(); }
    void reset()
    {
        if (h_) Free()(h_);
        h_ = Raw();
    }
    Raw get() const { return h_; }
    operator Raw() const { return h_; }

  protected:
    Raw h_ = Raw();
};
struct FreeDevice { void operator()(const volatile void *p) const { (void)hipFree(const_cast<void *>(p)); } };
struct FreeHost { void operator()(const volatile void *p) const { (void)hipHostFree(const_cast<void *>(p)); } };
struct FreeEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FreeStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
} // namespace hr_owned_detail

// Device memory: a typed pointer and how many elements it holds (bytes: DeviceBuf<char>).
template <class T> class DeviceBuf : public hr_owned_detail::Handle<T *, hr_owned_detail::FreeDevice> {
    typedef hr_owned_detail::Handle<T *, hr_owned_detail::FreeDevice> Base;

  public:
    hipError_t alloc(size_t n) // frees what it held; n elements, uninitialised
    {
        reset();
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess) this->h_ = (T *)p, cap_ = n;
        return e;
    }
    // Grow-only, contents NOT kept: no HIP call while the capacity suffices; otherwise free, then allocate n + headroom (room for the
    // next few requests).  A failed allocation leaves the handle empty with capacity 0 (no size is left behind: the next call starts over).
    hipError_t reserve(size_t n, size_t headroom = 0) { return (this->h_ && cap_ >= n) ? hipSuccess : alloc(n + headroom); }
    size_t capacity() const { return cap_; }
    void reset() { Base::reset(), cap_ = 0; }
    T *release() // hands the memory on without freeing it: the caller (or whom it gives the pointer to) owns it now
    {
        T *p = this->h_;
        this->h_ = nullptr, cap_ = 0;
        return p;
    }
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf &&o) noexcept : Base(std::move(o)), cap_(o.cap_) { o.cap_ = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept
    {
        if (this != &o) {
            const size_t cap = o.cap_; // (the base's assignment resets this handle first, which zeroes cap_)
            o.cap_ = 0;
            Base::operator=(std::move(o));
            cap_ = cap;
        }
        return *this;
    }

  private:
    size_t cap_ = 0;
};

// Pinned host memory; T may be volatile (words the host polls while a kernel writes them).  It keeps the flags it was allocated with:
// hipHostMallocDefault, or hipHostMallocCoherent | hipHostMallocMapped for memory the host reads while a kernel that writes it runs.
template <class T> class PinnedBuf : public hr_owned_detail::Handle<T *, hr_owned_detail::FreeHost> {
    typedef hr_owned_detail::Handle<T *, hr_owned_detail::FreeHost> Base;

  public:
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault)
    {
        reset();
        void *p = nullptr;
        const hipError_t e = hipHostMalloc(&p, n * sizeof(T), flags);
        if (e == hipSuccess) this->h_ = (T *)p, cap_ = n, flags_ = flags;
        return e;
    }
    hipError_t reserve(size_t n) { return (this->h_ && cap_ >= n) ? hipSuccess : alloc(n, flags_); } // as DeviceBuf::reserve, with its flags
    size_t capacity() const { return cap_; }
    unsigned flags() const { return flags_; }
    // the address the device uses for a mapped block
    template <class U> hipError_t devicePointer(U **out) const { return hipHostGetDevicePointer((void **)out, const_cast<void *>((const volatile void *)this->h_), 0); }
    void reset() { Base::reset(), cap_ = 0; }
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : Base(std::move(o)), cap_(o.cap_), flags_(o.flags_) { o.cap_ = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept
    {
        if (this != &o) {
            const size_t cap = o.cap_;
            o.cap_ = 0;
            Base::operator=(std::move(o));
            cap_ = cap, flags_ = o.flags_;
        }
        return *this;
    }

  private:
    size_t cap_ = 0;
    unsigned flags_ = hipHostMallocDefault;
};

struct Event : hr_owned_detail::Handle<hipEvent_t, hr_owned_detail::FreeEvent> {
    hipError_t create(unsigned flags = hipEventDefault) // destroys what it held
    {
        reset();
        hipEvent_t e = nullptr;
        const hipError_t err = hipEventCreateWithFlags(&e, flags);
        if (err == hipSuccess) h_ = e;
        return err;
    }
};

struct Stream : hr_owned_detail::Handle<hipStream_t, hr_owned_detail::FreeStream> {
    hipError_t create(unsigned flags)
    {
        reset();
        hipStream_t s = nullptr;
        const hipError_t err = hipStreamCreateWithFlags(&s, flags);
        if (err == hipSuccess) h_ = s;
        return err;
    }
    hipError_t createWithPriority(unsigned flags, int priority)
    {
        reset();
        hipStream_t s = nullptr;
        const hipError_t err = hipStreamCreateWithPriority(&s, flags, priority);
        if (err == hipSuccess) h_ = s;
        return err;
    }
};
