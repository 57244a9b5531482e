/* hip_util.h -- the host side's HIP helpers: the error check and owners of
 * device memory, pinned memory, events and modules, which move (by
 * construction) and do not copy.  Every owner frees in its destructor on the
 * device that is current then; what lives longer than a call is held per
 * device and destroyed through OnDevice. */
#ifndef PT_HIP_UTIL_H
#define PT_HIP_UTIL_H

#include <hip/hip_runtime.h>

#include "internal.h"

namespace pt
{

#define HIPCHECK(x)                                                                     \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess)                                                           \
            throw Error(PT_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* Restores the calling thread's current HIP device on scope exit. */
struct DeviceGuard
{
    int prev = -1;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

/* Deleter of a per-device holder (T::device): the holder and every owner in it
 * are destroyed with that device current, the caller's restored afterwards.
 * If the device cannot be made current the holder is left alone: nothing is
 * freed on another device. */
struct OnDevice
{
    template <class T>
    void operator()(T *p) const
    {
        int prev = 0;
        if (p && hipGetDevice(&prev) == hipSuccess && hipSetDevice(p->device) == hipSuccess) {
            delete p;
            (void)hipSetDevice(prev);
        }
    }
};

/* Grow-only memory of one element type; Mem says where it lives. */
template <class T, class Mem>
struct Buf
{
    T *p = nullptr;
    size_t n = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
    ~Buf() { release(); }
    void ensure(size_t count)
    {
        if (count <= n)
            return;
        release();
        HIPCHECK(Mem::alloc((void **)&p, count * sizeof(T)));
        n = count;
    }
    void release()
    {
        if (p)
            (void)Mem::free(p);
        p = nullptr;
        n = 0;
    }
};
struct DeviceMem
{
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void *p) { return hipFree(p); }
};
/* Page-locked host staging: transfers from and to it are true DMA, with no
 * driver-side staging copy (pt_render's small per-call transfers) */
struct PinnedMem
{
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;

/* device memory of one call */
struct Scratch
{
    std::vector<void *> v;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    void *alloc(size_t bytes)
    {
        void *q = nullptr;
        HIPCHECK(hipMalloc(&q, bytes ? bytes : 4));
        v.push_back(q);
        return q;
    }
    void *upload(const void *host, size_t bytes)
    {
        void *q = alloc(bytes);
        if (host)
            HIPCHECK(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice));
        return q;
    }
    ~Scratch()
    {
        for (void *q : v) (void)hipFree(q);
    }
};

/* HIP events, destroyed with their owner */
struct Events
{
    std::vector<hipEvent_t> e;
    Events() = default;
    Events(Events &&o) noexcept { e.swap(o.e); }
    void create(int n) /* not a constructor: the destructor must run if one creation fails */
    {
        for (int k = 0; k < n; k++) {
            e.push_back(nullptr);
            HIPCHECK(hipEventCreate(&e.back()));
        }
    }
    void record(int k, hipStream_t stream) { HIPCHECK(hipEventRecord(e[(size_t)k], stream)); }
    int add(hipStream_t stream) /* one more event, recorded now; returns its index */
    {
        create(1);
        record((int)e.size() - 1, stream);
        return (int)e.size() - 1;
    }
    float ms(int a, int b) const
    {
        float v = 0.0f;
        HIPCHECK(hipEventElapsedTime(&v, e[(size_t)a], e[(size_t)b]));
        return v;
    }
    ~Events()
    {
        for (hipEvent_t x : e)
            if (x)
                (void)hipEventDestroy(x);
    }
};

/* A loaded code object */
struct Module
{
    hipModule_t m = nullptr;
    Module() = default;
    Module(Module &&o) noexcept : m(o.m) { o.m = nullptr; }
    ~Module() { unload(); }
    explicit operator bool() const { return m != nullptr; }
    void load(const std::vector<char> &code)
    {
        unload();
        HIPCHECK(hipModuleLoadData(&m, code.data()));
    }
    void unload()
    {
        if (m)
            (void)hipModuleUnload(m);
        m = nullptr;
    }
    hipFunction_t fn(const char *name) const
    {
        hipFunction_t f;
        HIPCHECK(hipModuleGetFunction(&f, m, name));
        return f;
    }
};

} // namespace pt

#endif
