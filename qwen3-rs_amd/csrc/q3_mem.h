// q3_mem.h -- owned device and pinned host memory: the only place of the library that allocates or frees either (no kernels here).
//
// DevMem<T> owns one device allocation of n elements, PinMem<T> one pinned host allocation: move-only values like Graph
// (q3_engine.hip).  A member of q3_engine / BatchCtx / BlockScratch goes with its owner, a local on every return path; no list
// of pointers is kept anywhere.  Both convert to T*, so kernel-argument structs, make_launch, hipMemcpyAsync, pointer arithmetic
// and `if (!buf)` take them as they took the raw pointer.
// An allocation group -- buffers of which a later call takes all for granted once it sees the first -- is allocated into locals
// and moved into its owner together (DrawSite::alloc, q3_draw_host.inc): after a failure the owner holds none of it and the next call starts over.
// The allocator is a compile-time policy {allocate, release; for DevMem::grow also Stream, wait}, each returning 0 or a Q3 status.
// The library names the HIP defaults only; tests/mem_host.cpp defines Q3_MEM_NO_HIP and exercises the types over a counting one.
#pragma once
#include <stddef.h>
#include <utility>

struct HipDeviceAlloc;
struct HipPinnedAlloc;

template <class T, class A>
struct OwnedMem {
    T* p = nullptr;
    size_t n = 0;                // capacity in elements
    OwnedMem() = default;
    OwnedMem(const OwnedMem&) = delete;
    OwnedMem& operator=(const OwnedMem&) = delete;
    ~OwnedMem() { reset(); }
    OwnedMem(OwnedMem&& o) noexcept { swap(o); }
    OwnedMem& operator=(OwnedMem&& o) noexcept { OwnedMem t(std::move(o)); swap(t); return *this; }   // what this held goes with t
    operator T*() const { return p; }
    T* operator->() const { return p; }
    void swap(OwnedMem& o) { std::swap(p, o.p); std::swap(n, o.n); }
    void reset() {
        if (p) A::release(p);
        p = nullptr;
        n = 0;
    }
    // a fresh allocation of `count` elements, contents undefined; on failure the object is empty
    int alloc(size_t count) {
        reset();
        void* q = nullptr;
        if (int rc = A::allocate(&q, sizeof(T) * count)) return rc;
        p = (T*)q;
        n = count;
        return 0;
    }
};

template <class T, class A = HipDeviceAlloc>
struct DevMem : OwnedMem<T, A> {
    // Grow-only: room for `need` elements, contents not kept.  A re-allocation first waits for `st` -- launches in flight may still
    // read the buffer that goes -- so the wait happens exactly when a buffer is replaced, and no caller restates that condition.
    // On a failed allocation the object is empty (n == 0) and a later grow starts over.
    int grow(size_t need, typename A::Stream st) {
        if (need <= this->n) return 0;
        if (int rc = A::wait(st)) return rc;
        return this->alloc(need);
    }
};

template <class T, class A = HipPinnedAlloc>
using PinMem = OwnedMem<T, A>;

#ifndef Q3_MEM_NO_HIP
// (fail / HIP_TRY / Q3_OK: q3_engine.hip, in front of this header)  A failed allocation says how many bytes did not fit.
static int q3_mem_status(hipError_t e, const char* what, size_t bytes) {
    return e == hipSuccess ? Q3_OK : fail(Q3_ERR_HIP, "%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
}
struct HipDeviceAlloc {
    typedef hipStream_t Stream;
    static int allocate(void** p, size_t bytes) { return q3_mem_status(hipMalloc(p, bytes), "hipMalloc", bytes); }
    static void release(void* p) { (void)hipFree(p); }
    static int wait(hipStream_t st) { HIP_TRY(hipStreamSynchronize(st)); return Q3_OK; }
};
struct HipPinnedAlloc {
    static int allocate(void** p, size_t bytes) { return q3_mem_status(hipHostMalloc(p, bytes, hipHostMallocDefault), "hipHostMalloc", bytes); }
    static void release(void* p) { (void)hipHostFree(p); }
};
#endif
