// A stand-in for <hip/hip_runtime.h>, for the programs of tests/plan_owners alone: the few entry points gab_plan.hpp
// uses, as counting stubs, so that the owners and the entries can be exercised by a host compiler under a sanitizer
// without a GPU.  Every create hands out a fresh heap block as its handle and records it; every destroy must name a
// live handle of its own kind; a blocking copy copies (device memory is the heap here).  stub::fail_after(n) makes the
// n-th create from now fail.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <set>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define hipLaunchKernelGGL(...) ((void)0)

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
struct StubStream;
struct StubEvent;
typedef StubStream* hipStream_t;
typedef StubEvent* hipEvent_t;
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static const dim3 blockIdx, threadIdx;
inline unsigned atomicMin(unsigned* p, unsigned v) { const unsigned o = *p; if (v < o) *p = v; return o; }

constexpr unsigned hipDeviceMallocDefault = 0, hipDeviceMallocFinegrained = 1;
constexpr unsigned hipHostMallocDefault = 0;
constexpr unsigned hipEventDisableTiming = 2;
constexpr unsigned hipStreamNonBlocking = 1;

namespace stub {
enum Kind { kDevice, kPinned, kEvent, kStream, kKinds };
struct State {
    std::set<void*> live[kKinds];
    long creates[kKinds] = {}, destroys[kKinds] = {};
    long bad_destroys = 0;          // a handle that is not live, or not of this kind: a double destroy
    long countdown = -1;            // creates until one fails (-1: none)
};
inline State& state() { static State s; return s; }
inline void fail_after(long n) { state().countdown = n; }
inline hipError_t create(Kind k, void** out, size_t bytes) {
    State& s = state();
    if (s.countdown == 0) { s.countdown = -1; return hipErrorOutOfMemory; }
    if (s.countdown > 0) --s.countdown;
    void* p = std::calloc(bytes ? bytes : 1, 1);
    s.live[k].insert(p);
    ++s.creates[k];
    *out = p;
    return hipSuccess;
}
inline hipError_t destroy(Kind k, void* p) {
    State& s = state();
    if (!s.live[k].erase(p)) { ++s.bad_destroys; return hipErrorInvalidValue; }
    ++s.destroys[k];
    std::free(p);
    return hipSuccess;
}
}  // namespace stub

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
template <class T>
inline hipError_t hipMalloc(T** p, size_t bytes) { return stub::create(stub::kDevice, reinterpret_cast<void**>(p), bytes); }
inline hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned) { return stub::create(stub::kDevice, p, bytes); }
inline hipError_t hipFree(void* p) { return stub::destroy(stub::kDevice, p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub::create(stub::kPinned, p, bytes); }
inline hipError_t hipHostFree(void* p) { return stub::destroy(stub::kPinned, p); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return stub::create(stub::kEvent, reinterpret_cast<void**>(e), 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return stub::destroy(stub::kEvent, e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return stub::create(stub::kStream, reinterpret_cast<void**>(s), 1); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return stub::create(stub::kStream, reinterpret_cast<void**>(s), 1); }
inline hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { return stub::destroy(stub::kStream, s); }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
