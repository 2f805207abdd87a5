// gab_plan.hpp — what the host halves of the plans share.  Who owns device memory, pinned memory,
// events and streams: every plan.  For the seventeen track plans (eq, mix, delay, meter, resample, dynamics, reverb, gate,
// crossover, limiter, spectrum, resynthesis, denoise, saturator, nlms, fdaf and mconv) also "check, then commit" for a set of parameters (one check
// kernel, a rule per table); the bodies of their
// extern "C" entries (create, process_batch, a ranged set, the exposed table, destroy, and every call that starts with
// a null check); the table that is ramped from current to target over one buffer.
#pragma once

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gab_common.hpp"

namespace gab {

// ---- the owners ----
// Every GPU resource of a plan is a member of one of these four kinds, so deleting the plan (or a create that throws
// half-way, the plan in a unique_ptr) gives back all of it and no destroy lists what to free.  Move-only; get() is the
// raw handle for kernels and the runtime; made once, or again behind a release().
inline void refuse_live(const void* live, const char* who) {
    if (live) throw std::logic_error(std::string(who) + ": made again without a release() between");
}

// One device allocation (hipFree).  The contents are whatever the memory held.
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept { swap(o); }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept { swap(o); return *this; }     // (what this held goes with o)
    ~DeviceBuf() { release(); }
    void alloc(size_t n) { refuse_live(p_, "DeviceBuf"); GAB_HIP_CHECK(hipMalloc(&p_, n * sizeof(T))); n_ = n; }
    // flags: hipDeviceMallocFinegrained (a copy engine fills it while a kernel reads it) or hipDeviceMallocDefault
    void alloc_with_flags(size_t n, unsigned flags) {
        refuse_live(p_, "DeviceBuf");
        GAB_HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&p_), n * sizeof(T), flags));
        n_ = n;
    }
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }         // (for another size: release, then alloc)
    void fill(const T& v) {                                                     // v in every element, from the host
        const std::vector<T> h(n_, v);
        GAB_HIP_CHECK(hipMemcpy(p_, h.data(), n_ * sizeof(T), hipMemcpyHostToDevice));
    }
    void swap(DeviceBuf& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }
    T* get() const { return p_; }
    size_t size() const { return n_; }  // elements
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Pinned host memory (hipHostMalloc, hipHostFree), zeroed; the host reads and writes it in place.
template <class T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { swap(o); return *this; }
    ~PinnedBuf() { release(); }
    void alloc(size_t n) {
        refuse_live(p_, "PinnedBuf");
        GAB_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), hipHostMallocDefault));
        for (n_ = 0; n_ < n; ++n_) p_[n_] = T();
    }
    void release() { if (p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
    void swap(PinnedBuf& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }
    T* get() const { return p_; }
    T& operator[](size_t i) const { return p_[i]; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// An event without timing.
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept { swap(o); }
    Event& operator=(Event&& o) noexcept { swap(o); return *this; }
    ~Event() { release(); }
    void create() { refuse_live(e_, "Event"); GAB_HIP_CHECK(hipEventCreateWithFlags(&e_, hipEventDisableTiming)); }
    void release() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    void swap(Event& o) noexcept { std::swap(e_, o.e_); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }

private:
    hipEvent_t e_ = nullptr;
};

// A stream of the plan's own.
class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept { swap(o); }
    Stream& operator=(Stream&& o) noexcept { swap(o); return *this; }
    ~Stream() { release(); }
    void create(unsigned flags) { refuse_live(s_, "Stream"); GAB_HIP_CHECK(hipStreamCreateWithFlags(&s_, flags)); }
    // Non-blocking, at the HIGHEST priority: the runtime maps streams onto a few hardware queues per priority, and streams
    // of the default priority never share a queue with this one (an upload beside the caller's launch; a resident launch)
    static Stream highest_priority() {
        Stream s;
        int lo = 0, hi = 0;             // (numerically lower = higher priority)
        GAB_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        GAB_HIP_CHECK(hipStreamCreateWithPriority(&s.s_, hipStreamNonBlocking, hi));
        return s;
    }
    void release() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    void swap(Stream& o) noexcept { std::swap(s_, o.s_); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }

private:
    hipStream_t s_ = nullptr;
};

// ---- check, then commit: the check ----
// The check kernel lowers *flag (atomicMin) to the index of every value the plan's rule refuses, so the host can name
// the FIRST.  The flag starts as all ones, which therefore no index may be: a set of more than kMaxChecked values is
// refused unread.
constexpr unsigned kNoneRefused = 0xffffffffu;
constexpr size_t kMaxChecked = 0xfffffff0u;

// An infinity or a NaN, from the value's bits (__float_as_uint): the integer test, whatever the compiler knows of the float.
__device__ __forceinline__ bool not_finite(unsigned float_bits) { return (float_bits & 0x7f800000u) == 0x7f800000u; }

// A Rule is a small trivially copyable struct, passed by value, that holds the plan's few numbers and has
//   __device__ bool refuses(const T* src, size_t i) const    is src[i] outside the contract?  (src, not the value: a rule
//                                                            may read a neighbour of the value it judges)
//   std::string refusal(unsigned i, int first_track) const   the text behind "<who>: " for a refused index i (host)
template <class T, class Rule>
__global__ __launch_bounds__(256) void check_kernel(const T* __restrict__ src, unsigned* __restrict__ flag, size_t n,
                                                   Rule rule) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && rule.refuses(src, i)) atomicMin(flag, (unsigned)i);
}

// launch_check() launches a check kernel on s.  *first: the smallest refused index, or kNoneRefused.  The stream has been
// synchronised when this returns GAB_OK; the caller writes its tables only after it has looked at *first.
template <class F>
int first_refused(const DeviceBuf<unsigned>& flag, hipStream_t s, const char* kernel, F&& launch_check, unsigned* first) {
    GAB_HIP_CHECK(hipMemsetAsync(flag.get(), 0xff, sizeof(unsigned), s));
    launch_check();
    if (int rc = launch_status(kernel)) return rc;
    GAB_HIP_CHECK(hipMemcpyAsync(first, flag.get(), sizeof(unsigned), hipMemcpyDeviceToHost, s));
    GAB_HIP_CHECK(hipStreamSynchronize(s));
    return GAB_OK;
}

// check, then commit: n values at d_src against the rule on s; commit() only if none is refused.  A refused set has
// touched nothing but the flag, and the stream is synchronised.  commit() synchronises too: d_src is the caller's again.
template <class T, class Rule, class Commit>
int check_then(const DeviceBuf<unsigned>& flag, hipStream_t s, const char* who, const T* d_src, size_t n,
               const Rule& rule, int first_track, Commit&& commit) {
    if (n > kMaxChecked) return bad_arg((std::string(who) + ": the range is too large for one call").c_str());
    unsigned first_bad = kNoneRefused;
    if (int rc = first_refused(flag, s, "check_kernel", [&] {
            hipLaunchKernelGGL((check_kernel<T, Rule>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_src, flag.get(), n, rule);
        }, &first_bad))
        return rc;
    if (first_bad != kNoneRefused) {
        set_last_error(std::string(who) + ": " + rule.refusal(first_bad, first_track));
        return GAB_ERR_INVALID_ARG;
    }
    commit();
    return GAB_OK;
}

// The text of a row rule: value i of rows `row` wide, the first of them track first_track's.
inline std::string row_refusal(unsigned i, unsigned row, int first_track, const char* name, const char* rule) {
    return "track " + std::to_string(first_track + (int)(i / row)) + " field " + std::to_string((int)(i % row)) + " (" +
           name + ") " + rule + "; the plan keeps its parameters";
}

// ---- what a launch function asks of its pointers ----
// Do a[0, n_floats) and b[0, n_floats) share a byte?
inline bool overlaps(const float* a, const float* b, size_t n_floats) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = (uintptr_t)n_floats * sizeof(float);
    return pa < pb + bytes && pb < pa + bytes;
}

// Is every one of them on a 16-byte boundary (a null pointer is)?
inline bool all_aligned16(std::initializer_list<const void*> ps) {
    uintptr_t bits = 0;
    for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15u) == 0;
}

// The floats of a ring: the smallest power of two that is at least `need`.
inline size_t ring_capacity(size_t need) {
    size_t cap = 1;
    while (cap < need) cap *= 2;
    return cap;
}

// ---- the entries ----
// Every refusal of an argument: "<who>: <what>" and GAB_ERR_INVALID_ARG.
inline int refuse(const char* who, const char* what) { return bad_arg((std::string(who) + ": " + what).c_str()); }

// The body of an extern "C" function that starts with a null check: `needed` (the plan first), then body().
template <class Body>
int entry(const char* who, std::initializer_list<const void*> needed, Body&& body, const char* what = "null pointer") {
    return guarded([&]() -> int {
        for (const void* p : needed)
            if (!p) return refuse(who, what);
        return body();
    });
}

// The body of gab_X_process_batch: null pointers, then n_buffers, then body() (the plan's own checks and its launch).
// gab_X_process is entry() with a body that launches one buffer.
template <class Body>
int batch_entry(const char* who, std::initializer_list<const void*> needed, int n_buffers, Body&& body) {
    return entry(who, needed, [&]() -> int {
        if (n_buffers <= 0) return refuse(who, "n_buffers must be > 0");
        return body();
    });
}

// The body of gab_X_create.  check() is the plan's own verdict on its arguments (GAB_OK, or a refusal with its text
// set) and works out what build needs of them; build(P&) allocates and fills the plan, whose tracks and bufsize are
// set, and returns GAB_OK or a launch's status.  The plan sits in a unique_ptr until it is published, last: *out is null
// after every refusal and after a build that throws, and nothing of a half-built plan stays behind.
template <class P, class Check, class Build>
int create_entry(const char* who, P** out, int tracks, int bufsize, Check&& check, Build&& build) {
    return guarded([&]() -> int {
        if (!out) return refuse(who, "null plan pointer");
        *out = nullptr;
        if (tracks <= 0 || bufsize <= 0) return refuse(who, "tracks and bufsize must be > 0");
        if (int rc = check()) return rc;
        if (int rc = refuse_unsupported_runtime_mode(who)) return rc;
        auto p = std::make_unique<P>();
        p->tracks = tracks;
        p->bufsize = bufsize;
        if (int rc = build(*p)) return rc;
        *out = p.release();
        return GAB_OK;
    });
}

inline bool track_range_ok(int plan_tracks, int first_track, int n_tracks) {
    return !(first_track < 0 || n_tracks <= 0 || first_track > plan_tracks - n_tracks);
}

// The body of gab_X_set_* (whole: every track of the plan) and of gab_X_set_*_tracks (tracks [first_track, first_track +
// n_tracks)): null pointers, then the range, then the plan's set(plan, d_src, first_track, n_tracks, who, rest...).
template <class F, class P, class S, class... A>
int set_entry(const char* who, F set, P* plan, const S* d_src, bool whole, int first_track, int n_tracks, A... rest) {
    return entry(who, {plan, d_src}, [&]() -> int {
        if (whole) return set(plan, d_src, 0, plan->tracks, who, rest...);
        if (!track_range_ok(plan->tracks, first_track, n_tracks))
            return refuse(who, "the track range is outside the plan");
        return set(plan, d_src, first_track, n_tracks, who, rest...);
    });
}

// The body of gab_X_destroy; text: what a null plan is answered with.
template <class P>
int destroy_plan(P* plan, const char* text) {
    return guarded([&]() -> int {
        if (!plan) return bad_arg(text);
        delete plan;
        return GAB_OK;
    });
}

// ---- the ramped table ----
// Two copies of a plan's parameters and the ramp between them: a kernel takes `target`, except on the one buffer behind
// a ramped set, where sample s takes fmaf(target - current, r[s], current).  `pending` says that buffer is still to come.
struct RampedTable {
    DeviceBuf<float> current, target;   // [floats] each; the plan fills both when it is created
    DeviceBuf<float> ramp;              // [bufsize]: r[s] = (s + 1) / bufsize
    bool pending = false;

    void create(size_t floats, int bufsize) {
        current.alloc(floats);
        target.alloc(floats);
        ramp.alloc((size_t)bufsize);
        // r[s] = (s + 1) / B in float64, rounded once: no device division enters the bits
        std::vector<float> r((size_t)bufsize);
        for (int s = 0; s < bufsize; ++s) r[(size_t)s] = (float)(((double)s + 1.0) / (double)bufsize);
        GAB_HIP_CHECK(hipMemcpy(ramp.get(), r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice));
    }

    // `row` on every one of `tracks` tracks, in current and in target: what a new plan holds.
    void fill(const std::vector<float>& row, int tracks) {
        std::vector<float> init;
        init.reserve(row.size() * (size_t)tracks);
        for (int t = 0; t < tracks; ++t) init.insert(init.end(), row.begin(), row.end());
        GAB_HIP_CHECK(hipMemcpy(current.get(), init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemcpy(target.get(), init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
    }

    // The commit, for values that passed the check: n floats at `offset` of target; of current too unless they are
    // ramped in.  Synchronises: d_src is the caller's again when this returns.
    void commit(const float* d_src, size_t offset, size_t n, bool ramped, hipStream_t s) {
        GAB_HIP_CHECK(hipMemcpyAsync(target.get() + offset, d_src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (ramped) {
            pending = true;
        } else {
            GAB_HIP_CHECK(hipMemcpyAsync(current.get() + offset, d_src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    }

    // current := target by a copy on s, and no ramp is pending: behind the launch that ran the ramp (exactly once, on
    // that launch's stream), and at a reset.  Nothing waits here.
    void snap(hipStream_t s) {
        GAB_HIP_CHECK(hipMemcpyAsync(current.get(), target.get(), target.size() * sizeof(float), hipMemcpyDeviceToDevice, s));
        pending = false;
    }
};

// The body of gab_X_params / gab_mix_gains: the plan's tables themselves, not copies.
template <class P>
int expose_entry(const char* who, P* plan, RampedTable P::*table, float** d_current, float** d_target,
                 size_t* n_floats) {
    return entry(who, {plan, d_current, d_target, n_floats}, [&] {
        *d_current = (plan->*table).current.get();
        *d_target = (plan->*table).target.get();
        *n_floats = (plan->*table).current.size();
        return GAB_OK;
    });
}

}  // namespace gab
