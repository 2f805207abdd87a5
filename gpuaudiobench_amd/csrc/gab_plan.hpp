// gab_plan.hpp — what the host halves of the eq, mix and delay plans share: who owns device memory,
// "check, then commit" for a set of parameters, and the table that is ramped from current to target over one buffer.
#pragma once

#include <utility>
#include <vector>

#include "gab_common.hpp"

namespace gab {

// The owner of one hipMalloc allocation.  A plan holds these as members, so deleting the plan (or a create that throws
// half-way, the plan in a unique_ptr) frees every buffer it has.
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
    ~DeviceBuf() { if (p_) (void)hipFree(p_); }
    void alloc(size_t n) {              // once per buffer; the contents are whatever the memory held
        GAB_HIP_CHECK(hipMalloc(&p_, n * sizeof(T)));
        n_ = n;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }  // elements

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// ---- check, then commit: the check ----
// A plan's check kernel lowers *flag (atomicMin) to the index of every value it refuses, so the host can name the FIRST.
// The flag starts as all ones, which therefore no index may be: a set of more than kMaxChecked values is refused unread.
constexpr unsigned kNoneRefused = 0xffffffffu;
constexpr size_t kMaxChecked = 0xfffffff0u;

// An infinity or a NaN, from the value's bits (__float_as_uint): the integer test, whatever the compiler knows of the float.
__device__ __forceinline__ bool not_finite(unsigned float_bits) { return (float_bits & 0x7f800000u) == 0x7f800000u; }

// launch_check() launches the plan's check kernel on s.  *first: the smallest refused index, or kNoneRefused.  The stream
// has been synchronised when this returns GAB_OK; the caller writes its tables only after it has looked at *first.
template <class F>
int first_refused(const DeviceBuf<unsigned>& flag, hipStream_t s, const char* kernel, F&& launch_check, unsigned* first) {
    GAB_HIP_CHECK(hipMemsetAsync(flag.get(), 0xff, sizeof(unsigned), s));
    launch_check();
    if (int rc = launch_status(kernel)) return rc;
    GAB_HIP_CHECK(hipMemcpyAsync(first, flag.get(), sizeof(unsigned), hipMemcpyDeviceToHost, s));
    GAB_HIP_CHECK(hipStreamSynchronize(s));
    return GAB_OK;
}

inline bool track_range_ok(int plan_tracks, int first_track, int n_tracks) {
    return !(first_track < 0 || n_tracks <= 0 || first_track > plan_tracks - n_tracks);
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

}  // namespace gab
