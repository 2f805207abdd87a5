// k_resynthesis.hip — the resynthesis plan: the overlap-add inverse of the spectrum plan (include/gab_c_api.h,
// gab_resyn_*).  Rows of 513 complex bins per track and frame, as GAB_SPEC_COMPLEX writes them, become the track's
// stream again: every frame is inverse-transformed, scaled by 2^-10, multiplied by a synthesis window and added at its
// place on the hop grid; the 1024 samples that later frames still add to are carried on the device.  The rows are read
// and never written.  No counterpart in the reference.
//
//   resynthesis_kernel   one launch a call: one wave per pair of tracks, four waves a workgroup, no workgroup barrier.
//                        The wave holds its pair's accumulator in a wave-private LDS ring (2 x 1024 floats, indexed from
//                        a moving base) and walks the call's frames in ascending j — that walk is the order of the sum.
//                        Per frame: the finished samples in front of the frame's start go to d_out and their ring slots
//                        are stored as zero; the pair's two rows, read straight into the transform's entry layout
//                        a frame ahead (lane l, register r holds bin k = l + 64 r; k > 512 reads bin N - k), are packed as
//                        Z = Xa + i Xb; gab_fft.hpp's wave-held inverse runs through the wave's image; real and
//                        imaginary part are scaled, windowed and added into the ring, one __fadd_rn per slot.  Behind
//                        the last frame the rest of the call's samples go out and the ring is written back from its base.
//   ResynRule            refuses a window value that is not finite (gab_plan.hpp's check kernel).
//
// A slot's bits are the ordered float32 sum of the header: they depend on the frames' u, on g and on that order, not on
// bufsize, on the cut into calls or batches, on the alignment of d_out or on which frames share a launch.  No atomics, no
// scratch, no second launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_fft.hpp"
#include "gab_plan.hpp"
#include "gab_stft.hpp"

namespace gab {
namespace {

using fft::cf;

constexpr int kResynN = 1024;                             // the transform, and the floats of a track's accumulator
constexpr int kResynBins = kResynN / 2 + 1;               // 513
constexpr int kResynMinHop = 32;
constexpr int kResynImg = fft::Pad<16>::size(kResynN);    // cf entries of a wave's LDS image
constexpr int kResynMaxTracks = 1 << 26;                  // 2^23 workgroups of eight tracks: 2^31 threads

// The lanes of a wave hand ring slots to one another (a slot's lane moves with the base): LDS instructions of a wave
// execute in order, and this keeps the compiler from moving them across the hand-over.
__device__ __forceinline__ void resyn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Grid: x = group of four pairs.  rows: [frames][T][513] complex, only read.  acc: [T][1024]: acc[i] is the partial
// sum of the output sample i places behind the plan's position: on entry the call's first sample, on return the one
// behind its last.  window: [1024].  out: [n][T][B].  Frame f's first sample is output sample `first_end + f H` of the
// call (1 <= first_end <= H; the last such start <= n B).
__global__ __launch_bounds__(256) void resynthesis_kernel(const float2* __restrict__ rows, float* __restrict__ acc,
                                                         const float* __restrict__ window, float* __restrict__ out,
                                                         const cf* __restrict__ tw, int T, int B, int n_buffers, int H,
                                                         int first_end, int frames) {
    __shared__ cf lds[4 * kResynImg];
    __shared__ float rings[4 * 2 * kResynN];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * kResynImg;
    float* const ra = rings + w * 2 * kResynN;
    float* const rb = ra + kResynN;
    const int q = (int)blockIdx.x * 4 + w;
    const int ta = 2 * q;
    if (ta >= T) return;                                   // whole wave; no barriers below
    const bool hasb = ta + 1 < T;
    const bool one_buffer = n_buffers == 1;
    const int L = n_buffers * B;                           // (the host holds it below 2^31 - 1024)

    using WF = fft::WaveFFT1024<true>;
    WF::Twiddles t;
    WF::load_twiddles(t, tw, lane);
    int base = 0;                                          // the ring slot of the oldest sample that is not out yet
    int c = 0;                                             // samples of the call that are out

    // Samples [c, e) of the call (e - c <= 1024, wave-uniform) from the ring's front to d_out; their slots become zero
    // by a store, so whatever they held (a NaN too) is gone.
    auto emit = [&](int e) {
        const int m = e - c;
        for (int idx = lane; idx < m; idx += 64) {
            const int s = (base + idx) & (kResynN - 1);
            const int i = c + idx;
            size_t o;
            if (one_buffer) {
                o = (size_t)ta * B + i;
            } else {
                const unsigned nb = (unsigned)i / (unsigned)B, sb = (unsigned)i - nb * (unsigned)B;
                o = ((size_t)nb * T + ta) * B + sb;
            }
            out[o] = ra[s];
            ra[s] = 0.0f;
            if (hasb) out[o + B] = rb[s];
            rb[s] = 0.0f;
        }
        base = (base + m) & (kResynN - 1);
        c = e;
        resyn_wave_sync();
    };

    // The pair's two rows of a frame are requested a frame ahead (frame 0's here, in front of the ring's fill) and wanted
    // last: the loads fly while the transform before them runs and the finished samples go out.  Lane l, register r: bin
    // k = l + 64 r, for k > 512 bin N - k (conjugated below).
    float2 xa[16], xb[16];
    auto request = [&](int f) {
        const float2* const rowa = rows + ((size_t)f * T + ta) * kResynBins;
        const float2* const rowb = rowa + kResynBins;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = lane + 64 * r;
            const int kk = k > kResynN / 2 ? kResynN - k : k;
            xa[r] = rowa[kk];
            xb[r] = hasb ? rowb[kk] : make_float2(0.0f, 0.0f);
        }
    };
    if (frames > 0) request(0);
    float g[16];
    float* const acca = acc + (size_t)ta * kResynN;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = lane + 64 * r;
        g[r] = window[n];
        ra[n] = acca[n];
        rb[n] = hasb ? acca[kResynN + n] : 0.0f;
    }
    resyn_wave_sync();
    for (int f = 0; f < frames; ++f) {
        emit(first_end + f * H);                           // the ring's front is now the frame's first sample
        // Z[k] = Xa[k] + i Xb[k] (k <= 512), conj(Xa[N - k]) + i conj(Xb[N - k]) (k > 512); the imaginary parts of bins
        // 0 and 512 are read as zero
        cf z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = lane + 64 * r;
            const bool mirror = k > kResynN / 2;
            if (k == 0 || k == kResynN / 2) {
                xa[r].y = 0.0f;
                xb[r].y = 0.0f;
            }
            z[r] = mirror ? fft::mk(__fadd_rn(xa[r].x, xb[r].y), __fsub_rn(xb[r].x, xa[r].y))
                          : fft::mk(__fsub_rn(xa[r].x, xb[r].y), __fadd_rn(xa[r].y, xb[r].x));
        }
        if (f + 1 < frames) request(f + 1);
        WF::run(z, img, t, lane);                          // EXEC is all ones here: every loop above has reconverged
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int s = (base + lane + 64 * r) & (kResynN - 1);
            ra[s] = __fadd_rn(ra[s], __fmul_rn(g[r], __fmul_rn(z[r].x, 0x1p-10f)));
            rb[s] = __fadd_rn(rb[s], __fmul_rn(g[r], __fmul_rn(z[r].y, 0x1p-10f)));
        }
        resyn_wave_sync();
    }
    emit(L);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = lane + 64 * r;
        const int s = (base + n) & (kResynN - 1);
        acca[n] = ra[s];
        if (hasb) acca[kResynN + n] = rb[s];
    }
}

// src: [1024]
struct ResynRule {
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int) const {
        return "window value " + std::to_string(i) + " is not finite; the plan keeps its window";
    }
};

}  // namespace
}  // namespace gab

struct gab_resyn_plan {
    int tracks = 0, bufsize = 0, hop = 0;
    int phase = 0;                     // samples since the reset, mod hop
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::DeviceBuf<float> window;      // [1024]
    gab::DeviceBuf<float> acc;         // [T][1024]
    gab::DeviceBuf<unsigned> flag;

    // frames of a call of n buffers from the plan's position
    long long count(int n_buffers) const { return ((long long)phase + (long long)n_buffers * bufsize) / hop; }
};

namespace gab {
namespace {

// n buffers in one launch on s, from the plan's position; nothing is allocated, nothing waits.  *n_frames: host.
int resyn_launch(gab_resyn_plan* p, const float* d_rows, float* d_out, int n_buffers, int* n_frames, hipStream_t s,
                 const char* who) {
    const long long L = (long long)n_buffers * p->bufsize;
    if (L > 0x7fffffffLL - kResynN) return refuse(who, "n_buffers * bufsize must be below 2^31 - 1024");
    if (reinterpret_cast<uintptr_t>(d_rows) & 7u) return refuse(who, "d_rows must lie on an 8-byte boundary");
    const long long frames = p->count(n_buffers);
    if (frames > 0) {
        const uintptr_t r0 = reinterpret_cast<uintptr_t>(d_rows), o0 = reinterpret_cast<uintptr_t>(d_out);
        const uintptr_t rbytes = (uintptr_t)frames * (uintptr_t)p->tracks * kResynBins * 2 * sizeof(float);
        const uintptr_t obytes = (uintptr_t)L * (uintptr_t)p->tracks * sizeof(float);
        if (r0 < o0 + obytes && o0 < r0 + rbytes) return refuse(who, "d_rows and d_out overlap");
    }
    const unsigned groups = (unsigned)(((p->tracks + 1) / 2 + 3) / 4);
    resynthesis_kernel<<<dim3(groups), 256, 0, s>>>(reinterpret_cast<const float2*>(d_rows), p->acc.get(),
                                                    p->window.get(), d_out, p->tw, p->tracks, p->bufsize, n_buffers,
                                                    p->hop, p->hop - p->phase, (int)frames);
    if (int rc = launch_status("resynthesis_kernel")) return rc;
    p->phase = (int)(((long long)p->phase + L) % p->hop);
    *n_frames = (int)frames;
    return GAB_OK;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_resyn_create(gab_resyn_plan** out, int tracks, int bufsize, int hop) {
    return gab::create_entry("gab_resyn_create", out, tracks, bufsize, [&] {
        if (hop < gab::kResynMinHop || hop > gab::kResynN) return gab::bad_arg("gab_resyn_create: hop must be 32..1024");
        if (tracks > gab::kResynMaxTracks)
            return gab::bad_arg("gab_resyn_create: more than 2^23 workgroups (tracks / 8) in one launch");
        return GAB_OK;
    }, [&](gab_resyn_plan& p) {
        p.hop = hop;
        p.tw = gab::fft::device_twiddles();
        p.window.alloc(gab::kResynN);
        p.acc.alloc((size_t)tracks * gab::kResynN);
        p.flag.alloc(1);
        const std::vector<float> g = gab::stft_hann_dual(hop);  // of the spectrum plan's periodic Hann window
        GAB_HIP_CHECK(hipMemcpy(p.window.get(), g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.acc.get(), 0, p.acc.size() * sizeof(float)));
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_resyn_destroy(gab_resyn_plan* plan) { return gab::destroy_plan(plan, "gab_resyn_destroy: null pointer"); }

// check, then commit (gab_plan.hpp): a refused window leaves the plan's as it was
int gab_resyn_set_window(gab_resyn_plan* plan, const float* d_window, gab_stream_t stream) {
    return gab::set_entry("gab_resyn_set_window",
                          [&](gab_resyn_plan* p, const float* d_src, int, int, const char* who) -> int {
        hipStream_t s = gab::as_stream(stream);
        return gab::check_then(p->flag, s, who, d_src, (size_t)gab::kResynN, gab::ResynRule{}, 0, [&] {
            GAB_HIP_CHECK(hipMemcpyAsync(p->window.get(), d_src, gab::kResynN * sizeof(float), hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
        });
    }, plan, d_window, true, 0, 0);
}

int gab_resyn_reset(gab_resyn_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_resyn_reset", {plan}, [&] {
        GAB_HIP_CHECK(hipMemsetAsync(plan->acc.get(), 0, plan->acc.size() * sizeof(float), gab::as_stream(stream)));
        plan->phase = 0;
        return GAB_OK;
    });
}

int gab_resyn_process(gab_resyn_plan* plan, const float* d_rows, float* d_out, int* n_frames, gab_stream_t stream) {
    return gab::entry("gab_resyn_process", {plan, d_rows, d_out, n_frames}, [&] {
        return gab::resyn_launch(plan, d_rows, d_out, 1, n_frames, gab::as_stream(stream), "gab_resyn_process");
    });
}

int gab_resyn_process_batch(gab_resyn_plan* plan, const float* d_rows, float* d_out, int n_buffers, int* n_frames,
                            gab_stream_t stream) {
    return gab::batch_entry("gab_resyn_process_batch", {plan, d_rows, d_out, n_frames}, n_buffers, [&] {
        return gab::resyn_launch(plan, d_rows, d_out, n_buffers, n_frames, gab::as_stream(stream),
                                 "gab_resyn_process_batch");
    });
}

int gab_resyn_frames(gab_resyn_plan* plan, int n_buffers, int* capacity) {
    return gab::batch_entry("gab_resyn_frames", {plan, capacity}, n_buffers, [&]() -> int {
        const long long L = (long long)n_buffers * plan->bufsize;
        const long long cap = (L + plan->hop - 1) / plan->hop;
        if (cap > 0x7fffffffLL) return gab::refuse("gab_resyn_frames", "n_buffers * bufsize is too large");
        *capacity = (int)cap;
        return GAB_OK;
    });
}

int gab_resyn_count(gab_resyn_plan* plan, int n_buffers, int* frames) {
    return gab::batch_entry("gab_resyn_count", {plan, frames}, n_buffers, [&]() -> int {
        const long long n = plan->count(n_buffers);
        if (n > 0x7fffffffLL) return gab::refuse("gab_resyn_count", "n_buffers * bufsize is too large");
        *frames = (int)n;
        return GAB_OK;
    });
}

int gab_resyn_state(gab_resyn_plan* plan, float** d_acc, float** d_window, int* position_mod_hop) {
    return gab::entry("gab_resyn_state", {plan, d_acc, d_window, position_mod_hop}, [&] {
        *d_acc = plan->acc.get();
        *d_window = plan->window.get();
        *position_mod_hop = plan->phase;
        return GAB_OK;
    });
}

int gab_resyn_latency(gab_resyn_plan* plan, int* samples) {
    return gab::entry("gab_resyn_latency", {plan, samples}, [&] {
        *samples = gab::kResynN;
        return GAB_OK;
    });
}

}  // extern "C"
