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
// The packing, the ring and the window rule are gab_stft.hpp's, which the denoise plan shares.
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

constexpr int kResynMaxTracks = 1 << 26;                  // 2^23 workgroups of eight tracks: 2^31 threads

// Grid: x = group of four pairs.  rows: [frames][T][513] complex, only read.  acc: [T][1024]: acc[i] is the partial
// sum of the output sample i places behind the plan's position: on entry the call's first sample, on return the one
// behind its last.  window: [1024].  out: [n][T][B].  Frame f's first sample is output sample `first_end + f H` of the
// call (1 <= first_end <= H; the last such start <= n B).
__global__ __launch_bounds__(256) void resynthesis_kernel(const float2* __restrict__ rows, float* __restrict__ acc,
                                                         const float* __restrict__ window, float* __restrict__ out,
                                                         const cf* __restrict__ tw, int T, int B, int n_buffers, int H,
                                                         int first_end, int frames) {
    __shared__ cf lds[4 * stft::kImg];
    __shared__ float rings[4 * 2 * stft::kN];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    float* const ra = rings + w * 2 * stft::kN;
    const int q = (int)blockIdx.x * 4 + w;
    const int ta = 2 * q;
    if (ta >= T) return;                                   // whole wave; no barriers below
    const bool hasb = ta + 1 < T;

    using WF = fft::WaveFFT1024<true>;
    WF::Twiddles t;
    WF::load_twiddles(t, tw, lane);
    stft::Ring ring{ra, ra + stft::kN, out, T, B, ta, lane, n_buffers == 1, hasb};

    // The pair's two rows of a frame are requested a frame ahead (frame 0's here, in front of the ring's fill) and wanted
    // last: the loads fly while the transform before them runs and the finished samples go out.  Lane l, register r: bin
    // k = l + 64 r, for k > 512 bin N - k (stft::pack conjugates it).
    float2 xa[16], xb[16];
    auto request = [&](int f) {
        const float2* const rowa = rows + ((size_t)f * T + ta) * stft::kBins;
        const float2* const rowb = rowa + stft::kBins;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = lane + 64 * r;
            const int kk = k > stft::kN / 2 ? stft::kN - k : k;
            xa[r] = rowa[kk];
            xb[r] = hasb ? rowb[kk] : make_float2(0.0f, 0.0f);
        }
    };
    if (frames > 0) request(0);
    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = window[lane + 64 * r];
    float* const acca = acc + (size_t)ta * stft::kN;
    ring.fill(acca);
    stft::wave_sync();
    for (int f = 0; f < frames; ++f) {
        ring.emit(first_end + f * H);                      // the ring's front is now the frame's first sample
        cf z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            z[r] = stft::pack(fft::mk(xa[r].x, xa[r].y), fft::mk(xb[r].x, xb[r].y), lane + 64 * r);
        if (f + 1 < frames) request(f + 1);
        WF::run(z, img, t, lane);                          // EXEC is all ones here: every loop above has reconverged
        ring.add(z, g);
        stft::wave_sync();
    }
    ring.emit(n_buffers * B);                              // (the host holds it below 2^31 - 1024)
    ring.store(acca);
}

}  // namespace
}  // namespace gab

struct gab_resyn_plan {
    int tracks = 0, bufsize = 0, hop = 0;
    int phase = 0;                     // samples since the reset, mod hop
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::DeviceBuf<float> window;      // [1024]
    gab::DeviceBuf<float> acc;         // [T][1024]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch on s, from the plan's position; nothing is allocated, nothing waits.  *n_frames: host.
int resyn_launch(gab_resyn_plan* p, const float* d_rows, float* d_out, int n_buffers, int* n_frames, hipStream_t s,
                 const char* who) {
    if (int rc = stft::check_length(who, *p, n_buffers)) return rc;
    if (reinterpret_cast<uintptr_t>(d_rows) & 7u) return refuse(who, "d_rows must lie on an 8-byte boundary");
    const long long frames = stft::count(*p, n_buffers);
    if (frames > 0) {
        const uintptr_t r0 = reinterpret_cast<uintptr_t>(d_rows), o0 = reinterpret_cast<uintptr_t>(d_out);
        const uintptr_t rbytes = (uintptr_t)frames * (uintptr_t)p->tracks * stft::kBins * 2 * sizeof(float);
        const uintptr_t obytes = (uintptr_t)n_buffers * p->bufsize * p->tracks * sizeof(float);
        if (r0 < o0 + obytes && o0 < r0 + rbytes) return refuse(who, "d_rows and d_out overlap");
    }
    const unsigned groups = (unsigned)(((p->tracks + 1) / 2 + 3) / 4);
    resynthesis_kernel<<<dim3(groups), 256, 0, s>>>(reinterpret_cast<const float2*>(d_rows), p->acc.get(),
                                                    p->window.get(), d_out, p->tw, p->tracks, p->bufsize, n_buffers,
                                                    p->hop, stft::first_end(*p), (int)frames);
    if (int rc = launch_status("resynthesis_kernel")) return rc;
    stft::advance(*p, n_buffers);
    *n_frames = (int)frames;
    return GAB_OK;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_resyn_create(gab_resyn_plan** out, int tracks, int bufsize, int hop) {
    return gab::create_entry("gab_resyn_create", out, tracks, bufsize, [&] {
        if (int rc = gab::stft::check_hop("gab_resyn_create", hop)) return rc;
        if (tracks > gab::kResynMaxTracks)
            return gab::bad_arg("gab_resyn_create: more than 2^23 workgroups (tracks / 8) in one launch");
        return GAB_OK;
    }, [&](gab_resyn_plan& p) {
        p.hop = hop;
        p.tw = gab::fft::device_twiddles();
        p.window.alloc(gab::stft::kN);
        p.acc.alloc((size_t)tracks * gab::stft::kN);
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
        return gab::check_then(p->flag, s, who, d_src, (size_t)gab::stft::kN, gab::stft::WindowRule{0}, 0, [&] {
            GAB_HIP_CHECK(hipMemcpyAsync(p->window.get(), d_src, gab::stft::kN * sizeof(float), hipMemcpyDeviceToDevice, s));
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
    return gab::batch_entry("gab_resyn_frames", {plan, capacity}, n_buffers, [&] {
        return gab::stft::capacity("gab_resyn_frames", *plan, n_buffers, capacity);
    });
}

int gab_resyn_count(gab_resyn_plan* plan, int n_buffers, int* frames) {
    return gab::batch_entry("gab_resyn_count", {plan, frames}, n_buffers, [&]() -> int {
        const long long n = gab::stft::count(*plan, n_buffers);
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
        *samples = gab::stft::kN;
        return GAB_OK;
    });
}

}  // extern "C"
