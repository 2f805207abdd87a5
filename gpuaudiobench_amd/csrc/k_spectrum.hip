// k_spectrum.hip — the spectrum plan: a short-time Fourier analyser per track (include/gab_c_api.h, gab_spec_*).
// Frames of N = 1024 samples on a hop grid H, windowed, transformed, and written as complex bins, as powers per bin or
// as powers per band; the last 1023 samples of every track are carried on the device, so a frame reaches back over the
// calls before it.  The input is read and never written.  No counterpart in the reference, whose FFT benchmark is one
// stateless transform of 1024 samples.
//
//   spectrum_kernel<MODE>   one wave per (pair of tracks, frame), four waves a workgroup, no workgroup barrier: lane j
//                           gathers s[jH - N + j + 64 r] of both tracks (from the carried history where the index
//                           lies before the call, else from the call's blocks, across the buffers of a batch),
//                           multiplies by the window, runs gab_fft.hpp's wave-held 1024-point transform, unpacks the
//                           pair as fft_r2c_1024_kernel does, and writes the bins, their powers, or (through the
//                           wave's LDS image, lane b adding band b in order) the bands.
//   spectrum_hist_kernel    behind it on the same stream: a wave per track forms the last 1023 samples of
//                           history ++ call in registers and writes them only after every lane has read.
// The gather, the transform and the unpack, the power of a bin, the history update and the window rule are gab_stft.hpp's,
// which the denoise plan shares.
//
// A frame's bits depend on its pair's 1024 windowed samples (and, for powers, on the window's sum) and on nothing else:
// not on bufsize, the hop, the cut into calls, the alignment of d_in or the other frames of the launch.  Every frame
// takes the same scalar gather; there is no 16-byte load form (a lane's sixteen values lie 64 samples
// apart, so a float4 per lane would have to cross the wave through LDS first).
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

constexpr int kSpecMaxBands = 64;                         // a lane per band
constexpr unsigned kSpecMaxBlocks = 1u << 23;             // workgroups of one launch: 2^31 threads
enum { kSpecComplex = 0, kSpecBinsMode = 1, kSpecBandsMode = 2 };

// Grid: x = (group of four pairs) * frames + frame.  in: [n][T][B], only read.  hist: [T][1023], only read.  window:
// [1024].  Frame f ends `first_end + f H` samples behind the call's first (1 <= first_end; the last end <= n B).
// rows: [frames][T][513][2], [frames][T][513] or [frames][T][bands].  edges: [bands + 1].
template <int MODE>
__global__ __launch_bounds__(256) void spectrum_kernel(const float* __restrict__ in, const float* __restrict__ hist,
                                                      const float* __restrict__ window, const int* __restrict__ edges,
                                                      float* __restrict__ rows, const cf* __restrict__ tw, int T, int B,
                                                      int n_buffers, int H, int first_end, int frames, int bands,
                                                      float inv_edge, float inv_mid) {
    __shared__ cf lds[4 * stft::kImg];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    const int f = (int)(blockIdx.x % (unsigned)frames);
    const int q = (int)(blockIdx.x / (unsigned)frames) * 4 + w;
    const int ta = 2 * q;
    if (ta >= T) return;                                   // whole wave; no barriers below
    const bool hasb = ta + 1 < T;
    const int start = first_end + f * H - stft::kN;        // of the frame, relative to the call's first sample

    using WF = fft::WaveFFT1024<false>;
    WF::Twiddles t;
    WF::load_twiddles(t, tw, lane);
    float wn[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) wn[r] = window[lane + 64 * r];
    cf xa[9], xb[9];
    stft::analyse(in, hist, T, B, n_buffers == 1, ta, hasb, start, wn, img, t, lane, xa, xb);
    if constexpr (MODE == kSpecComplex) {
        float2* const oa = reinterpret_cast<float2*>(rows) + ((size_t)f * T + ta) * stft::kBins;
        float2* const ob = oa + stft::kBins;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            if (k <= stft::kN / 2) {
                oa[k] = make_float2(xa[r].x, xa[r].y);
                if (hasb) ob[k] = make_float2(xb[r].x, xb[r].y);
            }
        }
    } else {
        float pa[9], pb[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const float inv = stft::inv_of(lane + 64 * r, inv_edge, inv_mid);
            pa[r] = stft::power(xa[r].x, xa[r].y, inv);
            pb[r] = stft::power(xb[r].x, xb[r].y, inv);
        }
        if constexpr (MODE == kSpecBinsMode) {
            float* const oa = rows + ((size_t)f * T + ta) * stft::kBins;
            float* const ob = oa + stft::kBins;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int k = lane + 64 * r;
                if (k <= stft::kN / 2) {
                    oa[k] = pa[r];
                    if (hasb) ob[k] = pb[r];
                }
            }
        } else {
            // the powers through the wave's image (every lane has read its partners), then lane b adds band b in order
            float* const pw = reinterpret_cast<float*>(img);          // [2][576]
            stft::wave_sync();
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int k = lane + 64 * r;
                pw[k] = pa[r];
                pw[576 + k] = pb[r];
            }
            stft::wave_sync();
            if (lane < bands) {
                const int e0 = edges[lane], e1 = edges[lane + 1];
                float sa = 0.0f, sb = 0.0f;
                for (int k = e0; k < e1; ++k) {
                    sa = __fadd_rn(sa, pw[k]);
                    sb = __fadd_rn(sb, pw[576 + k]);
                }
                float* const oa = rows + ((size_t)f * T + ta) * bands;
                oa[lane] = sa;
                if (hasb) oa[bands + lane] = sb;
            }
        }
    }
}

// Grid: x = group of four tracks, a wave per track.  hist: [T][1023] becomes the last 1023 samples of hist ++ the call's
// n B samples: every value is in a register before any is written.
__global__ __launch_bounds__(256) void spectrum_hist_kernel(const float* __restrict__ in, float* hist, int T, int B,
                                                           int n_buffers) {
    const int lane = threadIdx.x & 63;
    const int t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    float v[16];
    stft::hist_read(v, in, hist, T, B, n_buffers == 1, t, t < T, n_buffers * B, lane);   // (n B < 2^31 - 1024: the host)
    __syncthreads();
    if (t < T) stft::hist_write(v, hist, t, lane);
}

}  // namespace
}  // namespace gab

struct gab_spec_plan {
    int tracks = 0, bufsize = 0, hop = 0, mode = 0, bands = 0;
    int phase = 0;                     // samples since the reset, mod hop
    float inv_edge = 0.0f, inv_mid = 0.0f;     // (float)(1 / S^2), (float)(4 / S^2)
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::DeviceBuf<float> window;      // [1024]
    gab::DeviceBuf<float> hist;        // [T][1023]
    gab::DeviceBuf<int> edges;         // [65]
    gab::DeviceBuf<unsigned> flag;

    int width() const {
        return mode == GAB_SPEC_COMPLEX ? 2 * gab::stft::kBins : bands ? bands : gab::stft::kBins;
    }
};

namespace gab {
namespace {

// The edge rule: 0 <= e_0 < e_1 < ... < e_bands <= 513.  The first value that breaks it, or -1.
int spectrum_bad_edge(const int* e, int bands) {
    for (int b = 0; b <= bands; ++b) {
        if (e[b] < 0 || e[b] > stft::kBins) return b;
        if (b > 0 && e[b] <= e[b - 1]) return b;
    }
    return -1;
}

// n buffers in two launches on s (the frames, then the history), from the plan's position; nothing is allocated,
// nothing waits.  *n_frames: host.
int spectrum_launch(gab_spec_plan* p, const float* d_in, float* d_rows, int n_buffers, int* n_frames, hipStream_t s,
                    const char* who) {
    if (int rc = stft::check_length(who, *p, n_buffers)) return rc;
    const long long frames = stft::count(*p, n_buffers);
    const long long groups = ((p->tracks + 1) / 2 + 3) / 4;
    if (frames * groups > (long long)kSpecMaxBlocks)
        return refuse(who, "more than 2^23 workgroups (frames x tracks / 8) in one call");
    if (frames > 0) {
        const dim3 grid((unsigned)(frames * groups));
        const int first_end = stft::first_end(*p);
#define GAB_SPEC(MM)                                                                                                   \
    spectrum_kernel<MM><<<grid, 256, 0, s>>>(d_in, p->hist.get(), p->window.get(), p->edges.get(), d_rows, p->tw,        \
                                             p->tracks, p->bufsize, n_buffers, p->hop, first_end, (int)frames,           \
                                             p->bands, p->inv_edge, p->inv_mid)
        if (p->mode == GAB_SPEC_COMPLEX) GAB_SPEC(kSpecComplex);
        else if (p->bands == 0) GAB_SPEC(kSpecBinsMode);
        else GAB_SPEC(kSpecBandsMode);
#undef GAB_SPEC
        if (int rc = launch_status("spectrum_kernel")) return rc;
    }
    spectrum_hist_kernel<<<dim3((unsigned)((p->tracks + 3) / 4)), 256, 0, s>>>(d_in, p->hist.get(), p->tracks,
                                                                              p->bufsize, n_buffers);
    if (int rc = launch_status("spectrum_hist_kernel")) return rc;
    stft::advance(*p, n_buffers);
    *n_frames = (int)frames;
    return GAB_OK;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_spec_create(gab_spec_plan** out, int tracks, int bufsize, int hop, int mode, int bands) {
    return gab::create_entry("gab_spec_create", out, tracks, bufsize, [&] {
        if (int rc = gab::stft::check_hop("gab_spec_create", hop)) return rc;
        if (mode != GAB_SPEC_COMPLEX && mode != GAB_SPEC_POWER)
            return gab::bad_arg("gab_spec_create: mode must be GAB_SPEC_COMPLEX or GAB_SPEC_POWER");
        if (bands < 0 || bands > gab::kSpecMaxBands) return gab::bad_arg("gab_spec_create: bands must be 0..64");
        if (mode == GAB_SPEC_COMPLEX && bands != 0)
            return gab::bad_arg("gab_spec_create: bands need GAB_SPEC_POWER (complex rows have no band form)");
        return GAB_OK;
    }, [&](gab_spec_plan& p) {
        p.hop = hop; p.mode = mode; p.bands = bands;
        p.tw = gab::fft::device_twiddles();
        p.window.alloc(gab::stft::kN);
        p.hist.alloc((size_t)tracks * gab::stft::kHist);
        p.edges.alloc(gab::kSpecMaxBands + 1);
        p.flag.alloc(1);
        // the periodic Hann window, float64, rounded once; S added in ascending n over the rounded values
        const std::vector<float> w = gab::stft_hann();
        gab::stft::scale(p, gab::stft_window_sum(w));
        int e[gab::kSpecMaxBands + 1] = {0};
        for (int b = 0; b <= bands; ++b) e[b] = bands ? (int)((long long)gab::stft::kBins * b / bands) : 0;
        GAB_HIP_CHECK(hipMemcpy(p.window.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemcpy(p.edges.get(), e, sizeof(e), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.hist.get(), 0, p.hist.size() * sizeof(float)));
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_spec_destroy(gab_spec_plan* plan) { return gab::destroy_plan(plan, "gab_spec_destroy: null pointer"); }

// check, then commit (gab_plan.hpp): a refused window, by the device's rule or by the host's on its sum, leaves the
// plan's as it was
int gab_spec_set_window(gab_spec_plan* plan, const float* d_window, gab_stream_t stream) {
    return gab::set_entry("gab_spec_set_window",
                          [&](gab_spec_plan* p, const float* d_src, int, int, const char* who) -> int {
        hipStream_t s = gab::as_stream(stream);
        bool zero_sum = false;
        const int rc = gab::check_then(p->flag, s, who, d_src, (size_t)gab::stft::kN, gab::stft::WindowRule{0}, 0, [&] {
            std::vector<float> w(gab::stft::kN);
            GAB_HIP_CHECK(hipMemcpyAsync(w.data(), d_src, w.size() * sizeof(float), hipMemcpyDeviceToHost, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
            const double S = gab::stft_window_sum(w);
            if (S == 0.0) { zero_sum = true; return; }
            GAB_HIP_CHECK(hipMemcpyAsync(p->window.get(), d_src, w.size() * sizeof(float), hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
            gab::stft::scale(*p, S);
        });
        if (rc) return rc;
        if (zero_sum) return gab::refuse(who, "the window's sum is zero; the plan keeps its window");
        return GAB_OK;
    }, plan, d_window, true, 0, 0);
}

int gab_spec_set_bands(gab_spec_plan* plan, const int* h_edges) {
    return gab::entry("gab_spec_set_bands", {plan, h_edges}, [&]() -> int {
        if (plan->bands == 0) return gab::refuse("gab_spec_set_bands", "the plan has no bands");
        const int bad = gab::spectrum_bad_edge(h_edges, plan->bands);
        if (bad >= 0) {
            gab::set_last_error("gab_spec_set_bands: edge " + std::to_string(bad) + " (" + std::to_string(h_edges[bad]) +
                                ") breaks 0 <= e_0 < e_1 < ... < e_bands <= 513; the plan keeps its edges");
            return GAB_ERR_INVALID_ARG;
        }
        GAB_HIP_CHECK(hipMemcpy(plan->edges.get(), h_edges, (size_t)(plan->bands + 1) * sizeof(int),
                                hipMemcpyHostToDevice));
        return GAB_OK;
    });
}

int gab_spec_reset(gab_spec_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_spec_reset", {plan}, [&] {
        GAB_HIP_CHECK(hipMemsetAsync(plan->hist.get(), 0, plan->hist.size() * sizeof(float), gab::as_stream(stream)));
        plan->phase = 0;
        return GAB_OK;
    });
}

int gab_spec_process(gab_spec_plan* plan, const float* d_in, float* d_rows, int* n_frames, gab_stream_t stream) {
    return gab::entry("gab_spec_process", {plan, d_in, d_rows, n_frames}, [&] {
        return gab::spectrum_launch(plan, d_in, d_rows, 1, n_frames, gab::as_stream(stream), "gab_spec_process");
    });
}

int gab_spec_process_batch(gab_spec_plan* plan, const float* d_in, float* d_rows, int n_buffers, int* n_frames,
                           gab_stream_t stream) {
    return gab::batch_entry("gab_spec_process_batch", {plan, d_in, d_rows, n_frames}, n_buffers, [&] {
        return gab::spectrum_launch(plan, d_in, d_rows, n_buffers, n_frames, gab::as_stream(stream),
                                    "gab_spec_process_batch");
    });
}

int gab_spec_frames(gab_spec_plan* plan, int n_buffers, int* capacity) {
    return gab::batch_entry("gab_spec_frames", {plan, capacity}, n_buffers, [&] {
        return gab::stft::capacity("gab_spec_frames", *plan, n_buffers, capacity);
    });
}

int gab_spec_state(gab_spec_plan* plan, float** d_hist, float** d_window, int* position_mod_hop) {
    return gab::entry("gab_spec_state", {plan, d_hist, d_window, position_mod_hop}, [&] {
        *d_hist = plan->hist.get();
        *d_window = plan->window.get();
        *position_mod_hop = plan->phase;
        return GAB_OK;
    });
}

}  // extern "C"
