// k_resample.hip — the resample plan: every track's stream from one sample rate to another by the rational factor
// L / M, a polyphase FIR whose tap row changes with every output sample (include/gab_c_api.h, gab_resample_*).  One
// launch per call, a batch included; the input is read once and never written.  No counterpart in the reference, which
// changes no stream's rate.
//
//   resample_kernel        the meter's tiles: a workgroup owns 64 tracks and walks the buffer in chunks of 64 input
//                          samples through an LDS tile whose rows carry the track's last K-1 samples in front of the
//                          chunk.  A lane is a track: output m has the same (i, p) on every track, so the position is
//                          wave-uniform, the tap row h_p arrives by scalar loads as the fmaf's scalar operand, and the
//                          K samples come from the lane's own tile row, two to an 8-byte LDS read.  All four waves walk
//                          the positions (scalar arithmetic); wave w computes every fourth output.  Outputs are turned
//                          through a second tile, 64 at a time, so that a row is stored 64 consecutive floats at once.
//   ResampleRule           refuses a tap table with a value that is not finite, naming the first (gab_plan.hpp's check
//                          kernel).
//
// The position of the next output, (i - first sample of the chunk, p), is carried in 32-bit integers by adding
// (M / L, M mod L) with a carry: no division on the device.  The host passes the position of the launch's first output;
// the buffers of a batch are more chunks of the same loop.  The chain of one output is the header's, whichever wave
// computes it, so the bits depend on nothing but the contract.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"
#include "gab_resample_design.hpp"    // resample_design: the header's taps, shared with the saturator plan

namespace gab {
namespace {

constexpr int kRsTracks = 64;            // tracks of a workgroup: the lanes of a wave
constexpr int kRsChunk = 64;              // input samples of a chunk
constexpr int kRsBatch = 64;              // outputs turned through the output tile at once
constexpr int kRsOutPitch = 65;           // floats: a lane per row writes, a lane per column reads, both over all banks
constexpr int kRsMaxRatio = 1024;
constexpr int kRsMaxTaps = 256;
constexpr int kRsMaxTable = 16384;        // floats: 64 KiB, the table a lane-per-output form would hold in LDS
constexpr int kRsMaxBufsize = 1 << 20;    // bufsize * L stays below 2^31

// A tile row: [1 unused][K-1 carried samples][64 samples of the chunk], K even, so the chunk starts at an even column.
// The pitch is twice an odd number: rows are 8-byte aligned and the 8-byte reads of 32 lanes, a row each at the same
// column, fall on 32 different pairs of the 64 banks.
__host__ __device__ constexpr int resample_pitch(int K) { return K + kRsChunk + ((K & 3) == 0 ? 2 : 0); }

constexpr size_t resample_lds_bytes(int K) {
    return ((size_t)kRsTracks * resample_pitch(K) + (size_t)kRsTracks * kRsOutPitch) * sizeof(float);
}

// y = fmaf(h[K-1], w[i-K+1], ... fmaf(h[1], w[i-1], h[0] * w[i])): row[c] is w[i], h is wave-uniform.
__device__ __forceinline__ float resample_chain(const float* __restrict__ h, const float* row, int c, int K) {
    float y;
    if (c & 1) {                                                     // wave-uniform: (c-1, c) is an aligned pair
        const float2 v0 = *reinterpret_cast<const float2*>(row + c - 1);
        y = fmaf(h[1], v0.x, __fmul_rn(h[0], v0.y));
#pragma unroll 4
        for (int j = 2; j < K; j += 2) {
            const float2 v = *reinterpret_cast<const float2*>(row + c - 1 - j);
            y = fmaf(h[j + 1], v.x, fmaf(h[j], v.y, y));
        }
    } else {                                                         // w[i] and w[i-K+1] alone, aligned pairs between
        y = __fmul_rn(h[0], row[c]);
#pragma unroll 4
        for (int j = 1; j < K - 1; j += 2) {
            const float2 v = *reinterpret_cast<const float2*>(row + c - 1 - j);
            y = fmaf(h[j + 1], v.x, fmaf(h[j], v.y, y));
        }
        y = fmaf(h[K - 1], row[c - K + 1], y);
    }
    return y;
}

// Grid: x = group of 64 tracks.  in: [n][T][B], only read.  out: [n][T][OC].  hist: [T][K-1].  taps: [L][K].
// (Mq, Mr) = (M / L, M mod L).  (ic, p): the launch's first output lies at input sample ic of its first buffer, phase p.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      float* __restrict__ hist, const float* __restrict__ taps, int T,
                                                      int B, int L, int Mq, int Mr, int K, int OC, int n_buffers,
                                                      int ic, int p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int pitch = resample_pitch(K);
    float* tile = lds;
    float* otile = lds + kRsTracks * pitch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * kRsTracks;
    const int nt = T - t0 < kRsTracks ? T - t0 : kRsTracks;          // tracks of this workgroup
    const int H = K - 1;

    for (int r = w; r < kRsTracks; r += 4)
        for (int c = lane; c < K; c += 64)
            tile[r * pitch + c] = (c >= 1 && r < nt) ? hist[(size_t)(t0 + r) * H + (c - 1)] : 0.0f;

    const float* row = tile + lane * pitch;
    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x0 = in + ((size_t)nb * T + t0) * B;
        float* o0 = out + ((size_t)nb * T + t0) * OC;
        int done = 0;                                                // outputs of this buffer so far
        for (int s0 = 0; s0 < B; s0 += kRsChunk) {
            const int len = B - s0 < kRsChunk ? B - s0 : kRsChunk;
            // ---- the chunk into the tile, zeros behind the buffer's end and below the last track ----
            {
                float v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int r = w + 4 * k;
                    v[k] = (r < nt && lane < len) ? x0[(size_t)r * B + s0 + lane] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) tile[(w + 4 * k) * pitch + K + lane] = v[k];
            }
            __syncthreads();
            // ---- the outputs whose newest sample lies in the chunk, 64 at a time ----
            while (ic < len) {
                int n = 0;
                do {
                    if ((n & 3) == w) otile[lane * kRsOutPitch + n] = resample_chain(taps + p * K, row, K + ic, K);
                    ++n;
                    p += Mr;
                    ic += Mq;
                    if (p >= L) { p -= L; ++ic; }
                } while (ic < len && n < kRsBatch);
                __syncthreads();
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int r = w + 4 * k;
                    if (r < nt && lane < n) o0[(size_t)r * OC + done + lane] = otile[r * kRsOutPitch + lane];
                }
                done += n;
                __syncthreads();
            }
            ic -= len;
            // ---- the last K-1 samples so far move to the front of the rows, 64 columns at a time, lowest first ----
            for (int q = 0; q < H; q += 64) {
                const int c = q + lane;
                float nh[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) nh[k] = c < H ? tile[(w + 4 * k) * pitch + 1 + len + c] : 0.0f;
                __syncthreads();
                if (c < H) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) tile[(w + 4 * k) * pitch + 1 + c] = nh[k];
                }
                __syncthreads();
            }
        }
        // ---- the rest of every row is defined: zeros ----
        if (tid < nt)
            for (int c = done; c < OC; ++c) o0[(size_t)tid * OC + c] = 0.0f;
    }
    for (int r = w; r < nt; r += 4)
        for (int c = lane; c < H; c += 64) hist[(size_t)(t0 + r) * H + c] = tile[r * pitch + 1 + c];
}

// src: [phases][taps]
struct ResampleRule {
    unsigned taps;                  // for the text only
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int) const {
        return "phase " + std::to_string(i / taps) + " tap " + std::to_string(i % taps) +
               " is not finite; the plan keeps its taps";
    }
};

int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

}  // namespace
}  // namespace gab

struct gab_resample_plan {
    int tracks = 0, bufsize = 0, L = 0, M = 0, K = 0, out_capacity = 0, period = 0;
    long long k = 0;                   // buffers since the reset, mod period
    gab::DeviceBuf<float> taps;        // [L][K]
    gab::DeviceBuf<float> hist;        // [T][K-1]
    gab::DeviceBuf<unsigned> flag;

    // lo(k) = ceil(k B L / M) for 0 <= k <= 2 period: below 2^42
    long long lo(long long kk) const { return gab::ceil_div(kk * bufsize * L, M); }
    int count(long long kk) const { return (int)(lo(kk + 1) - lo(kk)); }
};

namespace gab {
namespace {

// n buffers in one launch, from the plan's position; nothing is allocated, nothing waits.  counts: [n], host.
int resample_launch(gab_resample_plan* p, const float* d_in, float* d_out, int n_buffers, int* counts, hipStream_t s) {
    // the first output of buffer k: m = lo(k), at m M - k B L of an input sample's L parts, below M
    const long long pos = p->lo(p->k) * p->M - p->k * p->bufsize * p->L;
    const dim3 grid((unsigned)((p->tracks + kRsTracks - 1) / kRsTracks));
    resample_kernel<<<grid, 256, resample_lds_bytes(p->K), s>>>(d_in, d_out, p->hist.get(), p->taps.get(), p->tracks,
                                                               p->bufsize, p->L, p->M / p->L, p->M % p->L, p->K,
                                                               p->out_capacity, n_buffers, (int)(pos / p->L),
                                                               (int)(pos % p->L));
    if (int rc = launch_status("resample_kernel")) return rc;
    long long k = p->k;
    for (int i = 0; i < n_buffers; ++i) {
        counts[i] = p->count(k);
        k = (k + 1) % p->period;
    }
    p->k = k;
    return GAB_OK;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_resample_create(gab_resample_plan** out, int tracks, int bufsize, int up, int down, int taps) {
    int L = 0, M = 0;               // up and down, reduced
    return gab::create_entry("gab_resample_create", out, tracks, bufsize, [&] {
        if (bufsize > gab::kRsMaxBufsize) return gab::bad_arg("gab_resample_create: bufsize must be <= 2^20");
        if (up < 1 || up > gab::kRsMaxRatio || down < 1 || down > gab::kRsMaxRatio)
            return gab::bad_arg("gab_resample_create: up and down must be 1..1024");
        if (taps < 4 || taps > gab::kRsMaxTaps || taps % 2 != 0)
            return gab::bad_arg("gab_resample_create: taps must be even and 4..256");
        const int g = gab::gcd_int(up, down);
        L = up / g; M = down / g;
        if (L * taps > gab::kRsMaxTable) {
            gab::set_last_error("gab_resample_create: a table of up * taps = " + std::to_string(L * taps) +
                                " floats (up reduced) is more than 16384");
            return GAB_ERR_UNSUPPORTED;
        }
        return GAB_OK;
    }, [&](gab_resample_plan& p) {
        p.L = L; p.M = M; p.K = taps;
        const long long BL = (long long)bufsize * L;
        p.out_capacity = (int)gab::ceil_div(BL, M);
        p.period = M / gab::gcd_int((int)(BL % M), M);
        const size_t lds = gab::resample_lds_bytes(taps);
        if (lds > 64 * 1024)
            GAB_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gab::resample_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        p.taps.alloc((size_t)L * taps);
        p.hist.alloc((size_t)tracks * (taps - 1));
        p.flag.alloc(1);
        const std::vector<float> h = gab::resample_design(L, M, taps);
        GAB_HIP_CHECK(hipMemcpy(p.taps.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.hist.get(), 0, p.hist.size() * sizeof(float)));
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_resample_destroy(gab_resample_plan* plan) {
    return gab::destroy_plan(plan, "gab_resample_destroy: null pointer");
}

int gab_resample_shape(gab_resample_plan* plan, int* up, int* down, int* taps, int* out_capacity, int* period) {
    return gab::entry("gab_resample_shape", {plan, up, down, taps, out_capacity, period}, [&] {
        *up = plan->L; *down = plan->M; *taps = plan->K; *out_capacity = plan->out_capacity; *period = plan->period;
        return GAB_OK;
    });
}

// check, then commit (gab_plan.hpp): a refused table leaves the plan's as it was
int gab_resample_set_taps(gab_resample_plan* plan, const float* d_taps, gab_stream_t stream) {
    return gab::entry("gab_resample_set_taps", {plan, d_taps}, [&] {
        hipStream_t s = gab::as_stream(stream);
        const size_t n = (size_t)plan->L * plan->K;
        const gab::ResampleRule rule{(unsigned)plan->K};
        return gab::check_then(plan->flag, s, "gab_resample_set_taps", d_taps, n, rule, 0, [&] {
            GAB_HIP_CHECK(hipMemcpyAsync(plan->taps.get(), d_taps, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int gab_resample_reset(gab_resample_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_resample_reset", {plan}, [&] {
        GAB_HIP_CHECK(hipMemsetAsync(plan->hist.get(), 0, plan->hist.size() * sizeof(float), gab::as_stream(stream)));
        plan->k = 0;
        return GAB_OK;
    });
}

int gab_resample_process(gab_resample_plan* plan, const float* d_in, float* d_out, int* n_out, gab_stream_t stream) {
    return gab::entry("gab_resample_process", {plan, d_in, d_out, n_out},
                      [&] { return gab::resample_launch(plan, d_in, d_out, 1, n_out, gab::as_stream(stream)); });
}

int gab_resample_process_batch(gab_resample_plan* plan, const float* d_in, float* d_out, int n_buffers, int* counts,
                               gab_stream_t stream) {
    return gab::batch_entry("gab_resample_process_batch", {plan, d_in, d_out, counts}, n_buffers, [&] {
        return gab::resample_launch(plan, d_in, d_out, n_buffers, counts, gab::as_stream(stream));
    });
}

int gab_resample_state(gab_resample_plan* plan, float** d_hist, float** d_taps, long long* buffers_since_reset_mod_period) {
    return gab::entry("gab_resample_state", {plan, d_hist, d_taps, buffers_since_reset_mod_period}, [&] {
        *d_hist = plan->hist.get();
        *d_taps = plan->taps.get();
        *buffers_since_reset_mod_period = plan->k;
        return GAB_OK;
    });
}

}  // extern "C"
