// k_meter.hip — the meter plan: per track and buffer one row of eight levels {peak, true_peak, ms, kms, peak_hold,
// true_peak_max, kms_window, nonfinite} (include/gab_c_api.h, gab_meter_*).  One launch per call, a batch included; the
// input is read once and never written, and nothing is written but the rows and the carried state.
// No counterpart in the reference, whose gainstats is one stateless mean and max.
//
//   meter_kernel<VEC>     eq_sequential_kernel's tiles: a workgroup owns 64 tracks and walks the buffer in chunks of 64
//                         samples through an LDS tile.  Wave 0 owns the K filter in its ordered form, a lane per
//                         track, on the chunk in registers, and sums its squares there; waves 1..3 take the tile's
//                         rows in turn, a lane per sample, for peak, true peak, the sum of squares and the non-finite
//                         flag.  A row of the tile carries the track's last 11 samples in front of the chunk, so the
//                         true-peak taps read one contiguous run.  Buffers of a batch are more chunks of the same loop.
//   MeterRule             refuses a weighting outside the contract, naming the first value (gab_plan.hpp's check kernel).
//
// The K filter has no scan form: eq_scan_kernel's wave scan, restated for the two K sections, missed the bound the issue
// set per track and buffer at every buffer size (profiles/r11_meter.txt), so the ordered form runs at
// every size and every field is bit-identical to the header's restatement.  Every summation tree depends on bufsize
// alone: a track's bits do not depend on the track count, the input's alignment or how many buffers a call holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kMeterTracks = 64;          // tracks of a workgroup: the lanes of the filter wave
constexpr int kMeterChunk = 64;           // samples of a chunk: the lanes of a field wave, the segment of the sum trees
constexpr int kMeterHist = 11;            // samples carried per track: the true-peak taps reach back this far
constexpr int kMeterCol = 16;             // a tile row: [5 unused][11 carried samples][64 samples of the chunk]
constexpr int kMeterPitch = 84;           // floats: 16-byte aligned rows, b128 reads of 64 rows spread over the banks
constexpr int kMeterHistWords = 16;       // a d_hist row: 11 samples oldest first, peak_hold, true_peak_max, 3 zeros
constexpr int kMeterTaps = 12;            // per phase
constexpr int kMeterTapWords = 3 * kMeterTaps;
constexpr int kMeterCoeffWords = 12;      // [2][5] = {b0, b1, b2, a1, a2} per section, two words of padding
constexpr int kMeterMaxWindow = 64;
// The plan's constants: [36 taps][12].

// A hand-off through LDS inside the wave (k_delay.hip's): words that some lanes wrote or read are touched by other
// lanes next.
__device__ __forceinline__ void meter_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// One section, direct form II transposed, the header's roundings.
__device__ __forceinline__ float meter_section(const float* c, float x, float& s1, float& s2) {
    const float y = fmaf(c[0], x, s1);
    s1 = fmaf(c[1], x, fmaf(-c[3], y, s2));
    s2 = fmaf(c[2], x, __fmul_rn(-c[4], y));
    return y;
}

// Grid: x = group of 64 tracks.  in: [n][T][B], only read; VEC: 16-byte aligned and B a multiple of 4.  rows:
// [n][T][8].  hist: [T][16], filter: [T][2][2], ring: [T][W], pos: [T] (< W).  consts: [36 taps][12].
template <bool VEC>
__global__ __launch_bounds__(256) void meter_kernel(const float* __restrict__ in, float* __restrict__ rows,
                                                   float* __restrict__ hist, float* __restrict__ filter,
                                                   float* ring, unsigned* __restrict__ pos,
                                                   const float* __restrict__ consts, int T, int B, int W, int n_buffers,
                                                   float inv_B, float inv_W, float decay) {
    __shared__ __attribute__((aligned(16))) float tile[kMeterTracks][kMeterPitch];
    __shared__ float acc[kMeterTracks][4];                           // per row and buffer: peak, true peak, sum, flag
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blockIdx.x * kMeterTracks;
    const int nt = T - t0 < kMeterTracks ? T - t0 : kMeterTracks;     // tracks of this workgroup
    const float* taps = consts;
    const float* c0 = consts + kMeterTapWords;
    const float* c1 = c0 + 5;

    for (int idx = tid; idx < kMeterTracks * kMeterCol; idx += 256) {
        const int r = idx >> 4, c = idx & 15;
        tile[r][c] = (c >= 5 && r < nt) ? hist[(size_t)(t0 + r) * kMeterHistWords + (c - 5)] : 0.0f;
    }
    if (tid < kMeterTracks) { acc[tid][0] = 0.0f; acc[tid][1] = 0.0f; acc[tid][2] = 0.0f; acc[tid][3] = 0.0f; }
    // wave 0, lane = track: what is carried
    const bool owner = w == 0 && lane < nt;
    const size_t track = (size_t)t0 + lane;
    float s1a = 0.0f, s2a = 0.0f, s1b = 0.0f, s2b = 0.0f, hold = 0.0f, tpmax = 0.0f;
    int P = 0;
    if (owner) {
        const float* f = filter + track * 4;
        s1a = f[0]; s2a = f[1]; s1b = f[2]; s2b = f[3];
        hold = hist[track * kMeterHistWords + 11];
        tpmax = hist[track * kMeterHistWords + 12];
        P = (int)pos[track];
    }
    __syncthreads();

    const int nchunks = (B + kMeterChunk - 1) / kMeterChunk;
    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x0 = in + ((size_t)nb * T + t0) * B;
        float ksum = 0.0f;                                           // owner: the sum of the filtered squares so far
        for (int ch = 0; ch < nchunks; ++ch) {
            const int s0 = ch * kMeterChunk;
            const int len = B - s0 < kMeterChunk ? B - s0 : kMeterChunk;
            // ---- the chunk into the tile, zeros behind the buffer's end and below the last track ----
            if constexpr (VEC) {
                const int q = (tid & 15) * 4, rr = tid >> 4;
                float4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = rr + 16 * k;
                    v[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (r < nt && q < len) v[k] = *reinterpret_cast<const float4*>(x0 + (size_t)r * B + s0 + q);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(&tile[rr + 16 * k][kMeterCol + q]) = v[k];
            } else {
                float v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int r = w + 4 * k;
                    v[k] = (r < nt && lane < len) ? x0[(size_t)r * B + s0 + lane] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) tile[w + 4 * k][kMeterCol + lane] = v[k];
            }
            __syncthreads();
            if (w == 0) {
                // ---- the K filter, a lane per track, and the sum of its squares: a butterfly in registers ----
                if (owner) {
                    float x[kMeterChunk];
                    const float4* row = reinterpret_cast<const float4*>(&tile[lane][kMeterCol]);
#pragma unroll
                    for (int i = 0; i < kMeterChunk / 4; ++i) {
                        const float4 v = row[i];
                        x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
                    }
#pragma unroll
                    for (int i = 0; i < kMeterChunk; ++i) {
                        if (i < len) {                               // wave-uniform: the filter never runs on padding
                            const float y = meter_section(c1, meter_section(c0, x[i], s1a, s2a), s1b, s2b);
                            x[i] = __fmul_rn(y, y);
                        } else {
                            x[i] = 0.0f;
                        }
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
                        for (int i = 0; i < d; ++i) x[i] = __fadd_rn(x[i], x[i + d]);
                    ksum = __fadd_rn(ksum, x[0]);
                }
            } else {
                // ---- peak, true peak, sum of squares, non-finite: a lane per sample, the rows in turn ----
                for (int r = w - 1; r < nt; r += 3) {
                    float* row = tile[r];
                    float wnd[kMeterTaps];                           // wnd[j] = w[n - j]
#pragma unroll
                    for (int j = 0; j < kMeterTaps; ++j) wnd[j] = row[kMeterCol + lane - j];
                    const float nh = lane < kMeterHist ? row[5 + len + lane] : 0.0f;   // the last 11 samples so far
                    const float xv = wnd[0];
                    float tp = fabsf(wnd[5]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        float y = __fmul_rn(taps[k * kMeterTaps], wnd[0]);
#pragma unroll
                        for (int j = 1; j < kMeterTaps; ++j) y = fmaf(taps[k * kMeterTaps + j], wnd[j], y);
                        tp = fmaxf(tp, fabsf(y));
                    }
                    if (lane >= len) tp = 0.0f;
                    float pk = fabsf(xv), sq = __fmul_rn(xv, xv);
                    const bool nf = __ballot(not_finite(__float_as_uint(xv))) != 0;
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        pk = fmaxf(pk, __shfl_xor(pk, d, 64));
                        tp = fmaxf(tp, __shfl_xor(tp, d, 64));
                        sq = __fadd_rn(sq, __shfl_xor(sq, d, 64));
                    }
                    meter_wave_order();                              // every lane has read the row's front
                    if (lane < kMeterHist) row[5 + lane] = nh;
                    if (lane == 0) {
                        acc[r][0] = fmaxf(acc[r][0], pk);
                        acc[r][1] = fmaxf(acc[r][1], tp);
                        acc[r][2] = __fadd_rn(acc[r][2], sq);
                        if (nf) acc[r][3] = 1.0f;
                    }
                }
            }
            __syncthreads();
        }
        // ---- the row: wave 0, a lane per track ----
        if (owner) {
            const float pk = acc[lane][0], tp = acc[lane][1], nf = acc[lane][3];
            const float ms = __fmul_rn(acc[lane][2], inv_B), km = __fmul_rn(ksum, inv_B);
            acc[lane][0] = 0.0f; acc[lane][1] = 0.0f; acc[lane][2] = 0.0f; acc[lane][3] = 0.0f;
            hold = fmaxf(pk, __fmul_rn(hold, decay));
            tpmax = fmaxf(tpmax, tp);
            // the window: the newest value replaces the oldest, then oldest to newest in that order
            float* rg = ring + track * W;
            rg[P] = km;
            P = P + 1 == W ? 0 : P + 1;
            float sum = 0.0f;
            for (int k = 0; k < W; ++k) sum = __fadd_rn(sum, rg[P + k >= W ? P + k - W : P + k]);
            float* o = rows + ((size_t)nb * T + track) * GAB_METER_FIELDS;
            o[0] = pk; o[1] = tp; o[2] = ms; o[3] = km; o[4] = hold; o[5] = tpmax; o[6] = __fmul_rn(sum, inv_W); o[7] = nf;
        }
    }
    if (owner) {
        float* f = filter + track * 4;
        f[0] = s1a; f[1] = s2a; f[2] = s1b; f[3] = s2b;
        hist[track * kMeterHistWords + 11] = hold;
        hist[track * kMeterHistWords + 12] = tpmax;
        pos[track] = (unsigned)P;
    }
    for (int idx = tid; idx < kMeterTracks * kMeterCol; idx += 256) {
        const int r = idx >> 4, c = idx & 15;
        if (c >= 5 && r < nt) hist[(size_t)(t0 + r) * kMeterHistWords + (c - 5)] = tile[r][c];
    }
}

const char* const kMeterCoeff[5] = {"b0", "b1", "b2", "a1", "a2"};

// src: [2][5].  Refused: a value that is not finite; a2 with |a2| >= 1; a1 with |a1| >= 1 + a2 (asked only of a finite
// a2, which then is the value named).
struct MeterRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const int sec = (int)(i / 5), field = (int)(i % 5);
        const float v = src[i];
        bool bad = not_finite(__float_as_uint(v));
        const float a2f = src[sec * 5 + 4];
        const double a1 = src[sec * 5 + 3], a2 = a2f;
        if (field == 4) bad = bad || !(fabs(a2) < 1.0);
        if (field == 3 && !not_finite(__float_as_uint(a2f))) bad = bad || !(fabs(a1) < 1.0 + a2);
        return bad;
    }
    std::string refusal(unsigned i, int) const {
        const int field = (int)(i % 5u);
        return "section " + std::to_string((int)(i / 5u)) + " value " + std::to_string(field) + " (" + kMeterCoeff[field] +
               ") is not finite or outside the stability triangle (needs |a2| < 1 and |a1| < 1 + a2)"
               "; the plan keeps its weighting";
    }
};

// ITU-R BS.1770's K weighting at 48 kHz
const float kMeterDefault[10] = {1.53512485958697f, -2.69169618940638f, 1.19839281085285f, -1.69065929318241f,
                                 0.73248077421585f, 1.0f, -2.0f, 1.0f, -1.99004745483398f, 0.99007225036621f};

}  // namespace
}  // namespace gab

struct gab_meter_plan {
    int tracks = 0, bufsize = 0, window = 0;
    float inv_B = 0.0f, inv_W = 0.0f, decay = 1.0f;
    gab::DeviceBuf<float> consts;      // [36 taps][12: the two sections' coefficients]
    gab::DeviceBuf<float> hist;        // [T][16]
    gab::DeviceBuf<float> filter;      // [T][2][2]
    gab::DeviceBuf<float> ring;        // [T][window]
    gab::DeviceBuf<unsigned> pos;      // [T]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch; nothing is allocated, nothing waits
int meter_launch(gab_meter_plan* p, const float* d_in, float* d_rows, int n_buffers, hipStream_t s) {
    const dim3 grid((unsigned)((p->tracks + kMeterTracks - 1) / kMeterTracks));
    const bool vec = all_aligned16({d_in}) && p->bufsize % 4 == 0;
#define GAB_METER(VV)                                                                                              \
    meter_kernel<VV><<<grid, 256, 0, s>>>(d_in, d_rows, p->hist.get(), p->filter.get(), p->ring.get(),             \
                                          p->pos.get(), p->consts.get(), p->tracks, p->bufsize, p->window,        \
                                          n_buffers, p->inv_B, p->inv_W, p->decay)
    if (vec) GAB_METER(true); else GAB_METER(false);
#undef GAB_METER
    return launch_status("meter_kernel");
}

void meter_clear(gab_meter_plan* p, hipStream_t s) {
    GAB_HIP_CHECK(hipMemsetAsync(p->hist.get(), 0, p->hist.size() * sizeof(float), s));
    GAB_HIP_CHECK(hipMemsetAsync(p->filter.get(), 0, p->filter.size() * sizeof(float), s));
    GAB_HIP_CHECK(hipMemsetAsync(p->ring.get(), 0, p->ring.size() * sizeof(float), s));
    GAB_HIP_CHECK(hipMemsetAsync(p->pos.get(), 0, p->pos.size() * sizeof(unsigned), s));
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_meter_create(gab_meter_plan** out, int tracks, int bufsize, int window) {
    return gab::create_entry("gab_meter_create", out, tracks, bufsize, [&] {
        if (window < 1 || window > gab::kMeterMaxWindow) return gab::bad_arg("gab_meter_create: window must be 1..64");
        return GAB_OK;
    }, [&](gab_meter_plan& p) {
        p.window = window;
        p.inv_B = (float)(1.0 / (double)bufsize);
        p.inv_W = (float)(1.0 / (double)window);
        p.consts.alloc((size_t)gab::kMeterTapWords + gab::kMeterCoeffWords);
        p.hist.alloc((size_t)tracks * gab::kMeterHistWords);
        p.filter.alloc((size_t)tracks * 4);
        p.ring.alloc((size_t)tracks * window);
        p.pos.alloc((size_t)tracks);
        p.flag.alloc(1);
        // the true-peak taps: phase k = 1, 2, 3 of a 4x interpolator, 12 taps each, a Hann-like window of half-width
        // 6.5; float64, each phase divided by its sum (added in ascending j), rounded once
        float taps[gab::kMeterTapWords];
        const double pi = 3.14159265358979323846;
        for (int k = 1; k <= 3; ++k) {
            double h[gab::kMeterTaps], sum = 0.0;
            for (int j = 0; j < gab::kMeterTaps; ++j) {
                const double d = 5.0 + (double)k / 4.0 - (double)j;
                h[j] = std::sin(pi * d) / (pi * d) * (0.5 + 0.5 * std::cos(pi * d / 6.5));
                sum += h[j];
            }
            for (int j = 0; j < gab::kMeterTaps; ++j) taps[(k - 1) * gab::kMeterTaps + j] = (float)(h[j] / sum);
        }
        GAB_HIP_CHECK(hipMemcpy(p.consts.get(), taps, sizeof(taps), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.consts.get() + gab::kMeterTapWords, 0, gab::kMeterCoeffWords * sizeof(float)));
        GAB_HIP_CHECK(hipMemcpy(p.consts.get() + gab::kMeterTapWords, gab::kMeterDefault, sizeof(gab::kMeterDefault),
                                hipMemcpyHostToDevice));
        gab::meter_clear(&p, nullptr);
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_meter_destroy(gab_meter_plan* plan) { return gab::destroy_plan(plan, "gab_meter_destroy: null pointer"); }

// check, then commit (gab_plan.hpp): a refused set leaves the rows as they were
int gab_meter_set_weighting(gab_meter_plan* plan, const float* d_sections, gab_stream_t stream) {
    return gab::entry("gab_meter_set_weighting", {plan, d_sections}, [&] {
        hipStream_t s = gab::as_stream(stream);
        return gab::check_then(plan->flag, s, "gab_meter_set_weighting", d_sections, 10, gab::MeterRule{}, 0, [&] {
            GAB_HIP_CHECK(hipMemcpyAsync(plan->consts.get() + gab::kMeterTapWords, d_sections, 10 * sizeof(float),
                                         hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int gab_meter_set_decay(gab_meter_plan* plan, float decay, gab_stream_t) {
    return gab::guarded([&]() -> int {
        if (!(decay >= 0.0f && decay <= 1.0f)) return gab::bad_arg("gab_meter_set_decay: decay must be within [0, 1]");
        if (!plan) return gab::bad_arg("gab_meter_set_decay: null pointer");
        plan->decay = decay;                // a launch argument: in force from the next process call
        return GAB_OK;
    });
}

int gab_meter_reset(gab_meter_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_meter_reset", {plan}, [&] {
        gab::meter_clear(plan, gab::as_stream(stream));
        return GAB_OK;
    });
}

int gab_meter_process(gab_meter_plan* plan, const float* d_in, float* d_rows, gab_stream_t stream) {
    return gab::entry("gab_meter_process", {plan, d_in, d_rows},
                      [&] { return gab::meter_launch(plan, d_in, d_rows, 1, gab::as_stream(stream)); });
}

int gab_meter_process_batch(gab_meter_plan* plan, const float* d_in, float* d_rows, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_meter_process_batch", {plan, d_in, d_rows}, n_buffers,
                            [&] { return gab::meter_launch(plan, d_in, d_rows, n_buffers, gab::as_stream(stream)); });
}

int gab_meter_state(gab_meter_plan* plan, float** d_hist, float** d_filter, float** d_ring, unsigned** d_pos) {
    return gab::entry("gab_meter_state", {plan, d_hist, d_filter, d_ring, d_pos}, [&] {
        *d_hist = plan->hist.get();
        *d_filter = plan->filter.get();
        *d_ring = plan->ring.get();
        *d_pos = plan->pos.get();
        return GAB_OK;
    });
}

}  // extern "C"
