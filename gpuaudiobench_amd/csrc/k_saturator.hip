// k_saturator.hip — the saturator plan: per track an interpolator by R, a waveshaper {drive, bias, level} on the
// oversampled samples and a decimator by R, in one launch; bit for bit the composition resample plan (up R) ->
// gab_sat_apply -> resample plan (down R) (include/gab_c_api.h, gab_sat_*).  No counterpart in the
// reference.
//
//   sat_fused_kernel<R, CURVE, RAMP>  a workgroup of 256 lanes OWNS 16 tracks for the whole launch, every buffer of a
//                          batch included: it alone reads their two histories (at its start) and writes them (at its end),
//                          so there is no second launch and no lane stores a history word that another still has to load.
//                          It walks the tracks in chunks of 64 base samples through two LDS tiles whose rows carry the
//                          histories in front: [Ku-1 inputs][64 inputs] and [Kd-1 shaped][64 R shaped].  Per chunk:
//                            1. the chunk into the input tile (a row's 64 samples by 16 lanes, 16 bytes each);
//                            2. a lane owns 4 consecutive base samples of one track: it walks the Ku taps once with a
//                               window of 4 inputs in registers, one new LDS word per tap for 4 R fmaf, the tap a
//                               wave-uniform scalar operand; the 4 R values through the curve into the second tile;
//                            3. behind a barrier the same lane forms its 4 base outputs: Kd / R blocks of R taps, a window
//                               of 4 R shaped values in registers of which R are new per block (one 8- or 16-byte LDS
//                               read for 4 R fmaf); outputs into a third tile, the tails of both tiles into registers;
//                            4. behind a barrier the tails go to the front of the rows (the histories are shifted, not
//                               replaced: a chunk may be shorter than a history) and the outputs leave as they came in.
//                          Lanes 0..15 of every 16 are 16 different rows, and the row pitch of the shaped tile is 4 floats
//                          off a multiple of 64: the wide reads of step 3 spread over the banks.
//   sat_apply_kernel<CURVE, RAMP, VEC>  the curve alone on oversampled blocks, an element (or four) per lane.
//   SatParamRule, SatTapsRule          refuse a row or a tap that is not finite, naming the first (gab_plan.hpp).
//
// The chain of one sample is the header's whichever lane computes it, and the ramp row of a base sample depends on its
// position in the buffer alone: the bits depend on nothing but the contract.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"
#include "gab_resample_design.hpp"

namespace gab {
namespace {

constexpr int kSatTracks = 16;            // tracks of a workgroup
constexpr int kSatChunk = 64;             // base samples of a chunk
constexpr int kSatRun = 4;                // consecutive base samples of a lane: 16 lanes a row
constexpr int kSatOutPitch = 68;          // floats: rows on 16-byte boundaries, 4 off a multiple of 64
constexpr int kSatMaxBufsize = 1 << 20;
constexpr int kSatMaxUp = 64, kSatMaxDown = 256;
static_assert(kSatTracks * (kSatChunk / kSatRun) == 256, "a lane per run of every row");

// Input tile row: [Ku-1 carried][64 of the chunk].  Odd, so the 16-byte pieces of two rows start on different banks.
__host__ __device__ constexpr int sat_pitch_in(int Ku) { return Ku - 1 + kSatChunk; }
// Shaped tile row: [Kd-1 carried][64 R of the chunk]; Kd is a multiple of 4, so the sample in front of R-aligned
// groups sits at a multiple of R.  The pitch is 4 floats off a multiple of 64 (64 R is one).
__host__ __device__ constexpr int sat_pitch_os(int R, int Kd) { return kSatChunk * R + ((Kd - 1 + 59) / 64) * 64 + 4; }

constexpr size_t sat_lds_bytes(int R, int Ku, int Kd) {
    return (size_t)kSatTracks * (sat_pitch_os(R, Kd) + kSatOutPitch + sat_pitch_in(Ku)) * sizeof(float);
}
static_assert(sat_lds_bytes(8, kSatMaxUp, kSatMaxDown) <= 64 * 1024, "the tiles fit the default LDS limit");
static_assert(sat_pitch_os(8, 256) >= 255 + 512 && sat_pitch_os(2, 4) >= 3 + 128 && sat_pitch_os(4, 128) == 388, "");

template <int CURVE>
__device__ __forceinline__ float sat_curve(float x) {
    if constexpr (CURVE == GAB_SAT_RATIONAL) {
        return __fdiv_rn(x, __fadd_rn(1.0f, fabsf(x)));
    } else {
        const float c = x > 1.0f ? 1.0f : (x < -1.0f ? -1.0f : x);    // a NaN fails both and passes
        if constexpr (CURVE == GAB_SAT_HARD) return c;
        const float c2 = __fmul_rn(c, c);
        return __fmul_rn(c, fmaf(-0.5f, c2, 1.5f));
    }
}

__device__ __forceinline__ float sat_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }

// A track's row, and S(bias).
struct SatRow {
    float drive, bias, level, sb;
};

template <int CURVE>
__device__ __forceinline__ SatRow sat_row(const float* __restrict__ tab, size_t track) {
    SatRow r;
    r.drive = tab[track * GAB_SAT_FIELDS];
    r.bias = tab[track * GAB_SAT_FIELDS + 1];
    r.level = tab[track * GAB_SAT_FIELDS + 2];
    r.sb = sat_curve<CURVE>(r.bias);
    return r;
}

template <int CURVE>
__device__ __forceinline__ SatRow sat_row_ramped(const SatRow& c, const SatRow& t, float rr) {
    SatRow r;
    r.drive = sat_ramp(c.drive, t.drive, rr);
    r.bias = sat_ramp(c.bias, t.bias, rr);
    r.level = sat_ramp(c.level, t.level, rr);
    r.sb = sat_curve<CURVE>(r.bias);
    return r;
}

template <int CURVE>
__device__ __forceinline__ float sat_shape(float u, const SatRow& r) {
    return __fmul_rn(r.level, __fsub_rn(sat_curve<CURVE>(fmaf(r.drive, u, r.bias)), r.sb));
}

// Tap j of every phase on the lane's four base samples: xk = w[i0 + k - j].  up: [R][Ku], j wave-uniform.
template <int R, bool FIRST>
__device__ __forceinline__ void sat_up_step(float (&acc)[kSatRun][R], const float* __restrict__ up, int Ku, int j,
                                            float x0, float x1, float x2, float x3) {
#pragma unroll
    for (int p = 0; p < R; ++p) {
        const float h = up[p * Ku + j];
        if constexpr (FIRST) {
            acc[0][p] = __fmul_rn(h, x0); acc[1][p] = __fmul_rn(h, x1);
            acc[2][p] = __fmul_rn(h, x2); acc[3][p] = __fmul_rn(h, x3);
        } else {
            acc[0][p] = fmaf(h, x0, acc[0][p]); acc[1][p] = fmaf(h, x1, acc[1][p]);
            acc[2][p] = fmaf(h, x2, acc[2][p]); acc[3][p] = fmaf(h, x3, acc[3][p]);
        }
    }
}

// R shaped values from an R-aligned column of the lane's row into group G of the window.
template <int R, int G>
__device__ __forceinline__ void sat_load_group(float (&reg)[4 * R], const float* src) {
    if constexpr (R == 2) {
        const float2 v = *reinterpret_cast<const float2*>(src);
        reg[G * R] = v.x; reg[G * R + 1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < R / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
            reg[G * R + 4 * q] = v.x; reg[G * R + 4 * q + 1] = v.y;
            reg[G * R + 4 * q + 2] = v.z; reg[G * R + 4 * q + 3] = v.w;
        }
    }
}

// Taps jb .. jb + R - 1 of the lane's four outputs m0 + k.  With base = m0 R - jb, the window's word i is v[base - R + 1
// + i], output k takes word k R - r + R - 1 at tap jb + r.  The window is four groups of R words; from one block to the
// next the groups move up by one and the lowest is new, so group g lives in registers ((g + ROT) & 3) R .., ROT one less
// for every block: nothing is copied.  src: the column of v[base - R + 1], g: the taps at jb (wave-uniform).
template <int R, int ROT, bool FIRST>
__device__ __forceinline__ void sat_down_block(float (&reg)[4 * R], float (&acc)[kSatRun], const float* __restrict__ g,
                                               const float* src) {
    sat_load_group<R, (ROT & 3)>(reg, src);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float h = g[r];
#pragma unroll
        for (int k = 0; k < kSatRun; ++k) {
            const int i = k * R - r + R - 1;
            const float v = reg[(((i / R) + ROT) & 3) * R + i % R];
            acc[k] = (FIRST && r == 0) ? __fmul_rn(h, v) : fmaf(h, v, acc[k]);
        }
    }
}

// Grid: x = group of 16 tracks.  in: [n][T][B], only read; out: [n][T][B], apart from in.  hist_in: [T][Ku-1], hist_os:
// [T][Kd-1].  up: [R][Ku], down: [Kd].  cur, tgt: [T][3]; ramp: [B].  vec: both blocks 16-byte aligned and B a multiple
// of 4.  RAMP: the launch's first buffer runs the ramp from cur to tgt; every other buffer takes tgt.
template <int R, int CURVE, bool RAMP>
__global__ __launch_bounds__(256) void sat_fused_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       float* __restrict__ hist_in, float* __restrict__ hist_os,
                                                       const float* __restrict__ up, const float* __restrict__ down,
                                                       const float* __restrict__ cur, const float* __restrict__ tgt,
                                                       const float* __restrict__ ramp, int T, int B, int Ku, int Kd,
                                                       int n_buffers, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int PA = sat_pitch_in(Ku), PB = sat_pitch_os(R, Kd);
    float* tb = lds;                                    // the shaped tile
    float* to = tb + kSatTracks * PB;                   // the outputs' tile
    float* ta = to + kSatTracks * kSatOutPitch;         // the input tile
    const int tid = threadIdx.x;
    const int lrow = tid >> 4, lq = tid & 15;           // moving data: 16 lanes a row
    const int row = tid & 15, run = tid >> 4;           // arithmetic: 16 rows side by side
    const int t0 = blockIdx.x * kSatTracks;
    const int nt = T - t0 < kSatTracks ? T - t0 : kSatTracks;
    const int HA = Ku - 1, HB = Kd - 1;

    // the histories into the front of the rows; a row below the last track holds zeros
#pragma unroll
    for (int i = 0; i < kSatMaxUp / 16; ++i) {
        const int c = lq + 16 * i;
        if (c < HA) ta[lrow * PA + c] = lrow < nt ? hist_in[(size_t)(t0 + lrow) * HA + c] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < kSatMaxDown / 16; ++i) {
        const int c = lq + 16 * i;
        if (c < HB) tb[lrow * PB + c] = lrow < nt ? hist_os[(size_t)(t0 + lrow) * HB + c] : 0.0f;
    }
    const size_t track = (size_t)t0 + (row < nt ? row : nt - 1);
    const SatRow rt = sat_row<CURVE>(tgt, track);
    [[maybe_unused]] SatRow rc = rt;
    if constexpr (RAMP) rc = sat_row<CURVE>(cur, track);

    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x0 = in + ((size_t)nb * T + t0) * B;
        float* y0 = out + ((size_t)nb * T + t0) * B;
        const bool ramping = RAMP && nb == 0;
        for (int s0 = 0; s0 < B; s0 += kSatChunk) {
            const int len = B - s0 < kSatChunk ? B - s0 : kSatChunk;
            // ---- 1. the chunk into the input tile, zeros behind the buffer's end and below the last track ----
            {
                const int c = 4 * lq;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (lrow < nt && c < len) {
                    const float* src = x0 + (size_t)lrow * B + s0 + c;
                    if (vec) {                                           // len is a multiple of 4: c < len covers c + 3
                        v = *reinterpret_cast<const float4*>(src);
                    } else {
                        v.x = src[0];
                        if (c + 1 < len) v.y = src[1];
                        if (c + 2 < len) v.z = src[2];
                        if (c + 3 < len) v.w = src[3];
                    }
                }
                float* dst = ta + lrow * PA + HA + c;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
            __syncthreads();
            // ---- 2. up by R and the curve: base samples 4 run .. 4 run + 3 of this lane's row ----
            {
                const float* w = ta + row * PA + HA + kSatRun * run;     // w[k - j]: sample 4 run + k - j of the chunk
                float acc[kSatRun][R];
                float a = w[0], b = w[1], c = w[2], d = w[3];
                sat_up_step<R, true>(acc, up, Ku, 0, a, b, c, d);
                int j = 1;
                for (; j + 3 < Ku; j += 4) {                             // the window turns through four registers
                    d = w[-j];     sat_up_step<R, false>(acc, up, Ku, j, d, a, b, c);
                    c = w[-j - 1]; sat_up_step<R, false>(acc, up, Ku, j + 1, c, d, a, b);
                    b = w[-j - 2]; sat_up_step<R, false>(acc, up, Ku, j + 2, b, c, d, a);
                    a = w[-j - 3]; sat_up_step<R, false>(acc, up, Ku, j + 3, a, b, c, d);
                }
                for (; j < Ku; ++j) {
                    d = c; c = b; b = a; a = w[-j];
                    sat_up_step<R, false>(acc, up, Ku, j, a, b, c, d);
                }
                float* dst = tb + row * PB + HB + kSatRun * run * R;
#pragma unroll
                for (int k = 0; k < kSatRun; ++k) {
                    SatRow r = rt;
                    if (ramping) {                                       // uniform
                        const int s = s0 + kSatRun * run + k;            // behind the buffer's end: never stored
                        r = sat_row_ramped<CURVE>(rc, rt, ramp[s < B ? s : B - 1]);
                    }
#pragma unroll
                    for (int p = 0; p < R; ++p) dst[k * R + p] = sat_shape<CURVE>(acc[k][p], r);
                }
            }
            __syncthreads();
            // ---- 3. down by R: base outputs 4 run .. 4 run + 3; the tails of both tiles ----
            float keep_a[kSatMaxUp / 16], keep_b[kSatMaxDown / 16];
            {
                const float* v = tb + row * PB + Kd + kSatRun * run * R;  // the column behind v[m0 R], R-aligned
                float reg[4 * R], acc[kSatRun];
                sat_load_group<R, 1>(reg, v);
                sat_load_group<R, 2>(reg, v + R);
                sat_load_group<R, 3>(reg, v + 2 * R);
                sat_down_block<R, 0, true>(reg, acc, down, v - R);
                sat_down_block<R, 3, false>(reg, acc, down + R, v - 2 * R);
                int jb = 2 * R;
                for (; jb + 4 * R <= Kd; jb += 4 * R) {
                    sat_down_block<R, 2, false>(reg, acc, down + jb, v - jb - R);
                    sat_down_block<R, 1, false>(reg, acc, down + jb + R, v - jb - 2 * R);
                    sat_down_block<R, 0, false>(reg, acc, down + jb + 2 * R, v - jb - 3 * R);
                    sat_down_block<R, 3, false>(reg, acc, down + jb + 3 * R, v - jb - 4 * R);
                }
                if (jb < Kd) {
                    sat_down_block<R, 2, false>(reg, acc, down + jb, v - jb - R);
                    sat_down_block<R, 1, false>(reg, acc, down + jb + R, v - jb - 2 * R);
                }
                *reinterpret_cast<float4*>(to + row * kSatOutPitch + kSatRun * run) =
                    make_float4(acc[0], acc[1], acc[2], acc[3]);
#pragma unroll
                for (int i = 0; i < kSatMaxUp / 16; ++i) {
                    const int c = lq + 16 * i;
                    keep_a[i] = c < HA ? ta[lrow * PA + len + c] : 0.0f;
                }
#pragma unroll
                for (int i = 0; i < kSatMaxDown / 16; ++i) {
                    const int c = lq + 16 * i;
                    keep_b[i] = c < HB ? tb[lrow * PB + R * len + c] : 0.0f;
                }
            }
            __syncthreads();
            // ---- 4. the tails to the front of the rows; the outputs leave ----
#pragma unroll
            for (int i = 0; i < kSatMaxUp / 16; ++i) {
                const int c = lq + 16 * i;
                if (c < HA) ta[lrow * PA + c] = keep_a[i];
            }
#pragma unroll
            for (int i = 0; i < kSatMaxDown / 16; ++i) {
                const int c = lq + 16 * i;
                if (c < HB) tb[lrow * PB + c] = keep_b[i];
            }
            {
                const int c = 4 * lq;
                if (lrow < nt && c < len) {
                    const float4 o = *reinterpret_cast<const float4*>(to + lrow * kSatOutPitch + c);
                    float* dst = y0 + (size_t)lrow * B + s0 + c;
                    if (vec) {
                        *reinterpret_cast<float4*>(dst) = o;
                    } else {
                        dst[0] = o.x;
                        if (c + 1 < len) dst[1] = o.y;
                        if (c + 2 < len) dst[2] = o.z;
                        if (c + 3 < len) dst[3] = o.w;
                    }
                }
            }
            // (the next chunk's step 1 writes the input tile behind its history, and its barrier orders step 4's words)
        }
    }
    __syncthreads();
    if (lrow < nt) {
#pragma unroll
        for (int i = 0; i < kSatMaxUp / 16; ++i) {
            const int c = lq + 16 * i;
            if (c < HA) hist_in[(size_t)(t0 + lrow) * HA + c] = ta[lrow * PA + c];
        }
#pragma unroll
        for (int i = 0; i < kSatMaxDown / 16; ++i) {
            const int c = lq + 16 * i;
            if (c < HB) hist_os[(size_t)(t0 + lrow) * HB + c] = tb[lrow * PB + c];
        }
    }
}

// The curve alone.  in / out: [n][T][RB] (out may be in: a lane reads its elements before it writes them), RB = R B, R =
// 2^log2r.  A lane takes W = 4 (VEC: both blocks 16-byte aligned, RB a multiple of 4) or 1 consecutive elements of a
// row; per_row = ceil(RB / W) lanes a row, `total` lanes in all, walked with the grid's stride.
template <int CURVE, bool RAMP, bool VEC>
__global__ __launch_bounds__(256) void sat_apply_kernel(const float* in, float* out, const float* __restrict__ cur,
                                                       const float* __restrict__ tgt, const float* __restrict__ ramp,
                                                       int T, int RB, int log2r, size_t per_row, size_t total) {
    constexpr int W = VEC ? 4 : 1;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / per_row;                                   // the row: buffer * T + track
        const int col = (int)(i - r * per_row) * W;
        const size_t track = r % (size_t)T;
        const bool ramping = RAMP && r < (size_t)T;                     // the first buffer
        const SatRow rt = sat_row<CURVE>(tgt, track);
        [[maybe_unused]] SatRow rc = rt;
        if constexpr (RAMP) rc = sat_row<CURVE>(cur, track);
        const size_t at = r * (size_t)RB + (size_t)col;
        float x[W], y[W];
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(in + at);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = in[at];
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            SatRow row = rt;
            if (ramping) row = sat_row_ramped<CURVE>(rc, rt, ramp[(col + e) >> log2r]);
            y[e] = sat_shape<CURVE>(x[e], row);
        }
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(out + at) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            out[at] = y[0];
        }
    }
}

const char* const kSatFields[GAB_SAT_FIELDS] = {"drive", "bias", "level"};

// src: [n_rows][3]
struct SatParamRule {
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int first_track) const {
        return row_refusal(i, GAB_SAT_FIELDS, first_track, kSatFields[i % GAB_SAT_FIELDS], "must be finite");
    }
};

// src: [phases][taps]; which: 0 the up table, 1 the down table (for the text only)
struct SatTapsRule {
    unsigned taps;
    int which;
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int) const {
        return std::string(which ? "down" : "up") + " table phase " + std::to_string(i / taps) + " tap " +
               std::to_string(i % taps) + " is not finite; the plan keeps its taps";
    }
};

}  // namespace
}  // namespace gab

struct gab_sat_plan {
    int tracks = 0, bufsize = 0, R = 0, curve = 0, Ku = 0, Kd = 0;
    gab::RampedTable params;                   // current, target: [T][3]; the ramp over the B base samples
    gab::DeviceBuf<float> up, down;            // [R][Ku], [Kd]
    gab::DeviceBuf<float> hist_in, hist_os;    // [T][Ku-1], [T][Kd-1], oldest first
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

void sat_clear(gab_sat_plan* p, hipStream_t s) {
    if (p->R == 1) return;
    GAB_HIP_CHECK(hipMemsetAsync(p->hist_in.get(), 0, p->hist_in.size() * sizeof(float), s));
    GAB_HIP_CHECK(hipMemsetAsync(p->hist_os.get(), 0, p->hist_os.size() * sizeof(float), s));
}

template <int CURVE>
void sat_apply_launch(gab_sat_plan* p, const float* d_in, float* d_out, int n_buffers, bool ramp, hipStream_t s) {
    const int RB = p->R * p->bufsize;
    const bool vec = all_aligned16({d_in, d_out}) && RB % 4 == 0;
    const size_t per_row = vec ? (size_t)RB / 4 : (size_t)RB;
    const size_t total = (size_t)n_buffers * p->tracks * per_row;
    const size_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < ((size_t)1 << 22) ? blocks : ((size_t)1 << 22)));
    int log2r = 0;
    while ((1 << log2r) < p->R) ++log2r;
#define GAB_SAT_APPLY(RR, VV)                                                                                        \
    sat_apply_kernel<CURVE, RR, VV><<<grid, 256, 0, s>>>(d_in, d_out, p->params.current.get(), p->params.target.get(), \
                                                         p->params.ramp.get(), p->tracks, RB, log2r, per_row, total)
    if (vec) {
        if (ramp) GAB_SAT_APPLY(true, true); else GAB_SAT_APPLY(false, true);
    } else {
        if (ramp) GAB_SAT_APPLY(true, false); else GAB_SAT_APPLY(false, false);
    }
#undef GAB_SAT_APPLY
}

// The curve on n blocks of [T][R B]; then, if a ramp ran through the first of them, current := target.
int sat_apply(gab_sat_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    const size_t block = (size_t)p->tracks * p->bufsize * p->R;
    if (d_out != d_in && overlaps(d_in, d_out, (size_t)n_buffers * block))
        return refuse(who, "d_out may be d_in itself; any other overlap is refused");
    const bool ramp = p->params.pending;
    switch (p->curve) {
        case GAB_SAT_HARD: sat_apply_launch<GAB_SAT_HARD>(p, d_in, d_out, n_buffers, ramp, s); break;
        case GAB_SAT_CUBIC: sat_apply_launch<GAB_SAT_CUBIC>(p, d_in, d_out, n_buffers, ramp, s); break;
        default: sat_apply_launch<GAB_SAT_RATIONAL>(p, d_in, d_out, n_buffers, ramp, s); break;
    }
    if (int rc = launch_status("sat_apply_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

template <int R, int CURVE>
void sat_fused_launch(gab_sat_plan* p, const float* d_in, float* d_out, int n_buffers, bool ramp, hipStream_t s) {
    const dim3 grid((unsigned)((p->tracks + kSatTracks - 1) / kSatTracks));
    const int vec = all_aligned16({d_in, d_out}) && p->bufsize % 4 == 0 ? 1 : 0;
    const size_t lds = sat_lds_bytes(R, p->Ku, p->Kd);
#define GAB_SAT_FUSED(RR)                                                                                            \
    sat_fused_kernel<R, CURVE, RR><<<grid, 256, lds, s>>>(d_in, d_out, p->hist_in.get(), p->hist_os.get(), p->up.get(), \
                                                          p->down.get(), p->params.current.get(),                   \
                                                          p->params.target.get(), p->params.ramp.get(), p->tracks,   \
                                                          p->bufsize, p->Ku, p->Kd, n_buffers, vec)
    if (ramp) GAB_SAT_FUSED(true); else GAB_SAT_FUSED(false);
#undef GAB_SAT_FUSED
}

template <int R>
void sat_fused_curve(gab_sat_plan* p, const float* d_in, float* d_out, int n_buffers, bool ramp, hipStream_t s) {
    switch (p->curve) {
        case GAB_SAT_HARD: sat_fused_launch<R, GAB_SAT_HARD>(p, d_in, d_out, n_buffers, ramp, s); break;
        case GAB_SAT_CUBIC: sat_fused_launch<R, GAB_SAT_CUBIC>(p, d_in, d_out, n_buffers, ramp, s); break;
        default: sat_fused_launch<R, GAB_SAT_RATIONAL>(p, d_in, d_out, n_buffers, ramp, s); break;
    }
}

// n buffers in one launch.  Nothing is allocated and nothing waits here.
int sat_process(gab_sat_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    const size_t block = (size_t)p->tracks * p->bufsize;
    if (overlaps(d_in, d_out, (size_t)n_buffers * block))
        return refuse(who, "d_out may not overlap d_in: the output is delayed");
    if (p->R == 1) return sat_apply(p, d_in, d_out, n_buffers, s, who);
    const bool ramp = p->params.pending;
    switch (p->R) {
        case 2: sat_fused_curve<2>(p, d_in, d_out, n_buffers, ramp, s); break;
        case 4: sat_fused_curve<4>(p, d_in, d_out, n_buffers, ramp, s); break;
        default: sat_fused_curve<8>(p, d_in, d_out, n_buffers, ramp, s); break;
    }
    if (int rc = launch_status("sat_fused_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int sat_set_range(gab_sat_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                  hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_SAT_FIELDS;
    return check_then(p->flag, s, who, d_params, n, SatParamRule{}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * GAB_SAT_FIELDS, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_sat_create(gab_sat_plan** out, int tracks, int bufsize, int oversample, int curve, int up_taps, int down_taps) {
    return gab::create_entry("gab_sat_create", out, tracks, bufsize, [&] {
        const int R = oversample;
        if (bufsize > gab::kSatMaxBufsize) return gab::bad_arg("gab_sat_create: bufsize must be <= 2^20");
        if (R != 1 && R != 2 && R != 4 && R != 8) return gab::bad_arg("gab_sat_create: oversample must be 1, 2, 4 or 8");
        if (curve < GAB_SAT_HARD || curve > GAB_SAT_RATIONAL)
            return gab::bad_arg("gab_sat_create: curve must be 0 (hard), 1 (cubic) or 2 (rational)");
        if (R == 1) {
            if (up_taps != 0 || down_taps != 0)
                return gab::bad_arg("gab_sat_create: up_taps and down_taps must be 0 at oversample 1");
            return GAB_OK;
        }
        if (up_taps < 4 || up_taps > gab::kSatMaxUp || up_taps % 2 != 0)
            return gab::bad_arg("gab_sat_create: up_taps must be even and 4..64");
        if (down_taps < 4 || down_taps > gab::kSatMaxDown || down_taps % (2 * R) != 0)
            return gab::bad_arg("gab_sat_create: down_taps must be 4..256 and a multiple of 2 * oversample");
        return GAB_OK;
    }, [&](gab_sat_plan& p) {
        p.R = oversample; p.curve = curve; p.Ku = up_taps; p.Kd = down_taps;
        p.params.create((size_t)tracks * GAB_SAT_FIELDS, bufsize);
        p.params.fill({1.0f, 0.0f, 1.0f}, tracks);
        p.flag.alloc(1);
        if (p.R > 1) {
            const std::vector<float> hu = gab::resample_design(p.R, 1, p.Ku), hd = gab::resample_design(1, p.R, p.Kd);
            p.up.alloc(hu.size());
            p.down.alloc(hd.size());
            p.hist_in.alloc((size_t)tracks * (p.Ku - 1));
            p.hist_os.alloc((size_t)tracks * (p.Kd - 1));
            GAB_HIP_CHECK(hipMemcpy(p.up.get(), hu.data(), hu.size() * sizeof(float), hipMemcpyHostToDevice));
            GAB_HIP_CHECK(hipMemcpy(p.down.get(), hd.data(), hd.size() * sizeof(float), hipMemcpyHostToDevice));
            gab::sat_clear(&p, nullptr);
        }
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_sat_destroy(gab_sat_plan* plan) { return gab::destroy_plan(plan, "gab_sat_destroy: null pointer"); }

int gab_sat_info(gab_sat_plan* plan, int* oversample, int* curve, int* up_taps, int* down_taps, int* latency) {
    return gab::entry("gab_sat_info", {plan, oversample, curve, up_taps, down_taps, latency}, [&] {
        *oversample = plan->R; *curve = plan->curve; *up_taps = plan->Ku; *down_taps = plan->Kd;
        *latency = plan->R == 1 ? 0 : plan->Ku / 2 + plan->Kd / (2 * plan->R);
        return GAB_OK;
    });
}

int gab_sat_set_params(gab_sat_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_sat_set_params", gab::sat_set_range, plan, d_params, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_sat_set_params_tracks(gab_sat_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream) {
    return gab::set_entry("gab_sat_set_params_tracks", gab::sat_set_range, plan, d_params, false, first_track, n_tracks, ramp,
                          gab::as_stream(stream));
}

// check both, then commit both (gab_plan.hpp): a refused value in either table leaves both as they were
int gab_sat_set_taps(gab_sat_plan* plan, const float* d_up, const float* d_down, gab_stream_t stream) {
    return gab::entry("gab_sat_set_taps", {plan, d_up, d_down}, [&]() -> int {
        const char* who = "gab_sat_set_taps";
        if (plan->R == 1) return gab::refuse(who, "a plan at oversample 1 has no taps");
        hipStream_t s = gab::as_stream(stream);
        const size_t nu = (size_t)plan->R * plan->Ku, nd = (size_t)plan->Kd;
        if (int rc = gab::check_then(plan->flag, s, who, d_up, nu, gab::SatTapsRule{(unsigned)plan->Ku, 0}, 0, [] {}))
            return rc;
        return gab::check_then(plan->flag, s, who, d_down, nd, gab::SatTapsRule{(unsigned)plan->Kd, 1}, 0, [&] {
            GAB_HIP_CHECK(hipMemcpyAsync(plan->up.get(), d_up, nu * sizeof(float), hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipMemcpyAsync(plan->down.get(), d_down, nd * sizeof(float), hipMemcpyDeviceToDevice, s));
            GAB_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int gab_sat_reset(gab_sat_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_sat_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        gab::sat_clear(plan, s);
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_sat_process(gab_sat_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_sat_process", {plan, d_in, d_out}, [&] {
        return gab::sat_process(plan, d_in, d_out, 1, gab::as_stream(stream), "gab_sat_process");
    });
}

int gab_sat_process_batch(gab_sat_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_sat_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::sat_process(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_sat_process_batch");
    });
}

int gab_sat_apply(gab_sat_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_sat_apply", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::sat_apply(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_sat_apply");
    });
}

int gab_sat_params(gab_sat_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_sat_params", plan, &gab_sat_plan::params, d_current, d_target, n_floats);
}

int gab_sat_state(gab_sat_plan* plan, float** d_hist_in, float** d_hist_os, float** d_up, float** d_down) {
    return gab::entry("gab_sat_state", {plan, d_hist_in, d_hist_os, d_up, d_down}, [&] {
        *d_hist_in = plan->hist_in.get();
        *d_hist_os = plan->hist_os.get();
        *d_up = plan->up.get();
        *d_down = plan->down.get();
        return GAB_OK;
    });
}

}  // extern "C"
