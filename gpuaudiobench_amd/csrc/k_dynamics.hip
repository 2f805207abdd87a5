// k_dynamics.hip — the dynamics plan: a compressor / limiter per track with a carried smoothed gain, eight parameters
// {thr, slope, knee, kq, att, rel, makeup, range} that can be ramped over one buffer, linked detectors and a side chain
// (include/gab_c_api.h, gab_dyn_*).  No counterpart in the reference.
//
//   dyn_kernel<VEC, KEY, RAMP>  a workgroup is one wave and owns 64 tracks for the whole launch, every buffer of a
//                               batch included.  It walks the buffer in chunks of 64 samples:
//                                 1. pointwise, a lane per 16 rows x 4 samples: the chunk from memory into registers,
//                                    the link group's detector maximum across the lane's rows (and across lanes for
//                                    groups of 32 and 64), the level L, the gain computer's g into an LDS tile;
//                                 2. serial, a lane per track: the row of g in order, the smoothed gain s written over
//                                    it, the buffer's smallest s kept for the gain-reduction meter;
//                                 3. pointwise again: 2^s by the polynomial, the product with the chunk held in
//                                    registers, the store.
//                               The block is read once and written once; nothing leaves the wave, so there is no
//                               workgroup barrier.  A link group is at most 64 tracks and tracks % link == 0, so a
//                               group never straddles two waves.
//   DynRule                     refuses a parameter row outside the contract, naming the first (gab_plan.hpp's check
//                               kernel).
//
// log2 and exp2 are the two pinned polynomials below (tools/dyn_poly.py fits and measures them); no library
// transcendental is called.  The sequence of roundings per sample is the header's; the cut decides only where a value
// is held, so every launch form, alignment and track count gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kDynTracks = 64;            // tracks of a workgroup: the lanes of the serial phase
constexpr int kDynChunk = 64;             // samples of a chunk
constexpr int kDynPitch = 68;             // row pitch in floats: 16-byte aligned rows, conflict-free b128 access (kEqPitch)
constexpr int kDynRows = 16;              // rows of a lane in the pointwise phases: rows 16 (lane / 16) + k, 4 samples each
constexpr int kDynMaxLink = 64;

// log2(1 + t) = t r(t) on [0, 1): r's coefficients c0..c6.  exp2(f) = q(f) on [0, 1): d0..d6, d0 = 1.
// tools/dyn_poly.py: interpolation at Chebyshev nodes in float64, each coefficient rounded once.
#define GAB_DYN_C0 0x1.715454p+0f
#define GAB_DYN_C1 -0x1.7139ccp-1f
#define GAB_DYN_C2 0x1.e8f4cep-2f
#define GAB_DYN_C3 -0x1.5a7f8ep-2f
#define GAB_DYN_C4 0x1.b627dcp-3f
#define GAB_DYN_C5 -0x1.839766p-4f
#define GAB_DYN_C6 0x1.47f3eap-6f
#define GAB_DYN_D0 0x1.0p+0f
#define GAB_DYN_D1 0x1.62e43p-1f
#define GAB_DYN_D2 0x1.ebfc3ep-3f
#define GAB_DYN_D3 0x1.c69f98p-5f
#define GAB_DYN_D4 0x1.3c487cp-7f
#define GAB_DYN_D5 0x1.4cb7bp-10f
#define GAB_DYN_D6 0x1.b49554p-13f
const float kDynLog2[7] = {GAB_DYN_C0, GAB_DYN_C1, GAB_DYN_C2, GAB_DYN_C3, GAB_DYN_C4, GAB_DYN_C5, GAB_DYN_C6};
const float kDynExp2[7] = {GAB_DYN_D0, GAB_DYN_D1, GAB_DYN_D2, GAB_DYN_D3, GAB_DYN_D4, GAB_DYN_D5, GAB_DYN_D6};

// A hand-off through LDS inside the wave (k_delay.hip's): words that some lanes wrote or read are touched by other
// lanes next.
__device__ __forceinline__ void dyn_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float dyn_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }

// The detector's level: log2 of fmaxf(a, 2^-96), the exponent from the bits, the mantissa through the polynomial.
__device__ __forceinline__ float dyn_level(float a) {
    const unsigned u = __float_as_uint(fmaxf(a, 0x1p-96f));
    const int e = (int)(u >> 23) - 127;
    const float m = __uint_as_float((u & 0x7fffffu) | 0x3f800000u);
    const float t = __fsub_rn(m, 1.0f);                              // exact
    float r = GAB_DYN_C6;
    r = fmaf(r, t, GAB_DYN_C5);
    r = fmaf(r, t, GAB_DYN_C4);
    r = fmaf(r, t, GAB_DYN_C3);
    r = fmaf(r, t, GAB_DYN_C2);
    r = fmaf(r, t, GAB_DYN_C1);
    r = fmaf(r, t, GAB_DYN_C0);
    return __fadd_rn((float)e, __fmul_rn(t, r));
}

// The gain computer: the static curve's reduction at level L, in log2 units, <= 0.
__device__ __forceinline__ float dyn_computer(float L, float thr, float slope, float knee, float kq, float range) {
    const float over = __fsub_rn(L, thr);
    const float ok = __fadd_rn(over, knee);
    const float soft = __fmul_rn(__fmul_rn(ok, ok), kq);
    const float c = over <= -knee ? 0.0f : (over >= knee ? over : soft);
    return fmaxf(__fmul_rn(slope, c), range);
}

// 2^s for the smoothed gain s, clamped to [-126, 0]: the fraction through the polynomial, the integer part as an exponent.
__device__ __forceinline__ float dyn_exp2(float s) {
    const float sc = fminf(fmaxf(s, -126.0f), 0.0f);
    const float nf = floorf(sc);
    const float f = __fsub_rn(sc, nf);                               // exact
    float q = GAB_DYN_D6;
    q = fmaf(q, f, GAB_DYN_D5);
    q = fmaf(q, f, GAB_DYN_D4);
    q = fmaf(q, f, GAB_DYN_D3);
    q = fmaf(q, f, GAB_DYN_D2);
    q = fmaf(q, f, GAB_DYN_D1);
    q = fmaf(q, f, GAB_DYN_D0);
    return __fmul_rn(q, __uint_as_float((unsigned)((int)nf + 127) << 23));
}

// What a wave carries through a launch.
struct DynWave {
    float* tile;                // [64][kDynPitch]: g, then s
    const float* ptab;          // [64][8]: the target rows
    const float* pcur;          // [64][8]: the current rows (RAMP)
    float* rl;                  // [64]: the chunk's ramp values (RAMP)
    int lane, nt, link;
    float s;                    // lane = track: the smoothed gain
    float t_att, t_rel, c_att, c_rel;
};

// One buffer.  x, k, y: the rows of this wave's first track in that buffer; ramp: the table [B].
template <bool VEC, bool KEY, bool RAMPING>
__device__ __forceinline__ float dyn_buffer(DynWave& w, const float* x, const float* k, float* y,
                                            const float* __restrict__ ramp, int B) {
    const int lane = w.lane;
    const int r0 = (lane >> 4) * kDynRows, q = (lane & 15) * 4;
    float* tile = w.tile;
    float grmin = __builtin_inff();
    for (int s0 = 0; s0 < B; s0 += kDynChunk) {
        const int len = B - s0 < kDynChunk ? B - s0 : kDynChunk;
        if constexpr (RAMPING) w.rl[lane] = lane < len ? ramp[s0 + lane] : 1.0f;
        // ---- 1. the chunk into registers ----
        // Every load is unconditional, so that all of them are in flight before the first is used: a row below the last
        // track reads the last track's, a sample behind the buffer's end the chunk's first.  Such a value is never
        // stored, never enters the recurrence, and a link group never mixes rows of the two kinds.
        float xv[kDynRows][4], a[kDynRows][4];
        const int qc = q < len ? q : 0;                               // VEC: len is a multiple of 4, so q < len covers q + 3
#pragma unroll
        for (int i = 0; i < kDynRows; ++i) {
            const int r = r0 + i;
            const size_t row_at = (size_t)(r < w.nt ? r : w.nt - 1) * B + s0;
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(x + row_at + qc);
                xv[i][0] = v.x; xv[i][1] = v.y; xv[i][2] = v.z; xv[i][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[i][j] = x[row_at + (q + j < len ? q + j : 0)];
            }
        }
        if constexpr (KEY) {
#pragma unroll
            for (int i = 0; i < kDynRows; ++i) {
                const int r = r0 + i;
                const size_t row_at = (size_t)(r < w.nt ? r : w.nt - 1) * B + s0;
                if constexpr (VEC) {
                    const float4 v = *reinterpret_cast<const float4*>(k + row_at + qc);
                    a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[i][j] = k[row_at + (q + j < len ? q + j : 0)];
                }
            }
        }
        // the detector: |key| from 0 (a NaN is ignored), the maximum over the link group's rows
#pragma unroll
        for (int i = 0; i < kDynRows; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] = fmaxf(0.0f, fabsf(KEY ? a[i][j] : xv[i][j]));
#pragma unroll
        for (int d = 1; d < kDynRows; d *= 2) {
            if (w.link > d) {                                        // wave-uniform
#pragma unroll
                for (int i = 0; i < kDynRows; ++i) {
                    if ((i & d) == 0) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float m = fmaxf(a[i][j], a[i | d][j]);
                            a[i][j] = m;
                            a[i | d][j] = m;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int d = kDynRows; d < kDynMaxLink; d *= 2) {            // rows 16 and 32 apart: lanes 16 and 32 apart
            if (w.link > d) {
#pragma unroll
                for (int i = 0; i < kDynRows; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[i][j] = fmaxf(a[i][j], __shfl_xor(a[i][j], d, 64));
            }
        }
        if constexpr (RAMPING) dyn_wave_order();                     // rl is written
        float rr[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if constexpr (RAMPING) {
            const float4 v = *reinterpret_cast<const float4*>(w.rl + q);
            rr[0] = v.x; rr[1] = v.y; rr[2] = v.z; rr[3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < kDynRows; ++i) {
            const int r = r0 + i;
            const float4 t0 = *reinterpret_cast<const float4*>(w.ptab + r * GAB_DYN_FIELDS);
            const float t7 = w.ptab[r * GAB_DYN_FIELDS + 7];
            float g[4];
            if constexpr (RAMPING) {
                const float4 c0 = *reinterpret_cast<const float4*>(w.pcur + r * GAB_DYN_FIELDS);
                const float c7 = w.pcur[r * GAB_DYN_FIELDS + 7];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    g[j] = dyn_computer(dyn_level(a[i][j]), dyn_ramp(c0.x, t0.x, rr[j]), dyn_ramp(c0.y, t0.y, rr[j]),
                                        dyn_ramp(c0.z, t0.z, rr[j]), dyn_ramp(c0.w, t0.w, rr[j]), dyn_ramp(c7, t7, rr[j]));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = dyn_computer(dyn_level(a[i][j]), t0.x, t0.y, t0.z, t0.w, t7);
            }
            *reinterpret_cast<float4*>(tile + r * kDynPitch + q) = make_float4(g[0], g[1], g[2], g[3]);
        }
        dyn_wave_order();
        // ---- 2. the smoothing, a lane per track, in order ----
        {
            float4* row = reinterpret_cast<float4*>(tile + lane * kDynPitch);
            float s = w.s;
            const float d_att = __fsub_rn(w.t_att, w.c_att), d_rel = __fsub_rn(w.t_rel, w.c_rel);
            for (int i = 0; 4 * i < len; ++i) {
                float4 v = row[i];
                float gs[4] = {v.x, v.y, v.z, v.w};
                float rs[4] = {1.0f, 1.0f, 1.0f, 1.0f};
                if constexpr (RAMPING) {
                    const float4 rv = *reinterpret_cast<const float4*>(w.rl + 4 * i);
                    rs[0] = rv.x; rs[1] = rv.y; rs[2] = rv.z; rs[3] = rv.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * i + j < len) {                           // wave-uniform: the recurrence never runs on padding
                        const float att = RAMPING ? fmaf(d_att, rs[j], w.c_att) : w.t_att;
                        const float rel = RAMPING ? fmaf(d_rel, rs[j], w.c_rel) : w.t_rel;
                        const float g = gs[j];
                        const float al = g < s ? att : rel;
                        s = fmaf(al, __fsub_rn(s, g), g);
                        grmin = fminf(grmin, s);
                        gs[j] = s;
                    }
                }
                row[i] = make_float4(gs[0], gs[1], gs[2], gs[3]);
            }
            w.s = s;
        }
        dyn_wave_order();
        // ---- 3. the gain and the store ----
#pragma unroll
        for (int i = 0; i < kDynRows; ++i) {
            const int r = r0 + i;
            const float4 sv = *reinterpret_cast<const float4*>(tile + r * kDynPitch + q);
            const float ss[4] = {sv.x, sv.y, sv.z, sv.w};
            const float t6 = w.ptab[r * GAB_DYN_FIELDS + 6];
            float c6 = t6;
            if constexpr (RAMPING) c6 = w.pcur[r * GAB_DYN_FIELDS + 6];
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float makeup = RAMPING ? dyn_ramp(c6, t6, rr[j]) : t6;
                o[j] = __fmul_rn(xv[i][j], __fmul_rn(dyn_exp2(ss[j]), makeup));
            }
            const size_t at = (size_t)r * B + s0 + q;
            if constexpr (VEC) {
                if (r < w.nt && q < len) *reinterpret_cast<float4*>(y + at) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r < w.nt && q + j < len) y[at + j] = o[j];
            }
        }
        dyn_wave_order();                                            // the tile and rl are free for the next chunk
    }
    return grmin;
}

// Grid: x = group of 64 tracks, one wave.  in / key / out: [n][T][B]; out may be in (a chunk is read before it is
// written, by the same wave); key is only read.  gr: [n][T] or null.  smooth: [T].  VEC: all blocks 16-byte aligned and
// B a multiple of 4.  RAMP: the launch's first buffer runs the ramp from cur to tgt; every other buffer takes tgt.
template <bool VEC, bool KEY, bool RAMP>
__global__ __launch_bounds__(64) void dyn_kernel(const float* in, const float* key, float* out, float* gr,
                                                 float* __restrict__ smooth, const float* __restrict__ cur,
                                                 const float* __restrict__ tgt, const float* __restrict__ ramp, int T,
                                                 int B, int n_buffers, int link) {
    __shared__ __attribute__((aligned(16))) float tile[kDynTracks * kDynPitch];
    __shared__ __attribute__((aligned(16))) float ptab[kDynTracks * GAB_DYN_FIELDS];
    __shared__ __attribute__((aligned(16))) float pcur[RAMP ? kDynTracks * GAB_DYN_FIELDS : 4];
    __shared__ __attribute__((aligned(16))) float rl[RAMP ? kDynChunk : 4];
    const int lane = threadIdx.x;
    const int t0 = blockIdx.x * kDynTracks;
    DynWave w;
    w.tile = tile; w.ptab = ptab; w.pcur = pcur; w.rl = rl;
    w.lane = lane; w.link = link;
    w.nt = T - t0 < kDynTracks ? T - t0 : kDynTracks;
    const bool owner = lane < w.nt;
    const size_t track = (size_t)t0 + lane;
    // the rows of this wave's tracks, a lane per track; rows below the last track are zeros (their g is 0, unused)
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo, clo = lo, chi = lo;
    if (owner) {
        lo = *reinterpret_cast<const float4*>(tgt + track * GAB_DYN_FIELDS);
        hi = *reinterpret_cast<const float4*>(tgt + track * GAB_DYN_FIELDS + 4);
    }
    clo = lo; chi = hi;
    if constexpr (RAMP) {
        if (owner) {
            clo = *reinterpret_cast<const float4*>(cur + track * GAB_DYN_FIELDS);
            chi = *reinterpret_cast<const float4*>(cur + track * GAB_DYN_FIELDS + 4);
        }
        *reinterpret_cast<float4*>(pcur + lane * GAB_DYN_FIELDS) = clo;
        *reinterpret_cast<float4*>(pcur + lane * GAB_DYN_FIELDS + 4) = chi;
    }
    *reinterpret_cast<float4*>(ptab + lane * GAB_DYN_FIELDS) = lo;
    *reinterpret_cast<float4*>(ptab + lane * GAB_DYN_FIELDS + 4) = hi;
    w.t_att = hi.x; w.t_rel = hi.y; w.c_att = chi.x; w.c_rel = chi.y;
    w.s = owner ? smooth[track] : 0.0f;
    dyn_wave_order();

    const size_t block = (size_t)T * B;
    const float* x = in + (size_t)t0 * B;
    const float* k = KEY ? key + (size_t)t0 * B : nullptr;
    float* y = out + (size_t)t0 * B;
    int nb = 0;
    if constexpr (RAMP) {
        const float m = dyn_buffer<VEC, KEY, true>(w, x, k, y, ramp, B);
        if (gr && owner) gr[track] = m;
        nb = 1;
    }
    for (; nb < n_buffers; ++nb) {
        const float m = dyn_buffer<VEC, KEY, false>(w, x + nb * block, KEY ? k + nb * block : nullptr, y + nb * block,
                                                    ramp, B);
        if (gr && owner) gr[(size_t)nb * T + track] = m;
    }
    if (owner) smooth[track] = w.s;
}

const char* const kDynFields[GAB_DYN_FIELDS] = {"thr", "slope", "knee", "kq", "att", "rel", "makeup", "range"};
const char* const kDynRules[GAB_DYN_FIELDS] = {
    "must be finite and within [-128, 128]", "must be within [-1, 0]", "must be within [0, 64]",
    "must be finite and >= 0", "must be within [0, 1 - 2^-20]", "must be within [0, 1 - 2^-20]", "must be finite",
    "must be finite and <= 0"};

// src: [n_rows][8] (a NaN fails every comparison)
struct DynRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i & 7);
        bool bad = not_finite(__float_as_uint(v));
        if (field == 0) bad = bad || !(fabsf(v) <= 128.0f);
        if (field == 1) bad = bad || !(v >= -1.0f && v <= 0.0f);
        if (field == 2) bad = bad || !(v >= 0.0f && v <= 64.0f);
        if (field == 3) bad = bad || !(v >= 0.0f);
        if (field == 4 || field == 5) bad = bad || !(v >= 0.0f && v <= 0x1.ffffep-1f);   // 1 - 2^-20
        if (field == 7) bad = bad || !(v <= 0.0f);
        return bad;
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % GAB_DYN_FIELDS);
        return row_refusal(i, GAB_DYN_FIELDS, first_track, kDynFields[field], kDynRules[field]);
    }
};

}  // namespace
}  // namespace gab

struct gab_dyn_plan {
    int tracks = 0, bufsize = 0, link = 0;
    gab::RampedTable params;           // current, target: [T][8]
    gab::DeviceBuf<float> smooth;      // [T]: the smoothed gain, log2 units, <= 0
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch; then, if a ramp ran through the first of them, current := target.  Nothing is allocated and
// nothing waits here.
int dyn_process(gab_dyn_plan* p, const float* d_in, const float* d_key, float* d_out, float* d_gr, int n_buffers,
                hipStream_t s, const char* who) {
    if (d_key && overlaps(d_key, d_out, (size_t)n_buffers * p->tracks * p->bufsize))
        return refuse(who, "d_key may not overlap d_out");
    const dim3 grid((unsigned)((p->tracks + kDynTracks - 1) / kDynTracks));
    const bool vec = all_aligned16({d_in, d_out, d_key}) && p->bufsize % 4 == 0;
    const bool ramp = p->params.pending;
#define GAB_DYN(VV, KK, RR)                                                                                        \
    dyn_kernel<VV, KK, RR><<<grid, kDynTracks, 0, s>>>(d_in, d_key, d_out, d_gr, p->smooth.get(),                  \
                                                        p->params.current.get(), p->params.target.get(),           \
                                                        p->params.ramp.get(), p->tracks, p->bufsize, n_buffers,    \
                                                        p->link)
#define GAB_DYN_R(VV, KK) do { if (ramp) GAB_DYN(VV, KK, true); else GAB_DYN(VV, KK, false); } while (0)
    if (vec) {
        if (d_key) GAB_DYN_R(true, true); else GAB_DYN_R(true, false);
    } else {
        if (d_key) GAB_DYN_R(false, true); else GAB_DYN_R(false, false);
    }
#undef GAB_DYN_R
#undef GAB_DYN
    if (int rc = launch_status("dyn_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int dyn_set_range(gab_dyn_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                  hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_DYN_FIELDS;
    return check_then(p->flag, s, who, d_params, n, DynRule{}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * GAB_DYN_FIELDS, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_dyn_create(gab_dyn_plan** out, int tracks, int bufsize, int link) {
    return gab::create_entry("gab_dyn_create", out, tracks, bufsize, [&] {
        if (link < 1 || link > gab::kDynMaxLink || (link & (link - 1)) != 0)
            return gab::bad_arg("gab_dyn_create: link must be a power of two in 1..64");
        if (tracks % link != 0) return gab::bad_arg("gab_dyn_create: tracks must be a multiple of link");
        return GAB_OK;
    }, [&](gab_dyn_plan& p) {
        p.link = link;
        p.params.create((size_t)tracks * GAB_DYN_FIELDS, bufsize);
        p.smooth.alloc((size_t)tracks);
        p.flag.alloc(1);
        // pass-through: {0, 0, 0, 0, 0, 0, 1, -256} on every track, a smoothed gain of 0
        p.params.fill({0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, -256.0f}, tracks);
        GAB_HIP_CHECK(hipMemset(p.smooth.get(), 0, (size_t)tracks * sizeof(float)));
        return GAB_OK;
    });
}

int gab_dyn_destroy(gab_dyn_plan* plan) { return gab::destroy_plan(plan, "gab_dyn_destroy: null pointer"); }

int gab_dyn_set_params(gab_dyn_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_dyn_set_params", gab::dyn_set_range, plan, d_params, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_dyn_set_params_tracks(gab_dyn_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream) {
    return gab::set_entry("gab_dyn_set_params_tracks", gab::dyn_set_range, plan, d_params, false, first_track, n_tracks, ramp,
                          gab::as_stream(stream));
}

int gab_dyn_reset(gab_dyn_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_dyn_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->smooth.get(), 0, plan->smooth.size() * sizeof(float), s));
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_dyn_process(gab_dyn_plan* plan, const float* d_in, const float* d_key, float* d_out, float* d_gr,
                    gab_stream_t stream) {
    return gab::entry("gab_dyn_process", {plan, d_in, d_out}, [&] {
        return gab::dyn_process(plan, d_in, d_key, d_out, d_gr, 1, gab::as_stream(stream), "gab_dyn_process");
    });
}

int gab_dyn_process_batch(gab_dyn_plan* plan, const float* d_in, const float* d_key, float* d_out, float* d_gr,
                          int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_dyn_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::dyn_process(plan, d_in, d_key, d_out, d_gr, n_buffers, gab::as_stream(stream),
                                "gab_dyn_process_batch");
    });
}

int gab_dyn_params(gab_dyn_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_dyn_params", plan, &gab_dyn_plan::params, d_current, d_target, n_floats);
}

int gab_dyn_state(gab_dyn_plan* plan, float** d_smooth, size_t* n_floats) {
    return gab::entry("gab_dyn_state", {plan, d_smooth, n_floats}, [&] {
        *d_smooth = plan->smooth.get();
        *n_floats = plan->smooth.size();
        return GAB_OK;
    });
}

int gab_dyn_poly(const float** log2_coeffs, int* n_log2, const float** exp2_coeffs, int* n_exp2) {
    return gab::entry("gab_dyn_poly", {log2_coeffs, n_log2, exp2_coeffs, n_exp2}, [&] {
        *log2_coeffs = gab::kDynLog2;
        *n_log2 = 7;
        *exp2_coeffs = gab::kDynExp2;
        *n_exp2 = 7;
        return GAB_OK;
    });
}

}  // extern "C"
