// k_limiter.hip — the limiter plan: a brickwall look-ahead limiter per track with a window W = 2^k, three parameters
// {drive, ceil, rel} that can be ramped over one buffer, linked detectors and three carried histories of W - 1 samples
// (include/gab_c_api.h, gab_lim_*).  No counterpart in the reference.
//
//   lim_kernel<K, VEC, RAMP>  a workgroup is one wave and owns 8 tracks for the whole launch, every buffer of a batch
//                             included.  Per track it keeps three rings in LDS, xd, t and e: H = max(W, 64) words of
//                             history and the 64 of the chunk at hand.  It walks the buffer in chunks of 64 samples:
//                               1. pointwise, a lane per sample, the 8 rows in registers: the drive, the link group's
//                                  detector across the rows, the need t; xd and t into their rings;
//                               2. the window minimum m of every row, lanes along time (lim_window), into the e ring;
//                               3. serial, a lane per track: the release over the row of m in order, e written over it
//                                  (whole chunks that do not wrap in the ring without a test per sample);
//                               4. lanes along time again: the box sum of e (lim_window), the gain, the product with
//                                  the delayed xd, the store.
//                             The block is read once and written once, the histories once per launch; nothing leaves the
//                             wave, so there is no workgroup barrier.
//   lim_window<K, SUM, NR>    the doubling recursion V_2h[n] = V_h[n] op V_h[n - h] with a lane per sample: below 64 the
//                             neighbour comes by a lane shuffle, the lanes that reach into the 64 samples before from
//                             the pass before; from 64 on the neighbour is the same lane of an earlier pass.  The
//                             history's passes are recomputed from the ring for every chunk (H / 64 of them): nothing
//                             but the three histories is carried.  NR rows run side by side, for the shuffles' latency.
//   lim_detector_kernel       link groups of 16, 32 and 64 tracks are wider than a wave's 8: their detector is written into
//                             a block of the plan's by a launch in front (and a batch goes buffer by buffer).
//   LimRule                   refuses a parameter row outside the contract, naming the first (gab_plan.hpp's check kernel).
//
// The sequence of roundings per sample is the header's; the cut decides only where a value is held, so every launch
// form, alignment, bufsize and track count gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kLimTracks = 8;             // tracks of a workgroup (one wave): the lanes of the serial phase
constexpr int kLimChunk = 64;             // samples of a chunk: the lanes of the other phases
constexpr int kLimSide = 8;               // rows whose window minima run side by side
constexpr int kLimMaxLink = 64;
constexpr int kLimPF = 4;                 // floats of a parameter row in LDS (GAB_LIM_FIELDS, padded)

template <int K>
struct LimShape {
    static constexpr int W = 1 << K;
    static constexpr int D = W - 1;                   // the latency, and the words of a history
    static constexpr int H = W < 64 ? 64 : W;         // history words of a ring: whole passes of 64; the oldest H - D unused
    static constexpr int A = H / 64;                  // passes over the history in front of the chunk's
    static constexpr int R = H + kLimChunk;           // words of a ring
    static constexpr int P = R + 1;                   // row pitch: odd, so the serial phase's lanes hit 8 banks
};

// A hand-off through LDS inside the wave (k_dynamics.hip's).
__device__ __forceinline__ void lim_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float lim_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }

// Word p of a ring (0: the oldest, R - 1: the chunk's last) whose word 0 sits at `base`.
template <int K>
__device__ __forceinline__ int lim_pos(int base, int p) {
    const int i = base + p;
    return i >= LimShape<K>::R ? i - LimShape<K>::R : i;
}

// The need of a detector value d >= 0 (never a NaN) against the ceiling c.
__device__ __forceinline__ float lim_need(float d, float c) {
    float q = __fdiv_rn(c, d);
    if (__fmul_rn(q, d) > c) q = __uint_as_float(__float_as_uint(q) - 1u);   // q is not +0 here: 0 * d > c is false
    return d <= c ? 1.0f : q;
}

// V_W of the chunk's 64 samples, a lane each: V_1 = the ring's words (the chunk's own is `cur`), V_2h[n] = V_h[n] op
// V_h[n - h], op = + (SUM) or fminf.  A lane of pass 0 whose window reaches in front of the ring gets a value that
// nothing reads: a chunk sample's window ends at word 1 or later.
// It runs NR rows (rows + r * pitch) side by side: a level is a chain of dependent lane shuffles, and a wave that is
// alone on its SIMD has nothing else to issue while one is under way.  out[r]: V_W of row r.
template <int K, bool SUM, int NR>
__device__ __forceinline__ void lim_window(const float* rows, int base, int at, int lane, float (&out)[NR]) {
    using S = LimShape<K>;
    constexpr int kLevels = K < 6 ? K : 6;
    float prev[kLevels][NR], v64[S::A + 1][NR];
#pragma unroll
    for (int l = 0; l < kLevels; ++l)
#pragma unroll
        for (int r = 0; r < NR; ++r) prev[l][r] = 0.0f;
#pragma unroll
    for (int a = 0; a <= S::A; ++a) {
        const int from = a == S::A ? at : lim_pos<K>(base, 64 * a + lane);
        float v[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) v[r] = rows[r * S::P + from];
#pragma unroll
        for (int l = 0; l < kLevels; ++l) {
            const int h = 1 << l;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float c = lane >= 64 - h ? prev[l][r] : v[r];   // the top h lanes lend the pass before
                const float nb = __shfl(c, (lane - h) & 63, 64);
                prev[l][r] = v[r];
                v[r] = SUM ? __fadd_rn(v[r], nb) : fminf(v[r], nb);
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) v64[a][r] = v[r];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if constexpr (K <= 6) {
            out[r] = v64[S::A][r];
        } else if constexpr (K == 7) {
            out[r] = SUM ? __fadd_rn(v64[2][r], v64[1][r]) : fminf(v64[2][r], v64[1][r]);
        } else {
            static_assert(K == 8, "W is at most 256");
            const float hi = SUM ? __fadd_rn(v64[4][r], v64[3][r]) : fminf(v64[4][r], v64[3][r]);   // V_128 of the chunk
            const float lo = SUM ? __fadd_rn(v64[2][r], v64[1][r]) : fminf(v64[2][r], v64[1][r]);   // V_128 of 128 before
            out[r] = SUM ? __fadd_rn(hi, lo) : fminf(hi, lo);
        }
    }
}

// What a wave carries through a launch.
struct LimWave {
    float *rx, *rt, *re;        // [8][P]: the rings of xd, t and e
    float* tile;                // [4][64] (VEC): four rows between the 16-byte and the lane-per-sample layout
    const float* ptab;          // [8][4]: the target rows
    const float* pcur;          // [8][4]: the current rows (RAMP)
    int lane, nt, link, base;
    float e;                    // lane = track: e of the sample before
    float t_rel, c_rel;
    float gr;                   // lane = track: the buffer's smallest gain
};

// One buffer.  x, y: the rows of this wave's first track in that buffer; dx: the row of this wave's link group in the
// detector block (link > 8), else null; ramp: the table [B].
template <int K, bool VEC, bool RAMPING>
__device__ __forceinline__ void lim_buffer(LimWave& w, const float* x, float* y, const float* dx,
                                           const float* __restrict__ ramp, int B, bool want_gr) {
    using S = LimShape<K>;
    const int lane = w.lane;
    [[maybe_unused]] const int q = (lane & 15) * 4, qr = lane >> 4;   // VEC: samples q..q + 3 of row 4 j + qr
    w.gr = __builtin_inff();
    for (int s0 = 0; s0 < B; s0 += kLimChunk) {
        const int len = B - s0 < kLimChunk ? B - s0 : kLimChunk;
        // A lane behind the buffer's end holds a sample of the chunk again: in single words the chunk's last (sl), in
        // the 16-byte form samples 0..3 of the chunk (qc = 0).  Whatever it holds is never stored, never enters the
        // release, and no window of a sample in front of it reaches it: windows look back.
        const int sl = lane < len ? lane : len - 1;
        const int base = w.base;
        const int at = lim_pos<K>(base, S::H + lane);                 // this lane's word of the chunk
        float rr = 1.0f;
        if constexpr (RAMPING) rr = ramp[s0 + sl];
        // ---- 1. the chunk into registers, a lane per sample; a row below the last track repeats the last track's ----
        float xv[kLimTracks], a[kLimTracks];
        if constexpr (VEC) {
            const int qc = q < len ? q : 0;                           // len is a multiple of 4, so q < len covers q + 3
            const float* xq = x + s0 + qc;
            const int last = w.nt - 1;
            // both loads are in flight before the first is staged
            const float4 v0 = *reinterpret_cast<const float4*>(xq + (size_t)(qr < last ? qr : last) * B);
            const float4 v1 = *reinterpret_cast<const float4*>(xq + (size_t)(4 + qr < last ? 4 + qr : last) * B);
            float4* mine = reinterpret_cast<float4*>(w.tile + qr * kLimChunk + q);
            const float* col = w.tile + lane;
#define GAB_LIM_STAGE(J, V)                                                                                          \
            *mine = V;                                                                                               \
            lim_wave_order();                                                                                        \
            xv[4 * J] = col[0]; xv[4 * J + 1] = col[kLimChunk]; xv[4 * J + 2] = col[2 * kLimChunk];                  \
            xv[4 * J + 3] = col[3 * kLimChunk];                                                                      \
            lim_wave_order()
            GAB_LIM_STAGE(0, v0);
            GAB_LIM_STAGE(1, v1);
            static_assert(kLimTracks == 8, "two groups of four rows");
#undef GAB_LIM_STAGE
        } else {
#pragma unroll
            for (int r = 0; r < kLimTracks; ++r) xv[r] = x[(size_t)(r < w.nt ? r : w.nt - 1) * B + s0 + sl];
        }
        // the drive; the detector: |xd| where it is finite, else 0, the maximum over the link group's rows
#pragma unroll
        for (int r = 0; r < kLimTracks; ++r) {
            const float td = w.ptab[r * kLimPF];
            const float drive = RAMPING ? lim_ramp(w.pcur[r * kLimPF], td, rr) : td;
            xv[r] = __fmul_rn(drive, xv[r]);
            const float ax = fabsf(xv[r]);
            a[r] = __float_as_uint(ax) < 0x7f800000u ? ax : 0.0f;
        }
#pragma unroll
        for (int d = 1; d < kLimTracks; d *= 2) {
            if (w.link > d) {                                        // wave-uniform
#pragma unroll
                for (int r = 0; r < kLimTracks; ++r) {
                    if ((r & d) == 0) {
                        const float m = fmaxf(a[r], a[r | d]);
                        a[r] = m;
                        a[r | d] = m;
                    }
                }
            }
        }
        if (dx) {                                                    // a group wider than the wave: the launch in front
            const float dv = dx[s0 + sl];
#pragma unroll
            for (int r = 0; r < kLimTracks; ++r) a[r] = dv;
        }
#pragma unroll
        for (int r = 0; r < kLimTracks; ++r) {
            const float tc = w.ptab[r * kLimPF + 1];
            const float c = RAMPING ? lim_ramp(w.pcur[r * kLimPF + 1], tc, rr) : tc;
            w.rx[r * S::P + at] = xv[r];
            w.rt[r * S::P + at] = lim_need(a[r], c);
        }
        lim_wave_order();
        // ---- 2. the window minimum, lanes along time ----
#pragma unroll 1
        for (int r0 = 0; r0 < kLimTracks; r0 += kLimSide) {
            float m[kLimSide];
            lim_window<K, false, kLimSide>(w.rt + r0 * S::P, base, at, lane, m);
#pragma unroll
            for (int i = 0; i < kLimSide; ++i) w.re[(r0 + i) * S::P + at] = m[i];
        }
        lim_wave_order();
        // ---- 3. the release, a lane per track, in order ----
        if (lane < kLimTracks) {
            float* row = w.re + lane * S::P;
            float e = w.e;
            const float d_rel = __fsub_rn(w.t_rel, w.c_rel);
            const int p0 = lim_pos<K>(base, S::H);
            int sb = 0;
            if (len == kLimChunk && p0 + kLimChunk <= S::R) {
                // a whole chunk whose words lie in one piece (every chunk of a buffer that is a multiple of 64): no
                // test and no wrap per sample
                float* here = row + p0;
                for (; sb < kLimChunk; sb += 16) {
                    float mv[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) mv[j] = here[sb + j];
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float rel = RAMPING ? fmaf(d_rel, ramp[s0 + sb + j], w.c_rel) : w.t_rel;
                        e = fminf(mv[j], fmaf(rel, __fsub_rn(1.0f, e), e));
                        here[sb + j] = e;
                    }
                }
            }
            for (; sb < len; sb += 8) {
                float mv[8];
                int ix[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ix[j] = lim_pos<K>(base, S::H + (sb + j < kLimChunk ? sb + j : kLimChunk - 1));
                    mv[j] = row[ix[j]];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (sb + j < len) {                              // uniform: the recurrence never runs behind the end
                        const float rel = RAMPING ? fmaf(d_rel, ramp[s0 + sb + j], w.c_rel) : w.t_rel;
                        e = fminf(mv[j], fmaf(rel, __fsub_rn(1.0f, e), e));
                        row[ix[j]] = e;
                    }
                }
            }
            w.e = e;
        }
        lim_wave_order();
        // ---- 4. the box, the gain and the store, four rows at a time ----
        const int old = lim_pos<K>(base, S::H + lane - S::D);         // the word W - 1 samples before this lane's
#pragma unroll 1
        for (int j = 0; j < kLimTracks / 4; ++j) {
            float sum[4];
            lim_window<K, true, 4>(w.re + 4 * j * S::P, base, at, lane, sum);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * j + i;
                const float g = fminf(__fmul_rn(sum[i], 1.0f / (float)S::W), w.rt[r * S::P + old]);
                const float o = __fmul_rn(g, w.rx[r * S::P + old]);
                if (want_gr) {                                       // uniform
                    float m = lane < len ? g : __builtin_inff();
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) m = fminf(m, __shfl_xor(m, d, 64));
                    if (lane == r) w.gr = fminf(w.gr, m);
                }
                if constexpr (VEC) {
                    w.tile[i * kLimChunk + lane] = o;
                } else {
                    if (r < w.nt && lane < len) y[(size_t)r * B + s0 + lane] = o;
                }
            }
            if constexpr (VEC) {
                lim_wave_order();
                const int r = 4 * j + qr;
                const float4 v = *reinterpret_cast<const float4*>(w.tile + qr * kLimChunk + q);
                if (r < w.nt && q < len) *reinterpret_cast<float4*>(y + (size_t)r * B + s0 + q) = v;
                lim_wave_order();
            }
        }
        lim_wave_order();                                            // the rings are free for the next chunk
        w.base = lim_pos<K>(base, len);
    }
}

// Grid: x = group of 8 tracks, one wave.  in / out: [n][T][B]; out may be in (a chunk is read before it is written, by
// the same lane).  gr: [n][T] or null.  dext: [T / link][B] for link > 8, else null (then n_buffers is 1).  hx, ht, he:
// [T][W - 1], oldest first.  VEC: both blocks 16-byte aligned and B a multiple of 4.  RAMP: the launch's first buffer runs
// the ramp from cur to tgt; every other buffer takes tgt.
template <int K, bool VEC, bool RAMP>
__global__ __launch_bounds__(64) void lim_kernel(const float* in, float* out, float* gr, const float* __restrict__ dext,
                                                 float* __restrict__ hx, float* __restrict__ ht, float* __restrict__ he,
                                                 const float* __restrict__ cur, const float* __restrict__ tgt,
                                                 const float* __restrict__ ramp, int T, int B, int n_buffers, int link) {
    using S = LimShape<K>;
    __shared__ float rx[kLimTracks * S::P];
    __shared__ float rt[kLimTracks * S::P];
    __shared__ float re[kLimTracks * S::P];
    __shared__ __attribute__((aligned(16))) float tile[VEC ? 4 * kLimChunk : 4];
    __shared__ float ptab[kLimTracks * kLimPF];
    __shared__ float pcur[RAMP ? kLimTracks * kLimPF : 4];
    const int lane = threadIdx.x;
    const int t0 = blockIdx.x * kLimTracks;
    LimWave w;
    w.rx = rx; w.rt = rt; w.re = re; w.tile = tile; w.ptab = ptab; w.pcur = pcur;
    w.lane = lane; w.link = link; w.base = 0;
    w.nt = T - t0 < kLimTracks ? T - t0 : kLimTracks;
    // the rows of this wave's tracks, a lane per track; a row below the last track repeats the last track's
    const size_t track = (size_t)t0 + ((lane % kLimTracks) < w.nt ? (lane % kLimTracks) : w.nt - 1);
    w.t_rel = tgt[track * GAB_LIM_FIELDS + 2];
    w.c_rel = RAMP ? cur[track * GAB_LIM_FIELDS + 2] : w.t_rel;
    if (lane < kLimTracks) {
        ptab[lane * kLimPF] = tgt[track * GAB_LIM_FIELDS];
        ptab[lane * kLimPF + 1] = tgt[track * GAB_LIM_FIELDS + 1];
        if constexpr (RAMP) {
            pcur[lane * kLimPF] = cur[track * GAB_LIM_FIELDS];
            pcur[lane * kLimPF + 1] = cur[track * GAB_LIM_FIELDS + 1];
        }
    }
    w.e = he[track * S::D + S::D - 1];
    w.gr = 0.0f;
    // the histories into the rings' words [H - D, H); the words in front of them are what a new plan holds
#pragma unroll 1
    for (int r = 0; r < kLimTracks; ++r) {
        const size_t row_at = ((size_t)t0 + (r < w.nt ? r : w.nt - 1)) * S::D;
#pragma unroll
        for (int a = 0; a < S::A; ++a) {
            const int p = 64 * a + lane, j = p - (S::H - S::D);
            rx[r * S::P + p] = j >= 0 ? hx[row_at + j] : 0.0f;
            rt[r * S::P + p] = j >= 0 ? ht[row_at + j] : 1.0f;
            re[r * S::P + p] = j >= 0 ? he[row_at + j] : 1.0f;
        }
    }
    lim_wave_order();

    const size_t block = (size_t)T * B;
    const float* x = in + (size_t)t0 * B;
    float* y = out + (size_t)t0 * B;
    const float* dx = dext ? dext + (size_t)(t0 / link) * B : nullptr;
    const bool owner = lane < w.nt;
    int nb = 0;
    if constexpr (RAMP) {
        lim_buffer<K, VEC, true>(w, x, y, dx, ramp, B, gr != nullptr);
        if (gr && owner) gr[(size_t)t0 + lane] = w.gr;
        nb = 1;
    }
    for (; nb < n_buffers; ++nb) {
        lim_buffer<K, VEC, false>(w, x + nb * block, y + nb * block, dx, ramp, B, gr != nullptr);
        if (gr && owner) gr[(size_t)nb * T + t0 + lane] = w.gr;
    }
#pragma unroll 1
    for (int r = 0; r < w.nt; ++r) {
        const size_t row_at = ((size_t)t0 + r) * S::D;
#pragma unroll
        for (int a = 0; a < S::A; ++a) {
            const int p = 64 * a + lane, j = p - (S::H - S::D);
            const int from = r * S::P + lim_pos<K>(w.base, p);
            if (j >= 0) {
                hx[row_at + j] = rx[from];
                ht[row_at + j] = rt[from];
                he[row_at + j] = re[from];
            }
        }
    }
}

// The detector of link groups wider than a wave's tracks.  Grid: x = link group, y = 256 samples.  dext: [T / link][B].
template <bool RAMP>
__global__ __launch_bounds__(256) void lim_detector_kernel(const float* __restrict__ in, float* __restrict__ dext,
                                                          const float* __restrict__ cur, const float* __restrict__ tgt,
                                                          const float* __restrict__ ramp, int B, int link) {
    const int s = blockIdx.y * 256 + threadIdx.x;
    if (s >= B) return;
    const size_t first = (size_t)blockIdx.x * link;
    float rr = 1.0f;
    if constexpr (RAMP) rr = ramp[s];
    float m = 0.0f;
    for (int j = 0; j < link; ++j) {
        const float td = tgt[(first + j) * GAB_LIM_FIELDS];
        const float drive = RAMP ? lim_ramp(cur[(first + j) * GAB_LIM_FIELDS], td, rr) : td;
        const float ax = fabsf(__fmul_rn(drive, in[(first + j) * B + s]));
        m = fmaxf(m, __float_as_uint(ax) < 0x7f800000u ? ax : 0.0f);
    }
    dext[(size_t)blockIdx.x * B + s] = m;
}

const char* const kLimFields[GAB_LIM_FIELDS] = {"drive", "ceil", "rel"};
const char* const kLimRules[GAB_LIM_FIELDS] = {"must be within [0, 2^32]", "must be within [2^-32, 2^32]",
                                               "must be within [0, 1]"};

// src: [n_rows][3] (a NaN fails every comparison)
struct LimRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i % GAB_LIM_FIELDS);
        if (field == 0) return !(v >= 0.0f && v <= 0x1p+32f);
        if (field == 1) return !(v >= 0x1p-32f && v <= 0x1p+32f);
        return !(v >= 0.0f && v <= 1.0f);
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % GAB_LIM_FIELDS);
        return row_refusal(i, GAB_LIM_FIELDS, first_track, kLimFields[field], kLimRules[field]);
    }
};

}  // namespace
}  // namespace gab

struct gab_lim_plan {
    int tracks = 0, bufsize = 0, k = 0, link = 0;
    gab::RampedTable params;                   // current, target: [T][3]
    gab::DeviceBuf<float> hx, ht, he;          // [T][W - 1] each, oldest first: xd, t, e
    gab::DeviceBuf<float> dext;                // [T / link][B] for link > 8: the group detectors of the buffer at hand
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// What a new or reset plan holds: xd = 0, t = 1, e = 1.  Nothing waits here.
void lim_clear(gab_lim_plan* p, hipStream_t s) {
    static_assert(sizeof(float) == 4, "the fill below writes words");
    GAB_HIP_CHECK(hipMemsetAsync(p->hx.get(), 0, p->hx.size() * sizeof(float), s));
    GAB_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->ht.get()), 0x3f800000, p->ht.size(), s));
    GAB_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->he.get()), 0x3f800000, p->he.size(), s));
}

template <int K>
void lim_launch(gab_lim_plan* p, const float* d_in, float* d_out, float* d_gr, const float* dext, int n_buffers, bool vec,
                bool ramp, hipStream_t s) {
    const dim3 grid((unsigned)((p->tracks + kLimTracks - 1) / kLimTracks));
#define GAB_LIM(VV, RR)                                                                                             \
    lim_kernel<K, VV, RR><<<grid, kLimChunk, 0, s>>>(d_in, d_out, d_gr, dext, p->hx.get(), p->ht.get(), p->he.get(), \
                                                     p->params.current.get(), p->params.target.get(),               \
                                                     p->params.ramp.get(), p->tracks, p->bufsize, n_buffers, p->link)
    if (vec) {
        if (ramp) GAB_LIM(true, true); else GAB_LIM(true, false);
    } else {
        if (ramp) GAB_LIM(false, true); else GAB_LIM(false, false);
    }
#undef GAB_LIM
}

// n buffers in one launch (link <= 8), or per buffer the detector's launch and the limiter's (link > 8); then, if a
// ramp ran through the first of them, current := target.  Nothing is allocated and nothing waits here.
int lim_process(gab_lim_plan* p, const float* d_in, float* d_out, float* d_gr, int n_buffers, hipStream_t s,
                const char* who) {
    const size_t block = (size_t)p->tracks * p->bufsize;
    if (d_out != d_in && overlaps(d_in, d_out, (size_t)n_buffers * block))
        return refuse(who, "d_out may be d_in itself; any other overlap is refused");
    const bool vec = all_aligned16({d_in, d_out}) && p->bufsize % 4 == 0;
    const bool ramp = p->params.pending;
    const bool wide = p->link > kLimTracks;
    const int launches = wide ? n_buffers : 1, each = wide ? 1 : n_buffers;
    for (int b = 0; b < launches; ++b) {
        const float* in = d_in + b * block;
        const bool r = ramp && b == 0;
        if (wide) {
            const dim3 grid((unsigned)(p->tracks / p->link), (unsigned)((p->bufsize + 255) / 256));
            if (r)
                lim_detector_kernel<true><<<grid, 256, 0, s>>>(in, p->dext.get(), p->params.current.get(),
                                                               p->params.target.get(), p->params.ramp.get(), p->bufsize, p->link);
            else
                lim_detector_kernel<false><<<grid, 256, 0, s>>>(in, p->dext.get(), p->params.current.get(),
                                                                p->params.target.get(), p->params.ramp.get(), p->bufsize, p->link);
            if (int rc = launch_status("lim_detector_kernel")) return rc;
        }
        float* gr = d_gr ? d_gr + (size_t)b * p->tracks : nullptr;
        const float* dext = wide ? p->dext.get() : nullptr;
        switch (p->k) {
            case 2: lim_launch<2>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            case 3: lim_launch<3>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            case 4: lim_launch<4>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            case 5: lim_launch<5>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            case 6: lim_launch<6>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            case 7: lim_launch<7>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
            default: lim_launch<8>(p, in, d_out + b * block, gr, dext, each, vec, r, s); break;
        }
        if (int rc = launch_status("lim_kernel")) return rc;
    }
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int lim_set_range(gab_lim_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                  hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_LIM_FIELDS;
    return check_then(p->flag, s, who, d_params, n, LimRule{}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * GAB_LIM_FIELDS, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_lim_create(gab_lim_plan** out, int tracks, int bufsize, int lookahead_log2, int link) {
    return gab::create_entry("gab_lim_create", out, tracks, bufsize, [&] {
        if (lookahead_log2 < 2 || lookahead_log2 > 8) return gab::bad_arg("gab_lim_create: lookahead_log2 must be 2..8");
        if (link < 1 || link > gab::kLimMaxLink || (link & (link - 1)) != 0)
            return gab::bad_arg("gab_lim_create: link must be a power of two in 1..64");
        if (tracks % link != 0) return gab::bad_arg("gab_lim_create: tracks must be a multiple of link");
        return GAB_OK;
    }, [&](gab_lim_plan& p) {
        p.k = lookahead_log2;
        p.link = link;
        const size_t words = (size_t)tracks * ((1u << lookahead_log2) - 1);
        p.params.create((size_t)tracks * GAB_LIM_FIELDS, bufsize);
        p.hx.alloc(words);
        p.ht.alloc(words);
        p.he.alloc(words);
        if (link > gab::kLimTracks) p.dext.alloc((size_t)(tracks / link) * bufsize);
        p.flag.alloc(1);
        // a pure delay: {1, 2^32, 0} on every track, histories of xd = 0, t = 1, e = 1
        p.params.fill({1.0f, 0x1p+32f, 0.0f}, tracks);
        gab::lim_clear(&p, nullptr);
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_lim_destroy(gab_lim_plan* plan) { return gab::destroy_plan(plan, "gab_lim_destroy: null pointer"); }

int gab_lim_set_params(gab_lim_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_lim_set_params", gab::lim_set_range, plan, d_params, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_lim_set_params_tracks(gab_lim_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream) {
    return gab::set_entry("gab_lim_set_params_tracks", gab::lim_set_range, plan, d_params, false, first_track, n_tracks, ramp,
                          gab::as_stream(stream));
}

int gab_lim_reset(gab_lim_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_lim_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        gab::lim_clear(plan, s);
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_lim_process(gab_lim_plan* plan, const float* d_in, float* d_out, float* d_gr, gab_stream_t stream) {
    return gab::entry("gab_lim_process", {plan, d_in, d_out}, [&] {
        return gab::lim_process(plan, d_in, d_out, d_gr, 1, gab::as_stream(stream), "gab_lim_process");
    });
}

int gab_lim_process_batch(gab_lim_plan* plan, const float* d_in, float* d_out, float* d_gr, int n_buffers,
                          gab_stream_t stream) {
    return gab::batch_entry("gab_lim_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::lim_process(plan, d_in, d_out, d_gr, n_buffers, gab::as_stream(stream), "gab_lim_process_batch");
    });
}

int gab_lim_params(gab_lim_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_lim_params", plan, &gab_lim_plan::params, d_current, d_target, n_floats);
}

int gab_lim_state(gab_lim_plan* plan, float** d_x, float** d_t, float** d_e, size_t* per_track) {
    return gab::entry("gab_lim_state", {plan, d_x, d_t, d_e, per_track}, [&] {
        *d_x = plan->hx.get();
        *d_t = plan->ht.get();
        *d_e = plan->he.get();
        *per_track = ((size_t)1 << plan->k) - 1;
        return GAB_OK;
    });
}

int gab_lim_latency(gab_lim_plan* plan, int* samples) {
    return gab::entry("gab_lim_latency", {plan, samples}, [&] {
        *samples = (1 << plan->k) - 1;
        return GAB_OK;
    });
}

}  // extern "C"
