// k_gate.hip — the gate plan: a noise gate / ducker per track, a two-state machine with hysteresis and a hold counter
// whose linear gain glides between two levels; seven parameters {open, close, att, rel, g_open, g_closed, hold}, six
// of which can be ramped over one buffer, linked detectors and a side chain (include/gab_c_api.h, gab_gate_*).  No
// counterpart in the reference.
//
//   gate_kernel<VEC, KEY, RAMP>  a workgroup is four waves and owns 64 tracks for the whole launch, every buffer of a
//                                batch included; each wave owns 16 of them and walks the stream in chunks of 64
//                                samples:
//                                  0. the NEXT chunk's loads are issued (the input's, the key's), into registers of
//                                     their own, so that they fly while this chunk is worked on;
//                                  1. pointwise, a lane per 4 rows x 4 samples, the 16 lanes of a row along time: the
//                                     link group's detector maximum (inside the lane for groups of 2 and 4, across
//                                     lanes 16 and 32 apart for 8 and 16, across the workgroup's waves through LDS for
//                                     32 and 64), the sample's class (above open, between, below close), and from the
//                                     classes the STATE of every sample, by three integer prefix maxima along the row
//                                     (below); the goal tg and the coefficient al of every sample into two LDS tiles;
//                                  2. serial, lanes 0..15 a track each: g = fmaf(al, g - tg, tg) down the row in order,
//                                     written over tg;
//                                  3. pointwise again: the product with the chunk held in registers, the store.
//                                The block is read once and written once.  The waves of a workgroup meet at a barrier
//                                only where link > 16 (once per chunk); a link group is at most 64 tracks and
//                                tracks % link == 0, so a group never straddles two workgroups.
//
// The count without a serial pass.  The contract's c is an integer and never reads g, so whether sample t is open can
// be told from the classes alone, exactly: with
//     r(t)  the latest sample <= t that is not below close (every such sample re-arms the hold of an open gate); if the
//           chunk has none yet, the sample c_in - H - 1 before the chunk at which the carried count would have been H,
//     dead(t) = below(t) and t - r(t) > H: the hold has run out, the gate is shut whatever it was,
//     A(t)  the latest sample <= t above open (from -1 if the gate came in open), D(t) the latest dead one,
// the gate is open at t if and only if A(t) > D(t), and then c = H - (t - r(t)); shut, c = -1.  "The latest sample <= t
// with a property" is a prefix maximum of sample numbers: four values inside the lane, then four row_shr steps across
// the row's 16 lanes.  (Why: while open, every sample that is not below re-arms, so the count at t is H less the
// length of the run of below samples ending at t; the gate shuts exactly where such a run passes H; once shut only a
// sample above open opens it, and a run counted from a sample that did not re-arm a shut gate can only mark samples
// dead at which the gate is shut anyway or which a later above sample overrides.)
//   gate_reset_kernel            count := -1, gain := target[g_closed].
//   GateRule                     refuses a parameter row outside the contract, naming the first (gab_plan.hpp's check
//                                kernel).
//
// The sequence of roundings per sample is the header's; the cut decides only where a value is held, so every launch
// form, alignment and track count gives the same bits.  Why 16 tracks a wave and not 64 (k_dynamics.hip): DESIGN.md §4h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kGateTracks = 64;           // tracks of a workgroup: the largest link group
constexpr int kGateWaves = 4;             // its waves
constexpr int kGateWaveTracks = 16;       // tracks of a wave: the lanes of its serial phase
constexpr int kGateChunk = 64;            // samples of a chunk
constexpr int kGatePitch = 68;            // row pitch in words: 16-byte aligned rows, conflict-free b128 access (kEqPitch)
constexpr int kGateRows = 4;              // rows of a lane in the pointwise phases: rows 4 (lane / 16) + i, 4 samples each
constexpr int kGateMaxLink = 64;

// A hand-off through LDS inside the wave (k_delay.hip's): words that some lanes wrote or read are touched by other
// lanes next.
__device__ __forceinline__ void gate_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float gate_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }

// A chunk's words in registers: the input's and, with a key, the key's.
struct GateChunk {
    float x[kGateRows][4];
    float k[kGateRows][4];
};

// What a wave carries through a launch.
struct GateWave {
    float* tg;                  // [16][kGatePitch]: the goal of every sample, then the gain
    float* al;                  // [16][kGatePitch]: the coefficient of every sample
    float* xmax;                // [2][4][kGateChunk]: the waves' detector maxima, link > 16, by the chunk's parity
    int lane, wave, link, parity;
    // the lane's four pointwise rows (the same in the 16 lanes of a row)
    size_t row_at[kGateRows];   // first word of the row within a block (a row below the last track: the last track's)
    bool row_live[kGateRows];
    const float* ptab;          // [16][8]: the target rows of the wave's tracks (in LDS: registers are the scarcer)
    const float* pcur;          // [16][8]: the current rows (RAMP)
    int c[kGateRows], n_open[kGateRows];
    float g;                    // lane = track, lanes 0..15: the gain
};

// Every load is unconditional, so that all of them are in flight before the first is used: a row below the last track
// reads the last track's, a sample behind the buffer's end the chunk's first.  Such a value is never stored, never
// enters a recurrence, and a link group never mixes rows of the two kinds.
template <bool VEC, bool KEY>
__device__ __forceinline__ void gate_load(GateChunk& ch, const GateWave& w, const float* x, const float* k, int s0, int B) {
    const int q = (w.lane & 15) * 4;
    const int len = B - s0 < kGateChunk ? B - s0 : kGateChunk;
    const int qc = q < len ? q : 0;                                   // VEC: len is a multiple of 4, so q < len covers q + 3
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) {
        const size_t at = w.row_at[i] + s0;
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(x + at + qc);
            ch.x[i][0] = v.x; ch.x[i][1] = v.y; ch.x[i][2] = v.z; ch.x[i][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) ch.x[i][j] = x[at + (q + j < len ? q + j : 0)];
        }
    }
    if constexpr (KEY) {
#pragma unroll
        for (int i = 0; i < kGateRows; ++i) {
            const size_t at = w.row_at[i] + s0;
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(k + at + qc);
                ch.k[i][0] = v.x; ch.k[i][1] = v.y; ch.k[i][2] = v.z; ch.k[i][3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) ch.k[i][j] = k[at + (q + j < len ? q + j : 0)];
            }
        }
    }
}

// The point at which a load must have landed: the compiler places its wait for it here and not later.
__device__ __forceinline__ void gate_landed(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void gate_landed(int& v) { asm volatile("" : "+v"(v)); }

// The same for a chunk's words.  (Left to itself the compiler waited at the head of the chunk loop, for the loads it
// had just issued.)
template <bool KEY>
__device__ __forceinline__ void gate_landed(GateChunk& ch) {
#pragma unroll
    for (int i = 0; i < kGateRows; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gate_landed(ch.x[i][j]);
            if constexpr (KEY) gate_landed(ch.k[i][j]);
        }
}

constexpr int kGateNever = -(1 << 30);                               // "no such sample": below every sample number and -1

// Across the 16 lanes of a row (a DPP row): the value of the lane n places before this one, `fill` where there is none.
template <int N>
__device__ __forceinline__ int gate_row_shr(int v, int fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x110 + N, 0xf, 0xf, false);
}

// The maximum of v over the lanes BEFORE this one in its row, kGateNever in the row's first lane.
__device__ __forceinline__ int gate_max_before(int v) {
    v = max(v, gate_row_shr<1>(v, kGateNever));
    v = max(v, gate_row_shr<2>(v, kGateNever));
    v = max(v, gate_row_shr<4>(v, kGateNever));
    v = max(v, gate_row_shr<8>(v, kGateNever));
    return gate_row_shr<1>(v, kGateNever);
}

// The sum of v over this lane and the lanes before it in its row: the row's sum in its last lane.
__device__ __forceinline__ int gate_sum_upto(int v) {
    v += gate_row_shr<1>(v, 0);
    v += gate_row_shr<2>(v, 0);
    v += gate_row_shr<4>(v, 0);
    v += gate_row_shr<8>(v, 0);
    return v;
}

// The serial phase of one chunk for lanes 0..15, a track each: `len` samples of the rows at tg and al, the gain written
// over the goal.  FULL: len == 64, no test per sample.
template <bool FULL>
__device__ __forceinline__ float gate_serial(float g, float4* tg, const float4* al, int len) {
    auto four = [&](int i) {
        const float4 t = tg[i], a = al[i];
        const float ts[4] = {t.x, t.y, t.z, t.w}, as[4] = {a.x, a.y, a.z, a.w};
        float gs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (FULL || 4 * i + j < len) {                           // wave-uniform: the recurrence never runs on padding
                g = fmaf(as[j], __fsub_rn(g, ts[j]), ts[j]);
                gs[j] = g;
            }
        }
        tg[i] = make_float4(gs[0], gs[1], gs[2], gs[3]);
    };
    if constexpr (FULL) {
#pragma unroll 4
        for (int i = 0; i < kGateChunk / 4; ++i) four(i);
    } else {
        for (int i = 0; 4 * i < len; ++i) four(i);
    }
    return g;
}

// One chunk, its words already in ch; nx: the next chunk's, in flight until the serial phase is over.  y: the block of
// this buffer; ramp: the table [B].
template <bool VEC, bool KEY, bool RAMPING>
__device__ __forceinline__ void gate_chunk(GateWave& w, const GateChunk& ch, GateChunk& nx, float* y,
                                           const float* __restrict__ ramp, int s0, int B) {
    const int lane = w.lane;
    const int r0 = (lane >> 4) * kGateRows, q = (lane & 15) * 4;
    const int len = B - s0 < kGateChunk ? B - s0 : kGateChunk;
    // ---- 1. the detector: |key| from 0 (a NaN is ignored), the maximum over the link group's rows ----
    float a[kGateRows][4];
#pragma unroll
    for (int i = 0; i < kGateRows; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[i][j] = fmaxf(0.0f, fabsf(KEY ? ch.k[i][j] : ch.x[i][j]));
#pragma unroll
    for (int d = 1; d < kGateRows; d *= 2) {
        if (w.link > d) {                                            // workgroup-uniform, as every test of link below
#pragma unroll
            for (int i = 0; i < kGateRows; ++i) {
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
    for (int d = kGateRows; d < kGateWaveTracks; d *= 2) {           // rows 4 and 8 apart: lanes 16 and 32 apart
        if (w.link > d) {
#pragma unroll
            for (int i = 0; i < kGateRows; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[i][j] = fmaxf(a[i][j], __shfl_xor(a[i][j], 4 * d, 64));
        }
    }
    if (w.link > kGateWaveTracks) {
        // Every row of the wave holds the wave's maximum now.  The waves exchange theirs through LDS, one barrier a
        // chunk: the two halves of xmax alternate, and a wave that writes a half again has passed the barrier behind
        // the other half, which every wave reaches only after it has read this one.
        float* xm = w.xmax + w.parity * (kGateWaves * kGateChunk);
        w.parity ^= 1;
        if (lane < 16) *reinterpret_cast<float4*>(xm + w.wave * kGateChunk + q) = make_float4(a[0][0], a[0][1], a[0][2], a[0][3]);
        __syncthreads();
        float4 m = *reinterpret_cast<const float4*>(xm + (w.wave ^ 1) * kGateChunk + q);
        if (w.link > 2 * kGateWaveTracks) {
            const float4 m2 = *reinterpret_cast<const float4*>(xm + (w.wave ^ 2) * kGateChunk + q);
            const float4 m3 = *reinterpret_cast<const float4*>(xm + (w.wave ^ 3) * kGateChunk + q);
            m.x = fmaxf(m.x, fmaxf(m2.x, m3.x)); m.y = fmaxf(m.y, fmaxf(m2.y, m3.y));
            m.z = fmaxf(m.z, fmaxf(m2.z, m3.z)); m.w = fmaxf(m.w, fmaxf(m2.w, m3.w));
        }
        const float mm[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
        for (int i = 0; i < kGateRows; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] = fmaxf(a[i][j], mm[j]);
    }
    // ---- the state of every sample from the classes (the head of this file), then its goal and coefficient ----
    float rr[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if constexpr (RAMPING) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rr[j] = ramp[s0 + (q + j < len ? q + j : 0)];
    }
    const int t_end = len - 1;                                       // the chunk's last sample: lane t_end / 4 of a row holds it
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) {
        const float4 t03 = *reinterpret_cast<const float4*>(w.ptab + (r0 + i) * 8);
        const float4 t47 = *reinterpret_cast<const float4*>(w.ptab + (r0 + i) * 8 + 4);
        const float tgt[6] = {t03.x, t03.y, t03.z, t03.w, t47.x, t47.y};
        const int H = (int)t47.z, c_in = w.c[i];
        float p[4][6];                                               // the row's parameters at the lane's four samples
        if constexpr (RAMPING) {
            const float4 c03 = *reinterpret_cast<const float4*>(w.pcur + (r0 + i) * 8);
            const float4 c47 = *reinterpret_cast<const float4*>(w.pcur + (r0 + i) * 8 + 4);
            const float cur[6] = {c03.x, c03.y, c03.z, c03.w, c47.x, c47.y};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int f = 0; f < 6; ++f) p[j][f] = gate_ramp(cur[f], tgt[f], rr[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int f = 0; f < 6; ++f) p[j][f] = tgt[f];
        }
        bool above[4], below[4];
        int not_below[4], run = kGateNever;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            above[j] = a[i][j] > p[j][0];
            below[j] = !above[j] && !(a[i][j] >= p[j][1]);
            run = below[j] ? run : q + j;
            not_below[j] = run;
        }
        const int nb_before = gate_max_before(run);
        const int r_in = c_in - H - 1;
        int r[4], dead[4], opened[4];
        run = kGateNever;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int last = max(not_below[j], nb_before);
            r[j] = last >= 0 ? last : r_in;
            run = (below[j] && q + j - r[j] > H) ? q + j : run;
            dead[j] = run;
        }
        const int dead_before = gate_max_before(run);
        run = kGateNever;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            run = above[j] ? q + j : run;
            opened[j] = run;
        }
        const int opened_before = max(gate_max_before(run), c_in >= 0 ? -1 : kGateNever);
        float tg[4], al[4];
        int n = 0, c_end = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool o = max(opened[j], opened_before) > max(dead[j], dead_before);
            tg[j] = o ? p[j][4] : p[j][5];
            al[j] = o ? p[j][2] : p[j][3];
            n += (o && q + j < len) ? 1 : 0;
            if (j == (t_end & 3)) c_end = o ? H - (q + j - r[j]) : -1;          // wave-uniform
        }
        *reinterpret_cast<float4*>(w.tg + (r0 + i) * kGatePitch + q) = make_float4(tg[0], tg[1], tg[2], tg[3]);
        *reinterpret_cast<float4*>(w.al + (r0 + i) * kGatePitch + q) = make_float4(al[0], al[1], al[2], al[3]);
        w.n_open[i] += gate_sum_upto(n);                             // the row's count in the row's last lane
        w.c[i] = __shfl(c_end, (lane & 48) | (t_end >> 2), 64);      // the count behind the chunk's last sample, to the whole row
    }
    gate_wave_order();
    // ---- 2. the gain, a lane per track, in order ----
    if (lane < kGateWaveTracks) {
        float4* tg = reinterpret_cast<float4*>(w.tg + lane * kGatePitch);
        const float4* al = reinterpret_cast<const float4*>(w.al + lane * kGatePitch);
        if (len == kGateChunk) w.g = gate_serial<true>(w.g, tg, al, len);
        else w.g = gate_serial<false>(w.g, tg, al, len);
    }
    gate_wave_order();
    // ---- 3. the product and the store ----
    // The next chunk's loads are waited for here, in front of this chunk's stores: behind them the wait would be for
    // the stores as well (one counter, in order), and at the head of the next chunk there is then nothing to wait for.
    gate_landed<KEY>(nx);
    float o[kGateRows][4];
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) {
        const float4 gv = *reinterpret_cast<const float4*>(w.tg + (r0 + i) * kGatePitch + q);
        const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i][j] = __fmul_rn(ch.x[i][j], gg[j]);
    }
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) {
        const size_t at = w.row_at[i] + s0 + q;
        if constexpr (VEC) {
            if (w.row_live[i] && q < len) *reinterpret_cast<float4*>(y + at) = make_float4(o[i][0], o[i][1], o[i][2], o[i][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (w.row_live[i] && q + j < len) y[at + j] = o[i][j];
        }
    }
    gate_wave_order();                                               // the tiles are free for the next chunk
}

// Grid: x = group of 64 tracks, four waves of 16.  in / key / out: [n][T][B]; out may be in (a chunk is read before it
// is written, by the same wave, and the chunk that is prefetched is another one); key is only read.  act: [n][T] or
// null.  gain, count: [T].  VEC: all blocks 16-byte aligned and B a multiple of 4.  RAMP: the launch's first buffer runs
// the ramp from cur to tgt; every other buffer takes tgt.  The hold is tgt's on every buffer.
template <bool VEC, bool KEY, bool RAMP>
__global__ __launch_bounds__(kGateWaves * 64) void gate_kernel(const float* in, const float* key, float* out, int* act,
                                                               float* __restrict__ gain, int* __restrict__ count,
                                                               const float* __restrict__ cur, const float* __restrict__ tgt,
                                                               const float* __restrict__ ramp, int T, int B,
                                                               int n_buffers, int link) {
    __shared__ __attribute__((aligned(16))) float tile_tg[kGateWaves][kGateWaveTracks * kGatePitch];
    __shared__ __attribute__((aligned(16))) float tile_al[kGateWaves][kGateWaveTracks * kGatePitch];
    __shared__ __attribute__((aligned(16))) float xmax[2 * kGateWaves * kGateChunk];
    __shared__ __attribute__((aligned(16))) float ptab[kGateWaves][kGateWaveTracks * 8];
    __shared__ __attribute__((aligned(16))) float pcur[RAMP ? kGateWaves : 1][RAMP ? kGateWaveTracks * 8 : 4];
    GateWave w;
    w.lane = threadIdx.x & 63; w.wave = threadIdx.x >> 6; w.link = link; w.parity = 0;
    w.tg = tile_tg[w.wave]; w.al = tile_al[w.wave]; w.xmax = xmax;
    const int t0 = blockIdx.x * kGateTracks + w.wave * kGateWaveTracks;
    const int row0 = t0 + (w.lane >> 4) * kGateRows;                 // the first of the lane's pointwise rows
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) {
        const int r = row0 + i;
        const size_t rc = (size_t)(r < T ? r : T - 1);
        w.row_live[i] = r < T;
        w.row_at[i] = rc * B;
        w.c[i] = count[rc];
        w.n_open[i] = 0;
    }
    const int track = t0 + w.lane;
    const bool owner = w.lane < kGateWaveTracks && track < T;
    const size_t tc = (size_t)(owner ? track : T - 1);               // a lane without a track: the last one's, never stored
    w.g = gain[tc];
    // the rows of the wave's tracks into LDS, a lane per track
    w.ptab = ptab[w.wave];
    w.pcur = pcur[RAMP ? w.wave : 0];
    if (w.lane < kGateWaveTracks) {
#pragma unroll
        for (int f = 0; f < GAB_GATE_FIELDS; ++f) {
            ptab[w.wave][w.lane * 8 + f] = tgt[tc * GAB_GATE_FIELDS + f];
            if constexpr (RAMP) pcur[w.wave][w.lane * 8 + f] = cur[tc * GAB_GATE_FIELDS + f];
        }
    }
    gate_wave_order();
    // Everything loaded so far has landed before the chunk loop is entered: a load still in flight at its head would be
    // waited for in every round, and the round's own prefetch with it.
#pragma unroll
    for (int i = 0; i < kGateRows; ++i) gate_landed(w.c[i]);
    gate_landed(w.g);

    const size_t block = (size_t)T * B;
    const bool row_end = (w.lane & 15) == 15;                        // the lane that holds a row's count of open samples
    GateChunk ch, nx;
    gate_load<VEC, KEY>(ch, w, in, key, 0, B);
    gate_landed<KEY>(ch);
    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x = in + nb * block;
        const float* k = KEY ? key + nb * block : nullptr;
        float* y = out + nb * block;
        for (int s0 = 0; s0 < B; s0 += kGateChunk) {
            // ---- 0. the next chunk's loads, of this buffer or of the next ----
            const bool last = s0 + kGateChunk >= B;
            if (!last) gate_load<VEC, KEY>(nx, w, x, k, s0 + kGateChunk, B);
            else if (nb + 1 < n_buffers) gate_load<VEC, KEY>(nx, w, x + block, KEY ? k + block : nullptr, 0, B);
            if (RAMP && nb == 0) gate_chunk<VEC, KEY, RAMP>(w, ch, nx, y, ramp, s0, B);
            else gate_chunk<VEC, KEY, false>(w, ch, nx, y, ramp, s0, B);
            ch = nx;
        }
#pragma unroll
        for (int i = 0; i < kGateRows; ++i) {
            if (act && row_end && w.row_live[i]) act[(size_t)nb * T + row0 + i] = w.n_open[i];
            w.n_open[i] = 0;
        }
    }
    if (owner) gain[track] = w.g;
#pragma unroll
    for (int i = 0; i < kGateRows; ++i)
        if (row_end && w.row_live[i]) count[row0 + i] = w.c[i];
}

// gain: [T], count: [T], tgt: [T][7]
__global__ __launch_bounds__(256) void gate_reset_kernel(float* __restrict__ gain, int* __restrict__ count,
                                                         const float* __restrict__ tgt, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) {
        gain[t] = tgt[(size_t)t * GAB_GATE_FIELDS + 5];
        count[t] = -1;
    }
}

const char* const kGateFields[GAB_GATE_FIELDS] = {"open", "close", "att", "rel", "g_open", "g_closed", "hold"};
const char* const kGateRules[GAB_GATE_FIELDS] = {
    "must be within [0, 2^64]", "must be within [0, open]", "must be within [0, 1 - 2^-20]",
    "must be within [0, 1 - 2^-20]", "must be within [0, 256]", "must be within [0, 256]",
    "must be an integer within [0, 2^24]"};

// src: [n_rows][7] (a NaN fails every comparison).  close is held against the open of its own row, the value before it.
struct GateRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i % GAB_GATE_FIELDS);
        bool bad = not_finite(__float_as_uint(v)) || !(v >= 0.0f);
        if (field == 0) bad = bad || !(v <= 0x1p64f);
        if (field == 1) bad = bad || !(v <= src[i - 1]);
        if (field == 2 || field == 3) bad = bad || !(v <= 0x1.ffffep-1f);                   // 1 - 2^-20
        if (field == 4 || field == 5) bad = bad || !(v <= 256.0f);
        if (field == 6) bad = bad || !(v <= 0x1p24f) || truncf(v) != v;
        return bad;
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % GAB_GATE_FIELDS);
        return row_refusal(i, GAB_GATE_FIELDS, first_track, kGateFields[field], kGateRules[field]);
    }
};

}  // namespace
}  // namespace gab

struct gab_gate_plan {
    int tracks = 0, bufsize = 0, link = 0;
    gab::RampedTable params;           // current, target: [T][7]
    gab::DeviceBuf<float> gain;        // [T]: the gliding linear gain
    gab::DeviceBuf<int> count;         // [T]: the hold counter, -1 while closed
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch; then, if a ramp ran through the first of them, current := target.  Nothing is allocated and
// nothing waits here.
int gate_process(gab_gate_plan* p, const float* d_in, const float* d_key, float* d_out, int* d_act, int n_buffers,
                 hipStream_t s, const char* who) {
    if (d_key && overlaps(d_key, d_out, (size_t)n_buffers * p->tracks * p->bufsize))
        return refuse(who, "d_key may not overlap d_out");
    const dim3 grid((unsigned)((p->tracks + kGateTracks - 1) / kGateTracks));
    const bool vec = all_aligned16({d_in, d_out, d_key}) && p->bufsize % 4 == 0;
    const bool ramp = p->params.pending;
#define GAB_GATE(VV, KK, RR)                                                                                       \
    gate_kernel<VV, KK, RR><<<grid, kGateWaves * 64, 0, s>>>(d_in, d_key, d_out, d_act, p->gain.get(),             \
                                                             p->count.get(), p->params.current.get(),              \
                                                             p->params.target.get(), p->params.ramp.get(),         \
                                                             p->tracks, p->bufsize, n_buffers, p->link)
#define GAB_GATE_R(VV, KK) do { if (ramp) GAB_GATE(VV, KK, true); else GAB_GATE(VV, KK, false); } while (0)
    if (vec) {
        if (d_key) GAB_GATE_R(true, true); else GAB_GATE_R(true, false);
    } else {
        if (d_key) GAB_GATE_R(false, true); else GAB_GATE_R(false, false);
    }
#undef GAB_GATE_R
#undef GAB_GATE
    if (int rc = launch_status("gate_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int gate_set_range(gab_gate_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                   hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_GATE_FIELDS;
    return check_then(p->flag, s, who, d_params, n, GateRule{}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * GAB_GATE_FIELDS, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_gate_create(gab_gate_plan** out, int tracks, int bufsize, int link) {
    return gab::create_entry("gab_gate_create", out, tracks, bufsize, [&] {
        if (link < 1 || link > gab::kGateMaxLink || (link & (link - 1)) != 0)
            return gab::bad_arg("gab_gate_create: link must be a power of two in 1..64");
        if (tracks % link != 0) return gab::bad_arg("gab_gate_create: tracks must be a multiple of link");
        return GAB_OK;
    }, [&](gab_gate_plan& p) {
        p.link = link;
        p.params.create((size_t)tracks * GAB_GATE_FIELDS, bufsize);
        p.gain.alloc((size_t)tracks);
        p.count.alloc((size_t)tracks);
        p.flag.alloc(1);
        // pass-through: {0, 0, 0, 0, 1, 1, 0} on every track, a gain of 1, a count of -1
        p.params.fill({0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f}, tracks);
        p.gain.fill(1.0f);
        p.count.fill(-1);
        return GAB_OK;
    });
}

int gab_gate_destroy(gab_gate_plan* plan) { return gab::destroy_plan(plan, "gab_gate_destroy: null pointer"); }

int gab_gate_set_params(gab_gate_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_gate_set_params", gab::gate_set_range, plan, d_params, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_gate_set_params_tracks(gab_gate_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                               gab_stream_t stream) {
    return gab::set_entry("gab_gate_set_params_tracks", gab::gate_set_range, plan, d_params, false, first_track, n_tracks,
                          ramp, gab::as_stream(stream));
}

int gab_gate_reset(gab_gate_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_gate_reset", {plan}, [&]() -> int {
        hipStream_t s = gab::as_stream(stream);
        gab::gate_reset_kernel<<<dim3((unsigned)((plan->tracks + 255) / 256)), 256, 0, s>>>(
            plan->gain.get(), plan->count.get(), plan->params.target.get(), plan->tracks);
        if (int rc = gab::launch_status("gate_reset_kernel")) return rc;
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_gate_process(gab_gate_plan* plan, const float* d_in, const float* d_key, float* d_out, int* d_act,
                     gab_stream_t stream) {
    return gab::entry("gab_gate_process", {plan, d_in, d_out}, [&] {
        return gab::gate_process(plan, d_in, d_key, d_out, d_act, 1, gab::as_stream(stream), "gab_gate_process");
    });
}

int gab_gate_process_batch(gab_gate_plan* plan, const float* d_in, const float* d_key, float* d_out, int* d_act,
                           int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_gate_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::gate_process(plan, d_in, d_key, d_out, d_act, n_buffers, gab::as_stream(stream),
                                 "gab_gate_process_batch");
    });
}

int gab_gate_params(gab_gate_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_gate_params", plan, &gab_gate_plan::params, d_current, d_target, n_floats);
}

int gab_gate_state(gab_gate_plan* plan, float** d_gain, int** d_count, size_t* n_tracks) {
    return gab::entry("gab_gate_state", {plan, d_gain, d_count, n_tracks}, [&] {
        *d_gain = plan->gain.get();
        *d_count = plan->count.get();
        *n_tracks = plan->gain.size();
        return GAB_OK;
    });
}

}  // extern "C"
