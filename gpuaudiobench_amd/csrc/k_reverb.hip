// k_reverb.hip — the reverb plan: a feedback delay network per track.  N delay lines of integer length, each read m[i]
// samples back, scaled, low-passed by a carried one-pole, mixed through the unnormalised Walsh-Hadamard matrix and
// written back with the input; O outputs tapped from the low-pass states (include/gab_c_api.h, gab_reverb_*).  No
// counterpart in the reference.
//
//   reverb_kernel<N, O, RAMP>   a workgroup is one wave and owns 64 / N tracks, that is 64 chains (track, line), for the
//                               whole launch, every buffer of a batch included.  It walks the stream in chunks of
//                               C = min(64, the smallest delay of its tracks) samples: every line is read at least C
//                               samples back, so all of a chunk's line reads end before the chunk begins.  Per chunk:
//                                 1. lanes along time: each chain's C line words from memory (coalesced, all 64 loads
//                                    requested before the first is used), g * s into an LDS tile [64 chains][68];
//                                 2. a lane per chain: the one-pole runs down its row in order, q written over v;
//                                 3. lanes along time, per owned track: the N values of a column, the butterflies in
//                                    registers, N coalesced line stores, the outputs' ordered sums and their stores.
//                               Only step 2 is serial in time.  Nothing leaves the wave: no workgroup barrier.
//   ReverbRule, ReverbDelayRule refuse a parameter row, a delay, outside the contract, naming the first value
//                               (gab_plan.hpp's check kernel).
//   reverb_check_delays_kernel  the same for a set of delays.
//
// The sequence of roundings per sample is the header's; the cut decides only where a value is held, so every launch
// form, alignment and track count gives the same bits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kRevChains = 64;            // chains (track, line) of a workgroup: the lanes of the serial phase
constexpr int kRevChunk = 64;             // the longest chunk: the lanes of the phases along time
constexpr int kRevPitch = 68;             // row pitch in floats: 16-byte aligned rows, conflict-free b128 access (kEqPitch)
constexpr int kRevMaxLog2 = 20;           // max_delay <= 2^20 samples, as gab_delay_create

// A hand-off through LDS inside the wave (k_delay.hip's): words that some lanes wrote or read are touched by other
// lanes next.
__device__ __forceinline__ void rev_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The value lane `from` holds, for every lane (from is the same in all of them).
__device__ __forceinline__ float rev_of(float v, int from) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), from));
}
__device__ __forceinline__ unsigned rev_of(unsigned v, int from) {
    return (unsigned)__builtin_amdgcn_readlane((int)v, from);
}

// A field of one chain: the target t, the current c and d = t - c (rounded once).  On a ramp buffer the value of a
// sample is fmaf(d, r, c), else t.
struct RevField {
    float t, c, d;
};
template <bool RAMPING>
__device__ __forceinline__ float rev_value(const RevField& f, int from, float r) {
    if constexpr (RAMPING) return fmaf(rev_of(f.d, from), r, rev_of(f.c, from));
    return rev_of(f.t, from);
}

// What a wave carries through a launch.  Lane l is chain l: track l / N of the wave, line l % N.  A lane below the last
// chain holds zeros and the delay of the last chain; nothing it computes is stored.
struct RevWave {
    float* tile;                // [64][kRevPitch]: v, then q
    float* rl;                  // [64]: the chunk's ramp values (RAMPING)
    int lane, nt, nch;          // tracks and chains this wave owns
    RevField g, damp, b, c[2], dry;
    float q;                    // the low-pass state
    unsigned P;                 // the ring index of the track's next sample
    int m;                      // the line's delay
};

// One buffer.  x: the row of this wave's first track, y: of its first output, lines: of its first chain; ramp: the
// table [B]; C: the chunk.
template <int N, int O, bool RAMPING>
__device__ __forceinline__ void rev_buffer(RevWave& w, const float* x, float* y, float* lines,
                                           const float* __restrict__ ramp, int B, int C, unsigned mask) {
    constexpr int G = kRevChains / N;
    const int lane = w.lane;
    const size_t cap = (size_t)mask + 1;
    float* tile = w.tile;
    for (int s0 = 0; s0 < B; s0 += C) {
        const int len = B - s0 < C ? B - s0 : C;
        const int js = lane < len ? lane : 0;                         // a lane behind the chunk reads its first sample
        float r = 1.0f;
        if constexpr (RAMPING) {
            r = ramp[s0 + js];
            w.rl[lane] = r;
        }
        // ---- 1. the chunk's line words and its input into registers ----
        // Every load is unconditional, so that all of them are in flight before the first is used: a chain below the
        // last reads the last chain's words, a lane behind the chunk a masked (so valid) older or newer word.  Such a
        // value is never stored and never enters a recurrence that is.
        float v[kRevChains], xr[G];
#pragma unroll
        for (int c = 0; c < kRevChains; ++c) {
            const int cc = c < w.nch ? c : w.nch - 1;
            const unsigned at = (rev_of(w.P, cc) + (unsigned)lane - (unsigned)rev_of((unsigned)w.m, cc)) & mask;
            v[c] = lines[(size_t)cc * cap + at];
        }
#pragma unroll
        for (int tl = 0; tl < G; ++tl) xr[tl] = x[(size_t)(tl < w.nt ? tl : w.nt - 1) * B + s0 + js];
#pragma unroll
        for (int c = 0; c < kRevChains; ++c)
            tile[c * kRevPitch + lane] = __fmul_rn(rev_value<RAMPING>(w.g, c, r), v[c]);
        rev_wave_order();
        // ---- 2. the low-pass, a lane per chain, in order ----
        {
            float4* row = reinterpret_cast<float4*>(tile + lane * kRevPitch);
            float q = w.q;
            for (int i = 0; 4 * i < len; ++i) {
                const float4 vv = row[i];
                float vs[4] = {vv.x, vv.y, vv.z, vv.w};
                float rs[4] = {1.0f, 1.0f, 1.0f, 1.0f};
                if constexpr (RAMPING) {
                    const float4 rv = *reinterpret_cast<const float4*>(w.rl + 4 * i);
                    rs[0] = rv.x; rs[1] = rv.y; rs[2] = rv.z; rs[3] = rv.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * i + j < len) {                           // wave-uniform: the recurrence never runs on padding
                        const float damp = RAMPING ? fmaf(w.damp.d, rs[j], w.damp.c) : w.damp.t;
                        q = fmaf(damp, __fsub_rn(q, vs[j]), vs[j]);
                        vs[j] = q;
                    }
                }
                row[i] = make_float4(vs[0], vs[1], vs[2], vs[3]);
            }
            w.q = q;
        }
        rev_wave_order();
        // ---- 3. the mixing matrix, the lines' new words and the outputs ----
#pragma unroll
        for (int tl = 0; tl < G; ++tl) {
            if (tl < w.nt) {                                         // wave-uniform
                float q[N], u[N];
#pragma unroll
                for (int i = 0; i < N; ++i) u[i] = q[i] = tile[(tl * N + i) * kRevPitch + lane];
#pragma unroll
                for (int h = 1; h < N; h *= 2) {
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if ((k & h) == 0) {
                            const float a = u[k], bb = u[k + h];
                            u[k] = __fadd_rn(a, bb);
                            u[k + h] = __fsub_rn(a, bb);
                        }
                    }
                }
                const float xv = xr[tl];
                const unsigned at = (rev_of(w.P, tl * N) + (unsigned)lane) & mask;
                float nw[N], acc[O];
#pragma unroll
                for (int i = 0; i < N; ++i) nw[i] = fmaf(rev_value<RAMPING>(w.b, tl * N + i, r), xv, u[i]);
                const float dry = rev_value<RAMPING>(w.dry, tl * N, r);
#pragma unroll
                for (int o = 0; o < O; ++o) {
                    acc[o] = __fmul_rn(dry, xv);
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[o] = fmaf(rev_value<RAMPING>(w.c[o], tl * N + i, r), q[i], acc[o]);
                }
                if (lane < len) {
#pragma unroll
                    for (int i = 0; i < N; ++i) lines[(size_t)(tl * N + i) * cap + at] = nw[i];
#pragma unroll
                    for (int o = 0; o < O; ++o) y[(size_t)(tl * O + o) * B + s0 + lane] = acc[o];
                }
            }
        }
        w.P = (w.P + (unsigned)len) & mask;
        // A later chunk of this launch reads, with other lanes, line words stored just now (a delay shorter than the
        // launch).  LLVM's AMDGPU memory model (gfx90a / gfx942 / gfx950 code sequences) makes global memory coherent
        // at wavefront and workgroup scope without any cache invalidate when the code object is not in tgsplit mode: the
        // wave's accesses go through its compute unit's one vector L1, which serves them in order.  The
        // workgroup-scope release / acquire pair is the fence that model asks for and keeps the compiler from moving a
        // load above the stores; this file is built in the default, non-tgsplit mode.  The wait is stricter than the
        // model: the stores have left before a load goes (k_delay.hip).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        rev_wave_order();                                            // the tile and rl are free for the next chunk
    }
}

// Grid: x = group of 64 / N tracks, one wave.  in: [n][T][B]; out: [n][T * O][B], may be in when O == 1 (a chunk's
// input is in registers before its output is written, by the same wave).  lines: [T][N][cap], cap = mask + 1 a power of
// two >= max_delay + 64; pos: [T]; qstate, delays: [T][N]; cur, tgt: [T][N (3 + O) + 1].  RAMP: the launch's first
// buffer runs the ramp from cur to tgt; every other buffer takes tgt.
template <int N, int O, bool RAMP>
__global__ __launch_bounds__(kRevChains) void reverb_kernel(const float* in, float* out, float* lines, unsigned* pos,
                                                            float* qstate, const int* __restrict__ delays,
                                                            const float* __restrict__ cur,
                                                            const float* __restrict__ tgt,
                                                            const float* __restrict__ ramp, int T, int B,
                                                            int n_buffers, unsigned mask) {
    constexpr int G = kRevChains / N;
    constexpr int ROW = N * (3 + O) + 1;
    __shared__ __attribute__((aligned(16))) float tile[kRevChains * kRevPitch];
    __shared__ __attribute__((aligned(16))) float rl[RAMP ? kRevChunk : 4];
    const int lane = threadIdx.x;
    const int t0 = blockIdx.x * G;
    RevWave w;
    w.tile = tile; w.rl = rl; w.lane = lane;
    w.nt = T - t0 < G ? T - t0 : G;
    w.nch = w.nt * N;
    const bool owner = lane < w.nch;
    const int line = lane % N;
    const size_t track = (size_t)t0 + (owner ? lane / N : w.nt - 1);
    const size_t chain = track * N + (owner ? line : N - 1);         // a lane below the last chain: the last chain's

    auto field = [&](int at, RevField& f) {
        f.t = owner ? tgt[track * ROW + at] : 0.0f;
        f.c = f.t;
        if constexpr (RAMP) f.c = owner ? cur[track * ROW + at] : 0.0f;
        f.d = __fsub_rn(f.t, f.c);
    };
    field(line, w.g);
    field(N + line, w.damp);
    field(2 * N + line, w.b);
    field(3 * N + line, w.c[0]);
    if constexpr (O == 2) field(4 * N + line, w.c[1]); else w.c[1] = w.c[0];
    field(ROW - 1, w.dry);
    w.q = owner ? qstate[chain] : 0.0f;
    w.P = pos[track] & mask;
    w.m = delays[chain];

    // the chunk: the smallest delay among this wave's chains, 64 at the most
    int mmin = w.m;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int o = __shfl_xor(mmin, d, 64);
        mmin = o < mmin ? o : mmin;
    }
    mmin = __builtin_amdgcn_readfirstlane(mmin);
    const int C = mmin < 1 ? 1 : (mmin < kRevChunk ? mmin : kRevChunk);   // the tables hold delays >= 32: a guard

    const size_t in_block = (size_t)T * B, out_block = in_block * O;
    const float* x = in + (size_t)t0 * B;
    float* y = out + (size_t)t0 * O * B;
    float* ln = lines + (size_t)t0 * N * ((size_t)mask + 1);
    int nb = 0;
    if constexpr (RAMP) {
        rev_buffer<N, O, true>(w, x, y, ln, ramp, B, C, mask);
        nb = 1;
    }
    for (; nb < n_buffers; ++nb) rev_buffer<N, O, false>(w, x + nb * in_block, y + nb * out_block, ln, ramp, B, C, mask);
    if (owner) {
        qstate[chain] = w.q;
        if (line == 0) pos[track] = w.P;
    }
}

// src: [n_rows][row]
struct ReverbRule {
    int row, lines;
    float gmax;
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i % (size_t)row);
        bool bad = not_finite(__float_as_uint(v));
        if (field < lines) bad = bad || !(fabsf(v) <= gmax);
        else if (field < 2 * lines) bad = bad || !(v >= 0.0f && v <= 0x1.ffffep-1f);
        return bad;
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % (unsigned)row), N = lines;
        const char* name = field < N ? "g" : (field < 2 * N ? "damp" : (field < 3 * N ? "b" : (field < row - 1 ? "c" : "dry")));
        const char* rule = field < N ? "must be finite and at most gab_reverb_gmax(lines) in magnitude"
                                     : (field < 2 * N ? "must be within [0, 1 - 2^-20]" : "must be finite");
        return row_refusal(i, (unsigned)row, first_track, name, rule);
    }
};

// src: [n_rows][lines]
struct ReverbDelayRule {
    int lo, hi;
    unsigned lines;                 // for the text only
    __device__ bool refuses(const int* src, size_t i) const {
        const int v = src[i];
        return v < lo || v > hi;
    }
    std::string refusal(unsigned i, int first_track) const {
        return "track " + std::to_string(first_track + (int)(i / lines)) + " line " + std::to_string((int)(i % lines)) +
               " must be within [GAB_REVERB_MIN_DELAY, max_delay]; the plan keeps its delays";
    }
};

}  // namespace
}  // namespace gab

struct gab_reverb_plan {
    int tracks = 0, bufsize = 0, lines = 0, outs = 0, max_delay = 0, row = 0;
    size_t capacity = 0;               // floats of a line's ring: a power of two >= max_delay + 64
    gab::RampedTable params;           // current, target: [T][row]
    gab::DeviceBuf<float> ring;        // [T][N][capacity]
    gab::DeviceBuf<unsigned> pos;      // [T]: the ring index of the next sample
    gab::DeviceBuf<float> q;           // [T][N]: the low-pass states
    gab::DeviceBuf<int> delays;        // [T][N]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

bool reverb_lines_ok(int lines) { return lines == 4 || lines == 8 || lines == 16; }

float reverb_gmax(int lines) {
    return lines == 4 ? GAB_REVERB_GMAX_4 : (lines == 8 ? GAB_REVERB_GMAX_8 : (lines == 16 ? GAB_REVERB_GMAX_16 : 0.0f));
}

// n buffers in one launch; then, if a ramp ran through the first of them, current := target.  Nothing is allocated and
// nothing waits here.
int reverb_process(gab_reverb_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    if (p->outs != 1 && (const float*)d_out == d_in) return refuse(who, "d_out == d_in needs outs == 1");
    const int per_wave = kRevChains / p->lines;
    const dim3 grid((unsigned)((p->tracks + per_wave - 1) / per_wave));
    const unsigned mask = (unsigned)(p->capacity - 1);
    const bool ramp = p->params.pending;
#define GAB_REVERB(NN, OO, RR)                                                                                      \
    reverb_kernel<NN, OO, RR><<<grid, kRevChains, 0, s>>>(                                                          \
        d_in, d_out, p->ring.get(), p->pos.get(), p->q.get(), p->delays.get(), p->params.current.get(),            \
        p->params.target.get(), p->params.ramp.get(), p->tracks, p->bufsize, n_buffers, mask)
#define GAB_REVERB_N(NN)                                                                                            \
    do {                                                                                                            \
        if (p->outs == 1) { if (ramp) GAB_REVERB(NN, 1, true); else GAB_REVERB(NN, 1, false); }                     \
        else              { if (ramp) GAB_REVERB(NN, 2, true); else GAB_REVERB(NN, 2, false); }                     \
    } while (0)
    if (p->lines == 4) GAB_REVERB_N(4);
    else if (p->lines == 8) GAB_REVERB_N(8);
    else GAB_REVERB_N(16);
#undef GAB_REVERB_N
#undef GAB_REVERB
    if (int rc = launch_status("reverb_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int reverb_set_range(gab_reverb_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                     hipStream_t s) {
    const size_t row = (size_t)p->row, n = (size_t)n_tracks * row;
    return check_then(p->flag, s, who, d_params, n, ReverbRule{p->row, p->lines, reverb_gmax(p->lines)}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * row, n, ramp != 0, s); });
}

int reverb_set_delay_range(gab_reverb_plan* p, const int* d_delays, int first_track, int n_tracks, const char* who,
                           hipStream_t s) {
    const size_t N = (size_t)p->lines, n = (size_t)n_tracks * N;
    return check_then(p->flag, s, who, d_delays, n, ReverbDelayRule{GAB_REVERB_MIN_DELAY, p->max_delay, (unsigned)N},
                      first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->delays.get() + (size_t)first_track * N, d_delays, n * sizeof(int),
                                     hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_reverb_row_floats(int lines, int outs) {
    if (!gab::reverb_lines_ok(lines) || (outs != 1 && outs != 2)) return 0;
    return lines * (3 + outs) + 1;
}

float gab_reverb_gmax(int lines) { return gab::reverb_gmax(lines); }

int gab_reverb_create(gab_reverb_plan** out, int tracks, int bufsize, int lines, int outs, int max_delay) {
    return gab::create_entry("gab_reverb_create", out, tracks, bufsize, [&] {
        if (!gab::reverb_lines_ok(lines)) return gab::bad_arg("gab_reverb_create: lines must be 4, 8 or 16");
        if (outs != 1 && outs != 2) return gab::bad_arg("gab_reverb_create: outs must be 1 or 2");
        if (max_delay < GAB_REVERB_MIN_DELAY || max_delay > (1 << gab::kRevMaxLog2))
            return gab::bad_arg("gab_reverb_create: max_delay must be GAB_REVERB_MIN_DELAY..2^20");
        return GAB_OK;
    }, [&](gab_reverb_plan& p) {
        p.lines = lines; p.outs = outs; p.max_delay = max_delay;
        p.row = lines * (3 + outs) + 1;
        p.capacity = gab::ring_capacity((size_t)max_delay + gab::kRevChunk);
        const size_t chains = (size_t)tracks * (size_t)lines;
        p.params.create((size_t)tracks * (size_t)p.row, bufsize);
        p.ring.alloc(chains * p.capacity);
        p.pos.alloc((size_t)tracks);
        p.q.alloc(chains);
        p.delays.alloc(chains);
        p.flag.alloc(1);
        // pass-through: dry = 1, everything else 0, every delay max_delay, empty lines
        std::vector<float> init((size_t)p.row, 0.0f);
        init.back() = 1.0f;
        p.params.fill(init, tracks);
        p.delays.fill(max_delay);
        GAB_HIP_CHECK(hipMemset(p.ring.get(), 0, chains * p.capacity * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.pos.get(), 0, (size_t)tracks * sizeof(unsigned)));
        GAB_HIP_CHECK(hipMemset(p.q.get(), 0, chains * sizeof(float)));
        return GAB_OK;
    });
}

int gab_reverb_destroy(gab_reverb_plan* plan) { return gab::destroy_plan(plan, "gab_reverb_destroy: null pointer"); }

int gab_reverb_set_params(gab_reverb_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_reverb_set_params", gab::reverb_set_range, plan, d_params, true, 0, 0, ramp,
                          gab::as_stream(stream));
}

int gab_reverb_set_params_tracks(gab_reverb_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                                 gab_stream_t stream) {
    return gab::set_entry("gab_reverb_set_params_tracks", gab::reverb_set_range, plan, d_params, false, first_track,
                          n_tracks, ramp, gab::as_stream(stream));
}

int gab_reverb_set_delays(gab_reverb_plan* plan, const int* d_delays, gab_stream_t stream) {
    return gab::set_entry("gab_reverb_set_delays", gab::reverb_set_delay_range, plan, d_delays, true, 0, 0,
                          gab::as_stream(stream));
}

int gab_reverb_set_delays_tracks(gab_reverb_plan* plan, const int* d_delays, int first_track, int n_tracks,
                                 gab_stream_t stream) {
    return gab::set_entry("gab_reverb_set_delays_tracks", gab::reverb_set_delay_range, plan, d_delays, false, first_track,
                          n_tracks, gab::as_stream(stream));
}

int gab_reverb_reset(gab_reverb_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_reverb_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->ring.get(), 0, plan->ring.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->pos.get(), 0, plan->pos.size() * sizeof(unsigned), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->q.get(), 0, plan->q.size() * sizeof(float), s));
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_reverb_process(gab_reverb_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_reverb_process", {plan, d_in, d_out}, [&] {
        return gab::reverb_process(plan, d_in, d_out, 1, gab::as_stream(stream), "gab_reverb_process");
    });
}

int gab_reverb_process_batch(gab_reverb_plan* plan, const float* d_in, float* d_out, int n_buffers,
                             gab_stream_t stream) {
    return gab::batch_entry("gab_reverb_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::reverb_process(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_reverb_process_batch");
    });
}

int gab_reverb_params(gab_reverb_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_reverb_params", plan, &gab_reverb_plan::params, d_current, d_target, n_floats);
}

int gab_reverb_state(gab_reverb_plan* plan, float** d_lines, size_t* capacity, unsigned** d_pos, float** d_q,
                     int** d_delays) {
    return gab::entry("gab_reverb_state", {plan, d_lines, capacity, d_pos, d_q, d_delays}, [&] {
        *d_lines = plan->ring.get();
        *capacity = plan->capacity;
        *d_pos = plan->pos.get();
        *d_q = plan->q.get();
        *d_delays = plan->delays.get();
        return GAB_OK;
    });
}

}  // extern "C"
