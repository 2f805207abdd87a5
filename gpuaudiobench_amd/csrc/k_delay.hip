// k_delay.hip — the delay plan: a delay line per track, read at a fractional position, with a feedback path and four
// parameters {delay, feedback, wet, dry} that can be ramped over one buffer (include/gab_c_api.h, gab_delay_*).
// No counterpart in the reference, whose waveguide has fixed integer lengths.
//
//   delay_kernel<LAG, RAMP>  a wave owns one track for the whole launch, every buffer of a batch included.  It walks the
//                            stream in segments of at most 512 samples.  A segment's input, its ramp values and the
//                            values w that enter the line lie in the wave's own LDS; values older than the segment come
//                            from the ring in memory.  Inside a segment the wave works in chunks of m samples (m - 1
//                            for Lagrange), m the smallest integer delay of the segment: a chunk's taps end before the
//                            chunk begins, so its lanes are independent; the chunks follow each other in order.
//                            m >= the segment: one chunk.  m = 1: one sample at a time.
//   DelayRule                refuses a parameter row outside the contract, naming the first (gab_plan.hpp's check
//                            kernel).
//
// The sequence of roundings per sample is the header's; nothing here re-associates.  What the cut decides is only where
// a value is fetched from, so every launch form gives the same bits.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kDelaySeg = 512;            // samples of a segment: three LDS rows of this many floats per wave
constexpr int kDelayWaves = 4;            // tracks (waves) per workgroup
constexpr int kDelayMaxLog2 = 20;         // max_delay <= 2^20 samples
constexpr float kSixth = (float)(1.0 / 6.0);

// A hand-off through LDS inside the wave: words that some lanes wrote are read by other lanes next.  The wait lets the
// writes complete before a later read is issued, the fence keeps the compiler from moving a read above them.
__device__ __forceinline__ void delay_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float delay_clamp(float d, float dmin, float dmax) { return fminf(fmaxf(d, dmin), dmax); }

// The parameters of one sample: p = fmaf(target - current, r, current) on a ramp buffer, else the target.
struct DelayTrack {
    float cd, cf, cw, cy;       // current
    float td, tf, tw, ty;       // target
    float dmin, dmax;
};
struct DelaySample {
    int i;                      // floor of the clamped delay
    float fr, fb, wet, dry;
};
__device__ __forceinline__ float delay_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }
__device__ __forceinline__ DelaySample delay_sample(const DelayTrack& t, bool ramping, float r) {
    float d = t.td;
    DelaySample q;
    q.fb = t.tf; q.wet = t.tw; q.dry = t.ty;
    if (ramping) {
        d = delay_ramp(t.cd, t.td, r);
        q.fb = delay_ramp(t.cf, t.tf, r);
        q.wet = delay_ramp(t.cw, t.tw, r);
        q.dry = delay_ramp(t.cy, t.ty, r);
    }
    d = delay_clamp(d, t.dmin, t.dmax);
    const float fl = floorf(d);
    q.i = (int)fl;
    q.fr = __fsub_rn(d, fl);                                         // exact
    return q;
}

// The tap: am, a, b, b2 = w[n-i+1], w[n-i], w[n-i-1], w[n-i-2] (linear: a and b only).
template <bool LAG>
__device__ __forceinline__ float delay_tap(float fr, float am, float a, float b, float b2) {
    if constexpr (LAG) {
        const float fm1 = __fsub_rn(fr, 1.0f), fm2 = __fsub_rn(fr, 2.0f), fp1 = __fadd_rn(fr, 1.0f);
        const float hm = __fmul_rn(__fmul_rn(__fmul_rn(fr, fm1), fm2), -kSixth);
        const float h0 = __fmul_rn(__fmul_rn(__fmul_rn(fp1, fm1), fm2), 0.5f);
        const float h1 = __fmul_rn(__fmul_rn(__fmul_rn(fp1, fr), fm2), -0.5f);
        const float h2 = __fmul_rn(__fmul_rn(__fmul_rn(fp1, fr), fm1), kSixth);
        float v = __fmul_rn(hm, am);
        v = fmaf(h1, b, v);
        v = fmaf(h2, b2, v);
        return fmaf(h0, a, v);
    } else {
        return fmaf(fr, __fsub_rn(b, a), a);
    }
}

// w[k], k relative to the segment's first sample: the segment's own values from LDS, older ones from the ring.  Two
// loads of two address spaces, each under its own condition (one load through a selected pointer would be a flat load).
__device__ __forceinline__ float delay_fetch(const float* wl, const float* line, unsigned P, unsigned mask, int k) {
    float g = 0.0f;
    if (k < 0) g = line[(P + (unsigned)k) & mask];
    const float l = wl[k < 0 ? 0 : k];
    return k < 0 ? g : l;
}

// Grid: x = group of kDelayWaves tracks.  in / out: [n][T][B], may be the same memory (a sample's input is read before
// its output is written, by the same wave).  ring: [T][cap], cap = mask + 1 a power of two; pos: [T], the ring index of
// the next sample.  RAMP: the launch's first buffer runs the ramp from cur to tgt; every other buffer takes tgt.
template <bool LAG, bool RAMP>
__global__ __launch_bounds__(kDelayWaves * 64) void delay_kernel(const float* in, float* out, float* ring,
                                                                unsigned* __restrict__ pos,
                                                                const float* __restrict__ cur,
                                                                const float* __restrict__ tgt,
                                                                const float* __restrict__ ramp, int T, int B,
                                                                int n_buffers, unsigned mask, float dmin, float dmax) {
    constexpr int U = kDelaySeg / 64;                                // samples of a segment per lane
    __shared__ float lds_xy[kDelayWaves][kDelaySeg];                 // x on the way in, y on the way out
    __shared__ float lds_w[kDelayWaves][kDelaySeg];                  // what enters the line
    __shared__ float lds_r[RAMP ? kDelayWaves : 1][RAMP ? kDelaySeg : 1];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * kDelayWaves + wv;
    if (t >= T) return;                                              // no workgroup barrier anywhere below
    float* xy = lds_xy[wv];
    float* wl = lds_w[wv];
    float* rl = lds_r[RAMP ? wv : 0];
    float* line = ring + (size_t)t * ((size_t)mask + 1);
    const float* tp = tgt + (size_t)t * 4;
    DelayTrack tr;
    tr.td = tp[0]; tr.tf = tp[1]; tr.tw = tp[2]; tr.ty = tp[3];
    tr.cd = tr.td; tr.cf = tr.tf; tr.cw = tr.tw; tr.cy = tr.ty;
    if constexpr (RAMP) {
        const float* cp = cur + (size_t)t * 4;
        tr.cd = cp[0]; tr.cf = cp[1]; tr.cw = cp[2]; tr.cy = cp[3];
    }
    tr.dmin = dmin; tr.dmax = dmax;
    unsigned P = pos[t] & mask;

    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x = in + ((size_t)nb * T + t) * B;
        float* y = out + ((size_t)nb * T + t) * B;
        const bool ramping = RAMP && nb == 0;
        for (int s0 = 0; s0 < B; s0 += kDelaySeg) {
            const int len = B - s0 < kDelaySeg ? B - s0 : kDelaySeg;
            {   // the segment's input (and ramp) into LDS, every load requested before the first is used
                float xr[U], rr[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = lane + 64 * u;
                    xr[u] = j < len ? x[s0 + j] : 0.0f;
                    rr[u] = (ramping && j < len) ? ramp[s0 + j] : 1.0f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = lane + 64 * u;
                    if (j < len) {
                        xy[j] = xr[u];
                        if constexpr (RAMP) rl[j] = rr[u];
                    }
                }
            }
            // m: the smallest integer delay of the segment.  The ramp is monotone in s and so are the clamp and the
            // floor: the smaller of the two ends.
            int m = delay_sample(tr, ramping, ramping ? ramp[s0] : 1.0f).i;
            const int m1 = delay_sample(tr, ramping, ramping ? ramp[s0 + len - 1] : 1.0f).i;
            m = __builtin_amdgcn_readfirstlane(m1 < m ? m1 : m);
            const int chunk = LAG ? m - 1 : m;                       // >= 1: min_delay is 2 for Lagrange, 1 for linear
            delay_wave_order();

            if (chunk >= len) {
                // one chunk: every tap is older than the segment and comes from the ring; all loads first
                float am[U], a[U], b[U], b2[U];
                DelaySample q[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = lane + 64 * u;
                    am[u] = a[u] = b[u] = b2[u] = 0.0f;
                    if (j < len) {
                        float r = 1.0f;
                        if constexpr (RAMP) r = rl[j];
                        q[u] = delay_sample(tr, ramping, r);
                        const unsigned k = P + (unsigned)(j - q[u].i);
                        a[u] = line[k & mask];
                        b[u] = line[(k - 1u) & mask];
                        if constexpr (LAG) {
                            am[u] = line[(k + 1u) & mask];
                            b2[u] = line[(k - 2u) & mask];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = lane + 64 * u;
                    if (j < len) {
                        const float xv = xy[j];
                        const float v = delay_tap<LAG>(q[u].fr, am[u], a[u], b[u], b2[u]);
                        wl[j] = fmaf(q[u].fb, v, xv);
                        xy[j] = fmaf(q[u].wet, v, __fmul_rn(q[u].dry, xv));
                    }
                }
                delay_wave_order();
            } else {
                for (int c0 = 0; c0 < len; c0 += chunk) {
                    const int c1 = len - c0 < chunk ? len : c0 + chunk;
                    for (int j = c0 + lane; j < c1; j += 64) {
                        const float xv = xy[j];
                        float r = 1.0f;
                        if constexpr (RAMP) r = rl[j];
                        const DelaySample q = delay_sample(tr, ramping, r);
                        const int k = j - q.i;                       // w[n - i], relative to the segment
                        const float a = delay_fetch(wl, line, P, mask, k);
                        const float b = delay_fetch(wl, line, P, mask, k - 1);
                        float am = 0.0f, b2 = 0.0f;
                        if constexpr (LAG) {
                            am = delay_fetch(wl, line, P, mask, k + 1);
                            b2 = delay_fetch(wl, line, P, mask, k - 2);
                        }
                        const float v = delay_tap<LAG>(q.fr, am, a, b, b2);
                        wl[j] = fmaf(q.fb, v, xv);
                        xy[j] = fmaf(q.wet, v, __fmul_rn(q.dry, xv));
                    }
                    delay_wave_order();
                }
            }

#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = lane + 64 * u;
                if (j < len) {
                    line[(P + (unsigned)j) & mask] = wl[j];
                    y[s0 + j] = xy[j];
                }
            }
            P = (P + (unsigned)len) & mask;
            // A later segment of this launch reads, with other lanes, ring words stored just now.  LLVM's AMDGPU memory
            // model (gfx90a / gfx942 / gfx950 code sequences) makes global memory coherent at wavefront and workgroup
            // scope without any cache invalidate when the code object is not in tgsplit mode: a workgroup's waves share
            // one compute unit and its one vector L1, which serves a wave's accesses in order.  The workgroup-scope
            // release / acquire pair is the fence that model asks for (under tgsplit the compiler itself would add the
            // invalidate to it) and keeps the compiler from moving a load above the stores; this file is built in the
            // default, non-tgsplit mode.  The wait is stricter than the model: the stores have left before a load goes.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            delay_wave_order();
        }
    }
    if (lane == 0) pos[t] = P;
}

const char* const kDelayFields[4] = {"delay", "feedback", "wet", "dry"};

// src: [n_rows][4]
struct DelayRule {
    float dmin, dmax;
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i & 3);
        bool bad = not_finite(__float_as_uint(v));
        if (field == 0) bad = bad || !(v >= dmin && v <= dmax);
        if (field == 1) bad = bad || !(fabsf(v) < 1.0f);
        return bad;
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i & 3u);
        const char* rule = field == 0 ? "must be finite and within [min_delay, max_delay]"
                                      : (field == 1 ? "must be finite and below 1 in magnitude" : "must be finite");
        return row_refusal(i, 4, first_track, kDelayFields[field], rule);
    }
};

}  // namespace
}  // namespace gab

struct gab_delay_plan {
    int tracks = 0, bufsize = 0, max_delay = 0, interp = 0, min_delay = 0;
    size_t capacity = 0;               // floats of a track's ring: a power of two >= max_delay + 3 + bufsize
    gab::RampedTable params;           // current, target: [T][4]
    gab::DeviceBuf<float> ring;        // [T][capacity]
    gab::DeviceBuf<unsigned> pos;      // [T]: the ring index of the next sample
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch; then, if a ramp ran through the first of them, current := target.  Nothing is allocated and
// nothing waits here.
int delay_process(gab_delay_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s) {
    const dim3 grid((unsigned)((p->tracks + kDelayWaves - 1) / kDelayWaves));
    const unsigned mask = (unsigned)(p->capacity - 1);
    const float dmin = (float)p->min_delay, dmax = (float)p->max_delay;
    const bool ramp = p->params.pending;
#define GAB_DELAY(LL, RR)                                                                                           \
    delay_kernel<LL, RR><<<grid, kDelayWaves * 64, 0, s>>>(                                                        \
        d_in, d_out, p->ring.get(), p->pos.get(), p->params.current.get(), p->params.target.get(),                 \
        p->params.ramp.get(), p->tracks, p->bufsize, n_buffers, mask, dmin, dmax)
    if (p->interp == GAB_DELAY_LAGRANGE3) {
        if (ramp) GAB_DELAY(true, true); else GAB_DELAY(true, false);
    } else {
        if (ramp) GAB_DELAY(false, true); else GAB_DELAY(false, false);
    }
#undef GAB_DELAY
    if (int rc = launch_status("delay_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int delay_set_range(gab_delay_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                    hipStream_t s) {
    const size_t n = (size_t)n_tracks * 4;
    return check_then(p->flag, s, who, d_params, n, DelayRule{(float)p->min_delay, (float)p->max_delay}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * 4, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_delay_create(gab_delay_plan** out, int tracks, int bufsize, int max_delay, int interp) {
    const int min_delay = interp == GAB_DELAY_LAGRANGE3 ? 2 : 1;
    size_t cap = 0;
    return gab::create_entry("gab_delay_create", out, tracks, bufsize, [&] {
        if (interp != GAB_DELAY_LINEAR && interp != GAB_DELAY_LAGRANGE3)
            return gab::bad_arg("gab_delay_create: interp must be GAB_DELAY_LINEAR or GAB_DELAY_LAGRANGE3");
        if (max_delay < min_delay || max_delay > (1 << gab::kDelayMaxLog2))
            return gab::bad_arg("gab_delay_create: max_delay must be min_delay..2^20 (min_delay: 1 linear, 2 Lagrange)");
        cap = gab::ring_capacity((size_t)max_delay + 3 + (size_t)bufsize);
        if (cap > ((size_t)1 << 31)) return gab::bad_arg("gab_delay_create: bufsize is too large for a track's ring");
        return GAB_OK;
    }, [&](gab_delay_plan& p) {
        p.max_delay = max_delay; p.interp = interp; p.min_delay = min_delay; p.capacity = cap;
        p.params.create((size_t)tracks * 4, bufsize);
        p.ring.alloc((size_t)tracks * cap);
        p.pos.alloc((size_t)tracks);
        p.flag.alloc(1);
        // pass-through: {min_delay, 0, 0, 1} on every track, an empty line
        p.params.fill({(float)min_delay, 0.0f, 0.0f, 1.0f}, tracks);
        GAB_HIP_CHECK(hipMemset(p.ring.get(), 0, (size_t)tracks * cap * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.pos.get(), 0, (size_t)tracks * sizeof(unsigned)));
        return GAB_OK;
    });
}

int gab_delay_destroy(gab_delay_plan* plan) { return gab::destroy_plan(plan, "gab_delay_destroy: null pointer"); }

int gab_delay_set_params(gab_delay_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_delay_set_params", gab::delay_set_range, plan, d_params, true, 0, 0, ramp,
                          gab::as_stream(stream));
}

int gab_delay_set_params_tracks(gab_delay_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                                gab_stream_t stream) {
    return gab::set_entry("gab_delay_set_params_tracks", gab::delay_set_range, plan, d_params, false, first_track, n_tracks,
                          ramp, gab::as_stream(stream));
}

int gab_delay_reset(gab_delay_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_delay_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->ring.get(), 0, plan->ring.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->pos.get(), 0, plan->pos.size() * sizeof(unsigned), s));
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_delay_process(gab_delay_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_delay_process", {plan, d_in, d_out},
                      [&] { return gab::delay_process(plan, d_in, d_out, 1, gab::as_stream(stream)); });
}

int gab_delay_process_batch(gab_delay_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_delay_process_batch", {plan, d_in, d_out}, n_buffers,
                            [&] { return gab::delay_process(plan, d_in, d_out, n_buffers, gab::as_stream(stream)); });
}

int gab_delay_params(gab_delay_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_delay_params", plan, &gab_delay_plan::params, d_current, d_target, n_floats);
}

int gab_delay_line(gab_delay_plan* plan, float** d_ring, size_t* capacity, unsigned** d_pos) {
    return gab::entry("gab_delay_line", {plan, d_ring, capacity, d_pos}, [&] {
        *d_ring = plan->ring.get();
        *capacity = plan->capacity;
        *d_pos = plan->pos.get();
        return GAB_OK;
    });
}

}  // extern "C"
