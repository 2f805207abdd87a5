// k_nlms.hip — the adaptive-filter plan: a normalised-LMS filter per track (an echo canceller; with the step at 0 an
// FIR filter with its own taps per track).  L = 64 R taps, R in {1, 2, 4, 8}; parameters {mu, eps}, ramped over one
// buffer; the taps and the last L - 1 reference samples are carried on the device (include/gab_c_api.h, gab_nlms_*).
// No counterpart in the reference.
//
//   nlms_kernel<R, RAMP>   one wave per track, four waves a workgroup, no workgroup barrier, no atomics, no LDS.  Lane l
//                          holds taps w[64 q + l] and window X[64 q + l] = x[n - 64 q - l] in R registers each, for the
//                          whole launch: a batch moves the state once.  The stream is walked in chunks of 64 samples,
//                          one dword per lane (so alignment does not matter); per sample, in order:
//                            1. x[n], d[n] (and with RAMP mu, eps) are read from the chunk's lane n (v_readlane);
//                            2. the window moves up one tap: every register is rotated by one lane (wave_ror:1, one
//                               DPP move), lane 0 then takes the rotated lane 0 of the register below (one select), and
//                               lane 0 of register 0 the new sample;
//                            3. the two chains per lane, w X and X X, a product and R - 1 fmaf each;
//                            4. the two trees over the lanes in natural order, adjacent pairs first: lanes ^1 and ^2
//                               by quad_perm, ^4 by row_half_mirror, ^8 by row_mirror (every lane of a group holds
//                               the group's sum, and an addition commutes, so the mirrored partner gives the same
//                               bits), rows by row_bcast:15 and row_bcast:31; the root is lane 63's;
//                            5. e = d - y, s = mu / (P + eps) (the IEEE division), g = s e, all uniform;
//                            6. unless g is an infinity or a NaN: w = fmaf(g, X, w), R per lane;
//                            7. e and y go into lane n of the chunk's two output registers (one compare, two selects).
//                          A chunk's loads all come before its stores, and another wave never touches this track:
//                          err may be d_in and est may be d_ref.  Why rotate and select (and not wave_shr:1 with a
//                          carry through v_readlane), and what the launch costs: DESIGN.md §4q.
//   NlmsRule, NlmsTapRule  refuse a parameter row, a tap, outside the contract, naming the first (gab_plan.hpp's check
//                          kernel).
//
// The sequence of roundings per sample is the header's; the cut decides only where a value is held, so every launch
// form, buffer size, alignment and track count gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kNlmsWaves = 4;             // waves, and tracks, of a workgroup
constexpr int kNlmsChunk = 64;            // samples of a chunk: a dword per lane

// DPP controls (whole rows and banks, bound_ctrl off)
constexpr int kDppXor1 = 0xB1;            // quad_perm:[1,0,3,2]
constexpr int kDppXor2 = 0x4E;            // quad_perm:[2,3,0,1]
constexpr int kDppHalfMirror = 0x141;     // lane i of a half row takes lane 7 - i
constexpr int kDppMirror = 0x140;         // lane i of a row takes lane 15 - i
constexpr int kDppBcast15 = 0x142;        // lane 15 of a row to the next row
constexpr int kDppBcast31 = 0x143;        // lane 31 to rows 2 and 3
constexpr int kDppRor1 = 0x13C;           // wave_ror:1: lane l takes lane l - 1, lane 0 takes lane 63

// The value the control's source lane holds; a lane without a source (the first row under row_bcast:15, the first two
// under row_bcast:31) holds anything, and nothing reads it.
template <int CTRL>
__device__ __forceinline__ float nlms_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float nlms_lane(float v, int lane) {       // lane: the same in every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// The balanced tree over the 64 lanes in natural order, (2i, 2i + 1) first; the root, for every lane.  Below the rows
// every lane of a group holds its group's sum; across rows only the last lane of rows 1 and 3, then lane 63, do.
__device__ __forceinline__ float nlms_tree(float v) {
    v = __fadd_rn(v, nlms_dpp<kDppXor1>(v));
    v = __fadd_rn(v, nlms_dpp<kDppXor2>(v));
    v = __fadd_rn(v, nlms_dpp<kDppHalfMirror>(v));
    v = __fadd_rn(v, nlms_dpp<kDppMirror>(v));
    v = __fadd_rn(nlms_dpp<kDppBcast15>(v), v);                       // rows 1 and 3: the row before + this one
    v = __fadd_rn(nlms_dpp<kDppBcast31>(v), v);                       // row 3: rows 0..1 + rows 2..3
    return nlms_lane(v, 63);
}

__device__ __forceinline__ float nlms_ramp(float cur, float tgt, float r) { return fmaf(__fsub_rn(tgt, cur), r, cur); }

// Grid: x = group of four tracks, a wave each.  in / ref / err / est: [n][T][B]; err may be in, est may be ref, one of
// err and est may be null.  taps: [T][64 R]; hist: [T][64 R - 1], oldest first.  cur, tgt: [T][2].  RAMP: the launch's
// first buffer runs the ramp from cur to tgt; every other buffer takes tgt.
template <int R, bool RAMP>
__global__ __launch_bounds__(kNlmsWaves * 64) void nlms_kernel(const float* in, const float* ref, float* err, float* est,
                                                               float* __restrict__ taps, float* __restrict__ hist,
                                                               const float* __restrict__ cur,
                                                               const float* __restrict__ tgt,
                                                               const float* __restrict__ ramp, int T, int B,
                                                               int n_buffers) {
    constexpr int L = 64 * R;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * kNlmsWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= T) return;                                              // no workgroup barrier anywhere below
    float* const wt = taps + (size_t)t * L;
    float* const ht = hist + (size_t)t * (L - 1);
    float w[R], X[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int k = 64 * q + lane;
        w[q] = wt[k];
        X[q] = k < L - 1 ? ht[L - 2 - k] : 0.0f;                     // X[k] = the sample k + 1 before the next one
    }
    const float mu_t = tgt[2 * (size_t)t], eps_t = tgt[2 * (size_t)t + 1];
    float mu_c = mu_t, eps_c = eps_t;
    if constexpr (RAMP) {
        mu_c = cur[2 * (size_t)t];
        eps_c = cur[2 * (size_t)t + 1];
    }
    const bool first = lane == 0;
    const size_t block = (size_t)T * B;
    for (int nb = 0; nb < n_buffers; ++nb) {
        const size_t row = nb * block + (size_t)t * B;
        const bool ramping = RAMP && nb == 0;
        for (int s0 = 0; s0 < B; s0 += kNlmsChunk) {
            const int len = B - s0 < kNlmsChunk ? B - s0 : kNlmsChunk;
            const bool live = lane < len;
            // ---- the chunk's loads, all of them before any of its stores ----
            const float xc = live ? ref[row + s0 + lane] : 0.0f;
            const float dc = live ? in[row + s0 + lane] : 0.0f;
            float muc = mu_t, epsc = eps_t;
            if constexpr (RAMP) {
                if (ramping) {
                    const float r = live ? ramp[s0 + lane] : 1.0f;
                    muc = nlms_ramp(mu_c, mu_t, r);
                    epsc = nlms_ramp(eps_c, eps_t, r);
                }
            }
            float ec = 0.0f, yc = 0.0f;
            for (int j = 0; j < len; ++j) {
                const float xn = nlms_lane(xc, j), dn = nlms_lane(dc, j);
                const float mu = RAMP ? nlms_lane(muc, j) : mu_t, eps = RAMP ? nlms_lane(epsc, j) : eps_t;
                // ---- the window moves up one tap ----
                float rot[R];
#pragma unroll
                for (int q = 0; q < R; ++q) rot[q] = nlms_dpp<kDppRor1>(X[q]);
#pragma unroll
                for (int q = R - 1; q > 0; --q) X[q] = first ? rot[q - 1] : rot[q];
                X[0] = first ? xn : rot[0];
                // ---- the chains and the trees ----
                float ay = __fmul_rn(w[0], X[0]), ap = __fmul_rn(X[0], X[0]);
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    ay = fmaf(w[q], X[q], ay);
                    ap = fmaf(X[q], X[q], ap);
                }
                const float y = nlms_tree(ay), P = nlms_tree(ap);
                // ---- the error and the step, the same in every lane ----
                const float e = __fsub_rn(dn, y);
                const float den = __fadd_rn(P, eps);
                const float s = __fdiv_rn(mu, den);
                const float g = __fmul_rn(s, e);
                if (!not_finite(__builtin_amdgcn_readfirstlane(__float_as_uint(g)))) {
                    // R >= 4: a scalar branch around the update, not a select per register (the empty statement keeps it)
                    if constexpr (R >= 4) asm volatile("");
#pragma unroll
                    for (int q = 0; q < R; ++q) w[q] = fmaf(g, X[q], w[q]);
                }
                const bool mine = lane == j;
                ec = mine ? e : ec;
                yc = mine ? y : yc;
            }
            if (live) {
                if (err) err[row + s0 + lane] = ec;
                if (est) est[row + s0 + lane] = yc;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int k = 64 * q + lane;
        wt[k] = w[q];
        if (k < L - 1) ht[L - 2 - k] = X[q];
    }
}

const char* const kNlmsFields[GAB_NLMS_FIELDS] = {"mu", "eps"};
const char* const kNlmsRules[GAB_NLMS_FIELDS] = {"must be within [0, 2]", "must be within [2^-126, 2^64]"};

// src: [n_rows][2] (a NaN fails every comparison; -0.0 is a zero)
struct NlmsRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        if (not_finite(__float_as_uint(v))) return true;
        return (i % GAB_NLMS_FIELDS) == 0 ? !(v >= 0.0f && v <= 2.0f) : !(v >= 0x1p-126f && v <= 0x1p64f);
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % GAB_NLMS_FIELDS);
        return row_refusal(i, GAB_NLMS_FIELDS, first_track, kNlmsFields[field], kNlmsRules[field]);
    }
};

// src: [n_rows][L]
struct NlmsTapRule {
    unsigned L;
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int first_track) const {
        return "track " + std::to_string(first_track + (int)(i / L)) + " tap " + std::to_string((int)(i % L)) +
               " must be finite; the plan keeps its taps";
    }
};

}  // namespace
}  // namespace gab

struct gab_nlms_plan {
    int tracks = 0, bufsize = 0, taps = 0;
    gab::RampedTable params;           // current, target: [T][2]
    gab::DeviceBuf<float> w;           // [T][L]: the taps
    gab::DeviceBuf<float> hist;        // [T][L - 1]: the last L - 1 reference samples, oldest first
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch; then, if a ramp ran through the first of them, current := target.  Nothing is allocated and
// nothing waits here.
int nlms_process(gab_nlms_plan* p, const float* d_in, const float* d_ref, float* d_err, float* d_est, int n_buffers,
                 hipStream_t s, const char* who) {
    if (!d_err && !d_est) return refuse(who, "d_err and d_est may not both be null");
    const size_t n = (size_t)n_buffers * p->tracks * p->bufsize;
    if (d_err) {
        if (d_err != d_in && overlaps(d_err, d_in, n)) return refuse(who, "d_err may be d_in itself, but may not overlap it otherwise");
        if (overlaps(d_err, d_ref, n)) return refuse(who, "d_err may not overlap d_ref");
        if (d_est && overlaps(d_err, d_est, n)) return refuse(who, "d_err may not overlap d_est");
    }
    if (d_est) {
        if (d_est != d_ref && overlaps(d_est, d_ref, n)) return refuse(who, "d_est may be d_ref itself, but may not overlap it otherwise");
        if (overlaps(d_est, d_in, n)) return refuse(who, "d_est may not overlap d_in");
    }
    const dim3 grid((unsigned)((p->tracks + kNlmsWaves - 1) / kNlmsWaves));
    const bool ramp = p->params.pending;
#define GAB_NLMS(RR, RAMPED)                                                                                        \
    nlms_kernel<RR, RAMPED><<<grid, kNlmsWaves * 64, 0, s>>>(d_in, d_ref, d_err, d_est, p->w.get(), p->hist.get(),  \
                                                             p->params.current.get(), p->params.target.get(),       \
                                                             p->params.ramp.get(), p->tracks, p->bufsize, n_buffers)
#define GAB_NLMS_R(RR) do { if (ramp) GAB_NLMS(RR, true); else GAB_NLMS(RR, false); } while (0)
    switch (p->taps) {
        case 64: GAB_NLMS_R(1); break;
        case 128: GAB_NLMS_R(2); break;
        case 256: GAB_NLMS_R(4); break;
        default: GAB_NLMS_R(8); break;
    }
#undef GAB_NLMS_R
#undef GAB_NLMS
    if (int rc = launch_status("nlms_kernel")) return rc;
    if (ramp) p->params.snap(s);
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both tables and a pending ramp as they were.
int nlms_set_range(gab_nlms_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, int ramp,
                   hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_NLMS_FIELDS;
    return check_then(p->flag, s, who, d_params, n, NlmsRule{}, first_track,
                      [&] { p->params.commit(d_params, (size_t)first_track * GAB_NLMS_FIELDS, n, ramp != 0, s); });
}

// The taps of tracks [first_track, first_track + n_tracks): finite or refused; at once, the history stays.
int nlms_set_taps(gab_nlms_plan* p, const float* d_taps, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t L = (size_t)p->taps, n = (size_t)n_tracks * L;
    return check_then(p->flag, s, who, d_taps, n, NlmsTapRule{(unsigned)L}, first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->w.get() + (size_t)first_track * L, d_taps, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_nlms_create(gab_nlms_plan** out, int tracks, int bufsize, int taps) {
    return gab::create_entry("gab_nlms_create", out, tracks, bufsize, [&] {
        if (taps != 64 && taps != 128 && taps != 256 && taps != 512)
            return gab::bad_arg("gab_nlms_create: taps must be 64, 128, 256 or 512");
        return GAB_OK;
    }, [&](gab_nlms_plan& p) {
        p.taps = taps;
        p.params.create((size_t)tracks * GAB_NLMS_FIELDS, bufsize);
        p.w.alloc((size_t)tracks * taps);
        p.hist.alloc((size_t)tracks * (taps - 1));
        p.flag.alloc(1);
        // zero taps, no adaptation: est is +0 and err is d_in
        p.params.fill({0.0f, 1.0f}, tracks);
        p.w.fill(0.0f);
        p.hist.fill(0.0f);
        return GAB_OK;
    });
}

int gab_nlms_destroy(gab_nlms_plan* plan) { return gab::destroy_plan(plan, "gab_nlms_destroy: null pointer"); }

int gab_nlms_set_params(gab_nlms_plan* plan, const float* d_params, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_nlms_set_params", gab::nlms_set_range, plan, d_params, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_nlms_set_params_tracks(gab_nlms_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                               gab_stream_t stream) {
    return gab::set_entry("gab_nlms_set_params_tracks", gab::nlms_set_range, plan, d_params, false, first_track, n_tracks,
                          ramp, gab::as_stream(stream));
}

int gab_nlms_set_taps(gab_nlms_plan* plan, const float* d_taps, gab_stream_t stream) {
    return gab::set_entry("gab_nlms_set_taps", gab::nlms_set_taps, plan, d_taps, true, 0, 0, gab::as_stream(stream));
}

int gab_nlms_set_taps_tracks(gab_nlms_plan* plan, const float* d_taps, int first_track, int n_tracks, gab_stream_t stream) {
    return gab::set_entry("gab_nlms_set_taps_tracks", gab::nlms_set_taps, plan, d_taps, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_nlms_reset(gab_nlms_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_nlms_reset", {plan}, [&]() -> int {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->w.get(), 0, plan->w.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->hist.get(), 0, plan->hist.size() * sizeof(float), s));
        plan->params.snap(s);
        return GAB_OK;
    });
}

int gab_nlms_process(gab_nlms_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                     gab_stream_t stream) {
    return gab::entry("gab_nlms_process", {plan, d_in, d_ref}, [&] {
        return gab::nlms_process(plan, d_in, d_ref, d_err, d_est, 1, gab::as_stream(stream), "gab_nlms_process");
    });
}

int gab_nlms_process_batch(gab_nlms_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                           int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_nlms_process_batch", {plan, d_in, d_ref}, n_buffers, [&] {
        return gab::nlms_process(plan, d_in, d_ref, d_err, d_est, n_buffers, gab::as_stream(stream),
                                 "gab_nlms_process_batch");
    });
}

int gab_nlms_params(gab_nlms_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_nlms_params", plan, &gab_nlms_plan::params, d_current, d_target, n_floats);
}

int gab_nlms_state(gab_nlms_plan* plan, float** d_taps, float** d_history, int* taps) {
    return gab::entry("gab_nlms_state", {plan, d_taps, d_history, taps}, [&] {
        *d_taps = plan->w.get();
        *d_history = plan->hist.get();
        *taps = plan->taps;
        return GAB_OK;
    });
}

}  // extern "C"
