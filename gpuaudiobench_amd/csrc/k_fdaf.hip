// k_fdaf.hip — the block adaptive-filter plan: a partitioned frequency-domain NLMS filter per track (the multidelay
// block filter, MDF): K partitions of 512 taps, L = 512 K up to 16 384 taps, adapted per bin once per block of 512
// samples, with the gradient constraint on one partition a block (include/gab_c_api.h, gab_fdaf_*).  Where the nlms
// plan (k_nlms.hip) ends at 512 taps and a serial recursion per sample, this one reaches a room's echo path and is
// bound by the traffic of its own state.  No counterpart in the reference.
//
//   fdaf_kernel        one launch a call or batch: one wave per pair of tracks (2q, 2q + 1), four waves a workgroup, no
//                      workgroup barrier, no atomics.  The wave owns its pair's state and walks the call's blocks in
//                      ascending order.  A lane keeps bins k = lane + 64 r (r < 9; r = 8 is bin 512, lane 0's) of both
//                      tracks, and every global word of W and X is read and written by the lane that owns its bin: the
//                      only hand-overs between lanes go through the wave's LDS image, behind stft::wave_sync.  Per block
//                      the header's seven steps:
//                        1. the window [prev | x_b] of the pair, from registers (prev) and one gather (x_b), through
//                           stft::spectra — what stft::analyse runs behind its gather, so the newest delay-line slot is
//                           the spectrum plan's row bit for bit.  stft::analyse itself is not called: it gathers the
//                           whole window from global memory, and d_est may be d_ref, so the block before this one
//                           may already hold estimates; and a window of ones is no product;
//                        2. one pass over the delay line and the partitions: Y and S, the newest slot from registers;
//                        3. stft::pack (the bins above 512 through the image), the inverse, est and e;
//                        4. the skip, a ballot over the pair's 1024 errors;
//                        5. E = stft::spectra of [0 | e];
//                        6. the second and last pass over the delay line: every W_p, stored by its own lane, the
//                           partition that step 7 takes kept in registers instead;
//                        7. the constraint on partition c: pack, inverse, the tail zeroed, stft::spectra, store.
//                      Five transforms a block whatever K is.  prev and count move once a launch.
//   fdaf_taps_kernel   set_taps: a wave per (track, partition): the spectrum of [h[512 p .. 512 p + 512) | 0], the track
//                      alone in the transform (its partner's half is zeros), so a track's W depends on its own taps
//                      whatever range the call names.
//   FdafRule, FdafTapRule   refuse a parameter row, a tap, outside the contract, naming the first.
//
// Output bits depend on the pair's samples, rows and state alone: not on bufsize, the cut into calls or batches, the
// alignment, or which plan holds the pair.  Registers, LDS, occupancy and what the launch costs: DESIGN.md §4r.
#include <hip/hip_runtime.h>

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

constexpr int kFdafBlock = stft::kN / 2;                  // 512: the block, and the taps of a partition
constexpr int kFdafMaxK = 32;

// The header's two products, written down once (every fmaf one rounding):
//   acc + a b        re = fmaf(a.re, b.re, fmaf(-a.im, b.im, acc.re))    im = fmaf(a.re, b.im, fmaf(a.im, b.re, acc.im))
//   acc + conj(a) b  re = fmaf(a.re, b.re, fmaf(a.im, b.im, acc.re))     im = fmaf(a.re, b.im, fmaf(-a.im, b.re, acc.im))
// which is what fft::cfma and fft::cfma_cj are, two packed instructions each.
__device__ __forceinline__ cf fdaf_mac(cf x, cf w, cf acc) { return fft::cfma(x, w, acc); }
__device__ __forceinline__ cf fdaf_step(cf x, cf g, cf w) { return fft::cfma_cj(x, g, w); }
__device__ __forceinline__ float fdaf_power(cf x, float s) { return fmaf(x.y, x.y, fmaf(x.x, x.x, s)); }

// Grid: x = group of four pairs.  in (d), ref (x), err, est: [n][T][B], B a multiple of 512; err may be in, est may be
// ref, one of err and est may be null.  W, X: [T][K][513] complex.  prev: [T][512].  count: [T].  params: [T][2].
__global__ __launch_bounds__(256) void fdaf_kernel(const float* in, const float* ref, float* err, float* est,
                                                   cf* __restrict__ W, cf* __restrict__ X, float* __restrict__ prev,
                                                   unsigned* __restrict__ count, const float* __restrict__ params,
                                                   const cf* __restrict__ tw, int T, int B, int n_buffers, int K) {
    __shared__ cf lds[4 * stft::kImg];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    const int q = (int)blockIdx.x * 4 + w;
    const int ta = 2 * q, tb = 2 * q + 1;
    if (ta >= T) return;                                   // whole wave; no workgroup barrier anywhere below
    const bool hasb = tb < T;                              // an odd last track: beside zero samples, zero taps and {0, 1}

    using FWD = fft::WaveFFT1024<false>;
    using INV = fft::WaveFFT1024<true>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);

    const size_t plane = (size_t)K * stft::kBins;
    cf* const Wa = W + (size_t)ta * plane;
    cf* const Wb = Wa + plane;
    cf* const Xa = X + (size_t)ta * plane;
    cf* const Xb = Xa + plane;
    const float mua = params[2 * (size_t)ta], epsa = params[2 * (size_t)ta + 1];
    const float mub = hasb ? params[2 * (size_t)tb] : 0.0f, epsb = hasb ? params[2 * (size_t)tb + 1] : 1.0f;
    const bool adapta = mua != 0.0f, adaptb = mub != 0.0f;  // a track whose mu is 0 never writes its W
    const unsigned count0 = (unsigned)__builtin_amdgcn_readfirstlane((int)count[ta]);
    int slot = (int)(count0 % (unsigned)K);                // block b's ring slot, and the partition step 7 takes
    float pa[8], pb[8];                                    // the block before: sample lane + 64 j
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        pa[j] = prev[(size_t)ta * kFdafBlock + lane + 64 * j];
        pb[j] = hasb ? prev[(size_t)tb * kFdafBlock + lane + 64 * j] : 0.0f;
    }
    const int per = B / kFdafBlock, blocks = n_buffers * per;
    for (int g = 0; g < blocks; ++g) {
        const int nb = g / per;
        const size_t rowa = ((size_t)nb * T + ta) * B + (size_t)(g - nb * per) * kFdafBlock + lane;
        const size_t rowb = rowa + B;
        // ---- 1. the window's spectra, and the delay line's newest slot ----
        cf z[16];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            z[j] = fft::mk(pa[j], pb[j]);
            pa[j] = ref[rowa + 64 * j];
            pb[j] = hasb ? ref[rowb + 64 * j] : 0.0f;
            z[j + 8] = fft::mk(pa[j], pb[j]);
        }
        cf xa[9], xb[9];
        stft::wave_sync();                                 // the image is free: the block before has its partners
        stft::spectra(z, img, t, lane, xa, xb);
        cf* const Xna = Xa + (size_t)slot * stft::kBins;
        cf* const Xnb = Xb + (size_t)slot * stft::kBins;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            if (k <= stft::kN / 2) {
                Xna[k] = xa[r];
                if (hasb) Xnb[k] = xb[r];
            }
        }
        // ---- 2. Y and S: p ascending, one chain per bin ----
        cf ya[9], yb[9];
        float sa[9], sb[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            ya[r] = yb[r] = fft::mk(0.0f, 0.0f);
            sa[r] = sb[r] = 0.0f;
            if (k <= stft::kN / 2) {
                const cf wa0 = Wa[k], wb0 = hasb ? Wb[k] : fft::mk(0.0f, 0.0f);
                ya[r] = fdaf_mac(xa[r], wa0, ya[r]);
                yb[r] = fdaf_mac(xb[r], wb0, yb[r]);
                sa[r] = fdaf_power(xa[r], sa[r]);
                sb[r] = fdaf_power(xb[r], sb[r]);
            }
        }
        for (int p = 1; p < K; ++p) {
            const int sp = slot - p < 0 ? slot - p + K : slot - p;
            const size_t ox = (size_t)sp * stft::kBins, ow = (size_t)p * stft::kBins;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int k = lane + 64 * r;
                if (k <= stft::kN / 2) {
                    const cf x0 = Xa[ox + k], w0 = Wa[ow + k];
                    const cf x1 = hasb ? Xb[ox + k] : fft::mk(0.0f, 0.0f), w1 = hasb ? Wb[ow + k] : fft::mk(0.0f, 0.0f);
                    ya[r] = fdaf_mac(x0, w0, ya[r]);
                    yb[r] = fdaf_mac(x1, w1, yb[r]);
                    sa[r] = fdaf_power(x0, sa[r]);
                    sb[r] = fdaf_power(x1, sb[r]);
                }
            }
        }
        // ---- 3. the estimate and the error ----
        stft::wave_sync();                                 // every lane has read its partners of step 1
        stft::pack_rows(ya, yb, img, lane, z);
        INV::run(z, img, t, lane);
        float ea[8], eb[8];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // (+0 added: a -0 out of a transform of zeros becomes +0, everything else is itself)
            const float esta = fmaf(z[j + 8].x, 0x1p-10f, 0.0f), estb = fmaf(z[j + 8].y, 0x1p-10f, 0.0f);
            ea[j] = __fsub_rn(in[rowa + 64 * j], esta);
            eb[j] = hasb ? __fsub_rn(in[rowb + 64 * j], estb) : __fsub_rn(0.0f, estb);
            bad = bad || not_finite(__float_as_uint(ea[j])) || not_finite(__float_as_uint(eb[j]));
            if (err) {
                err[rowa + 64 * j] = ea[j];
                if (hasb) err[rowb + 64 * j] = eb[j];
            }
            if (est) {
                est[rowa + 64 * j] = esta;
                if (hasb) est[rowb + 64 * j] = estb;
            }
        }
        // ---- 4. the skip: wave-uniform; and nothing to do where neither track adapts ----
        if (__builtin_amdgcn_ballot_w64(bad) == 0 && (adapta || adaptb)) {
            // ---- 5. E ----
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                z[j] = fft::mk(0.0f, 0.0f);
                z[j + 8] = fft::mk(ea[j], eb[j]);
            }
            cf ga[9], gb[9];
            stft::wave_sync();
            stft::spectra(z, img, t, lane, ga, gb);
            // ---- 6. G = s E, then every partition ----
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const float s0 = __fdiv_rn(mua, __fadd_rn(sa[r], epsa)), s1 = __fdiv_rn(mub, __fadd_rn(sb[r], epsb));
                ga[r] = fft::mk(__fmul_rn(s0, ga[r].x), __fmul_rn(s0, ga[r].y));
                gb[r] = fft::mk(__fmul_rn(s1, gb[r].x), __fmul_rn(s1, gb[r].y));
            }
            cf ca[9], cb[9];                               // partition c = slot, for step 7
#pragma unroll
            for (int r = 0; r < 9; ++r) ca[r] = cb[r] = fft::mk(0.0f, 0.0f);
            for (int p = 0; p < K; ++p) {
                const int sp = slot - p < 0 ? slot - p + K : slot - p;
                const size_t ox = (size_t)sp * stft::kBins, ow = (size_t)p * stft::kBins;
                const bool newest = p == 0, held = p == slot;
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    const int k = lane + 64 * r;
                    if (k <= stft::kN / 2) {
                        const cf x0 = newest ? xa[r] : Xa[ox + k];
                        const cf x1 = newest ? xb[r] : hasb ? Xb[ox + k] : fft::mk(0.0f, 0.0f);
                        const cf w0 = fdaf_step(x0, ga[r], Wa[ow + k]);
                        const cf w1 = fdaf_step(x1, gb[r], hasb ? Wb[ow + k] : fft::mk(0.0f, 0.0f));
                        if (held) {
                            ca[r] = w0;
                            cb[r] = w1;
                        } else {
                            if (adapta) Wa[ow + k] = w0;
                            if (adaptb) Wb[ow + k] = w1;
                        }
                    }
                }
            }
            // ---- 7. the constraint on partition c: its last 512 taps in time become +0 ----
            stft::wave_sync();                             // every lane has read its partners of step 5
            stft::pack_rows(ca, cb, img, lane, z);
            INV::run(z, img, t, lane);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                z[j] = fft::mk(__fmul_rn(z[j].x, 0x1p-10f), __fmul_rn(z[j].y, 0x1p-10f));
                z[j + 8] = fft::mk(0.0f, 0.0f);
            }
            stft::wave_sync();
            stft::spectra(z, img, t, lane, ca, cb);
            const size_t oc = (size_t)slot * stft::kBins;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int k = lane + 64 * r;
                if (k <= stft::kN / 2) {
                    if (adapta) Wa[oc + k] = ca[r];
                    if (adaptb) Wb[oc + k] = cb[r];
                }
            }
        }
        slot = slot + 1 == K ? 0 : slot + 1;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        prev[(size_t)ta * kFdafBlock + lane + 64 * j] = pa[j];
        if (hasb) prev[(size_t)tb * kFdafBlock + lane + 64 * j] = pb[j];
    }
    if (lane == 0) {
        count[ta] = count0 + (unsigned)blocks;
        if (hasb) count[tb] = count0 + (unsigned)blocks;
    }
}

// Grid: x = group of four (track, partition) of the range, a wave each.  taps: [n_tracks][512 K].  W: the plan's, the
// range's first track at first_track.
__global__ __launch_bounds__(256) void fdaf_taps_kernel(const float* __restrict__ taps, cf* __restrict__ W,
                                                        const cf* __restrict__ tw, int first_track, int n_tracks, int K) {
    __shared__ cf lds[4 * stft::kImg];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    const long long i = (long long)blockIdx.x * 4 + w;
    if (i >= (long long)n_tracks * K) return;              // whole wave; no workgroup barrier below
    const int ti = (int)(i / K), p = (int)(i - (long long)ti * K);
    using FWD = fft::WaveFFT1024<false>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);
    stft::tap_spectrum(taps + ((size_t)ti * K + p) * kFdafBlock, W + ((size_t)(first_track + ti) * K + p) * stft::kBins,
                       img, t, lane);
}

const char* const kFdafFields[GAB_FDAF_FIELDS] = {"mu", "eps"};
const char* const kFdafRules[GAB_FDAF_FIELDS] = {"must be within [0, 1]", "must be within [2^-126, 2^64]"};

// src: [n_rows][2] (a NaN fails every comparison; -0.0 is a zero)
struct FdafRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        if (not_finite(__float_as_uint(v))) return true;
        return (i % GAB_FDAF_FIELDS) == 0 ? !(v >= 0.0f && v <= 1.0f) : !(v >= 0x1p-126f && v <= 0x1p64f);
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % GAB_FDAF_FIELDS);
        return row_refusal(i, GAB_FDAF_FIELDS, first_track, kFdafFields[field], kFdafRules[field]);
    }
};

// src: [n_rows][L]
struct FdafTapRule {
    unsigned L;
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int first_track) const {
        return "track " + std::to_string(first_track + (int)(i / L)) + " tap " + std::to_string((int)(i % L)) +
               " must be finite; the plan keeps its taps";
    }
};

}  // namespace
}  // namespace gab

struct gab_fdaf_plan {
    int tracks = 0, bufsize = 0, partitions = 0;
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::DeviceBuf<float> params;      // [T][2]: {mu, eps}, unramped
    gab::DeviceBuf<float> W;           // [T][K][513][2]: the partitions' half-spectra
    gab::DeviceBuf<float> X;           // [T][K][513][2]: the delay line, block b in slot b mod K
    gab::DeviceBuf<float> prev;        // [T][512]: the reference block before
    gab::DeviceBuf<unsigned> count;    // [T]: blocks since the reset
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch.  Nothing is allocated and nothing waits here.
int fdaf_process(gab_fdaf_plan* p, const float* d_in, const float* d_ref, float* d_err, float* d_est, int n_buffers,
                 hipStream_t s, const char* who) {
    if (!d_err && !d_est) return refuse(who, "d_err and d_est may not both be null");
    if (int rc = stft::check_length(who, *p, n_buffers)) return rc;
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
    const unsigned groups = (unsigned)(((p->tracks + 1) / 2 + 3) / 4);
    fdaf_kernel<<<dim3(groups), 256, 0, s>>>(d_in, d_ref, d_err, d_est, reinterpret_cast<cf*>(p->W.get()),
                                             reinterpret_cast<cf*>(p->X.get()), p->prev.get(), p->count.get(),
                                             p->params.get(), p->tw, p->tracks, p->bufsize, n_buffers, p->partitions);
    return launch_status("fdaf_kernel");
}

// check, then commit (gab_plan.hpp): a refused set leaves the table as it was.  Unramped: in force from the next block.
int fdaf_set_range(gab_fdaf_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t n = (size_t)n_tracks * GAB_FDAF_FIELDS;
    return check_then(p->flag, s, who, d_params, n, FdafRule{}, first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->params.get() + (size_t)first_track * GAB_FDAF_FIELDS, d_params, n * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
}

// The taps of tracks [first_track, first_track + n_tracks), in time: finite or refused; then their partitions' spectra.
// The delay line, prev and count stay.
int fdaf_set_taps(gab_fdaf_plan* p, const float* d_taps, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t L = (size_t)p->partitions * kFdafBlock, n = (size_t)n_tracks * L;
    int rc_launch = GAB_OK;
    const int rc = check_then(p->flag, s, who, d_taps, n, FdafTapRule{(unsigned)L}, first_track, [&] {
        const long long waves = (long long)n_tracks * p->partitions;
        fdaf_taps_kernel<<<dim3((unsigned)((waves + 3) / 4)), 256, 0, s>>>(d_taps, reinterpret_cast<cf*>(p->W.get()), p->tw,
                                                                          first_track, n_tracks, p->partitions);
        rc_launch = launch_status("fdaf_taps_kernel");
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
    return rc ? rc : rc_launch;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_fdaf_create(gab_fdaf_plan** out, int tracks, int bufsize, int partitions) {
    return gab::create_entry("gab_fdaf_create", out, tracks, bufsize, [&] {
        if (bufsize % gab::kFdafBlock != 0) return gab::bad_arg("gab_fdaf_create: bufsize must be a multiple of 512");
        if (partitions < 1 || partitions > gab::kFdafMaxK) return gab::bad_arg("gab_fdaf_create: partitions must be 1..32");
        return GAB_OK;
    }, [&](gab_fdaf_plan& p) {
        p.partitions = partitions;
        p.tw = gab::fft::device_twiddles();
        const size_t spectra = (size_t)tracks * partitions * gab::stft::kBins * 2;
        p.params.alloc((size_t)tracks * GAB_FDAF_FIELDS);
        p.W.alloc(spectra);
        p.X.alloc(spectra);
        p.prev.alloc((size_t)tracks * gab::kFdafBlock);
        p.count.alloc((size_t)tracks);
        p.flag.alloc(1);
        // zero taps, no adaptation: est is +0 and err is d_in
        std::vector<float> rows((size_t)tracks * GAB_FDAF_FIELDS, 0.0f);
        for (int t = 0; t < tracks; ++t) rows[(size_t)t * GAB_FDAF_FIELDS + 1] = 1.0f;
        GAB_HIP_CHECK(hipMemcpy(p.params.get(), rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.W.get(), 0, spectra * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.X.get(), 0, spectra * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.prev.get(), 0, p.prev.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.count.get(), 0, p.count.size() * sizeof(unsigned)));
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_fdaf_destroy(gab_fdaf_plan* plan) { return gab::destroy_plan(plan, "gab_fdaf_destroy: null pointer"); }

int gab_fdaf_set_params(gab_fdaf_plan* plan, const float* d_params, gab_stream_t stream) {
    return gab::set_entry("gab_fdaf_set_params", gab::fdaf_set_range, plan, d_params, true, 0, 0, gab::as_stream(stream));
}

int gab_fdaf_set_params_tracks(gab_fdaf_plan* plan, const float* d_params, int first_track, int n_tracks,
                               gab_stream_t stream) {
    return gab::set_entry("gab_fdaf_set_params_tracks", gab::fdaf_set_range, plan, d_params, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_fdaf_set_taps(gab_fdaf_plan* plan, const float* d_taps, gab_stream_t stream) {
    return gab::set_entry("gab_fdaf_set_taps", gab::fdaf_set_taps, plan, d_taps, true, 0, 0, gab::as_stream(stream));
}

int gab_fdaf_set_taps_tracks(gab_fdaf_plan* plan, const float* d_taps, int first_track, int n_tracks, gab_stream_t stream) {
    return gab::set_entry("gab_fdaf_set_taps_tracks", gab::fdaf_set_taps, plan, d_taps, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_fdaf_reset(gab_fdaf_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_fdaf_reset", {plan}, [&]() -> int {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->W.get(), 0, plan->W.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->X.get(), 0, plan->X.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->prev.get(), 0, plan->prev.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->count.get(), 0, plan->count.size() * sizeof(unsigned), s));
        return GAB_OK;
    });
}

int gab_fdaf_process(gab_fdaf_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                     gab_stream_t stream) {
    return gab::entry("gab_fdaf_process", {plan, d_in, d_ref}, [&] {
        return gab::fdaf_process(plan, d_in, d_ref, d_err, d_est, 1, gab::as_stream(stream), "gab_fdaf_process");
    });
}

int gab_fdaf_process_batch(gab_fdaf_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                           int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_fdaf_process_batch", {plan, d_in, d_ref}, n_buffers, [&] {
        return gab::fdaf_process(plan, d_in, d_ref, d_err, d_est, n_buffers, gab::as_stream(stream),
                                 "gab_fdaf_process_batch");
    });
}

int gab_fdaf_params(gab_fdaf_plan* plan, float** d_params, size_t* n_floats) {
    return gab::entry("gab_fdaf_params", {plan, d_params, n_floats}, [&] {
        *d_params = plan->params.get();
        *n_floats = plan->params.size();
        return GAB_OK;
    });
}

int gab_fdaf_state(gab_fdaf_plan* plan, float** d_W, float** d_X, float** d_prev, unsigned** d_count, int* partitions) {
    return gab::entry("gab_fdaf_state", {plan, d_W, d_X, d_prev, d_count, partitions}, [&] {
        *d_W = plan->W.get();
        *d_X = plan->X.get();
        *d_prev = plan->prev.get();
        *d_count = plan->count.get();
        *partitions = plan->partitions;
        return GAB_OK;
    });
}

}  // extern "C"
