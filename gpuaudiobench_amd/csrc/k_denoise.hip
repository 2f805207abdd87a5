// k_denoise.hip — the denoise plan: a noise-reduction gate per (track, bin) with a smoothed gain, between the spectrum
// plan's analysis and the resynthesis plan's overlap-add (include/gab_c_api.h, gab_dn_*).  Two forms share one state and
// one arithmetic: stream in -> stream out in one launch, the rows never leaving the wave; and complex rows in -> complex
// rows out for whoever already holds a spectrum plan's rows.  On one device the fused form IS spectrum plan -> rows form
// -> resynthesis plan, bit for bit: outputs, history, accumulator and mask.  No counterpart in the reference.
//
//   denoise_kernel        one launch a call: one wave per pair of tracks, four waves a workgroup, no workgroup barrier.
//                         The wave owns its pair's state and walks the call's frames in ascending j (the order of the mask
//                         recursion and of the overlap-add).  Per frame: stft::analyse's gather, window product, wave-held
//                         forward transform and unpack; the gate on the lane's bins k = lane + 64 r (r < 9), mask and
//                         thresholds in registers for the whole call; the gated bins through the wave's image, from where
//                         every lane takes the bins above 512 as bin N - k (moved, not recomputed: the rows form's bits);
//                         stft::pack's packing, wave-held inverse, stft::Ring's scale, window and one rounded addition
//                         per slot into a wave-private LDS ring, whose finished samples go out in front of every frame.
//                         These stages are written out here, statement for statement what gab_stft.hpp holds for the
//                         other two plans: through the helpers the compiler schedules this kernel 0.4 to 2.3 % slower
//                         (DESIGN.md §4o), so a change to a helper is made here too.  Behind the
//                         last frame the same wave emits the rest, writes the accumulator and the mask back and forms the
//                         new history from the old one and the call's samples, every value in a register before any is
//                         written.  No input ring in LDS: a frame's samples come from the caches.
//   denoise_rows_kernel   one thread per (track, bin), contiguous along k; it walks the frames in order, the mask in a
//                         register, and reads a bin and writes a bin per frame (in place or apart).
//   DenoiseThrRule, DenoiseParamRule    what gab_plan.hpp's check kernel refuses of a table (the windows:
//                         gab_stft.hpp's rule).
//
// Output bits depend on the pair's samples, the tables and the order of frames; not on bufsize, on the cut into calls or
// batches, on the alignment of d_in or d_out or on which frames share a launch.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
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

constexpr int kDnMaxTracks = 1 << 26;                     // 2^23 workgroups of eight tracks: 2^31 threads
constexpr int kDnFields = GAB_DN_FIELDS;                  // {floor, att, rel}

// The gate of one bin, the header's five lines: every operation rounded once, one fused multiply-add where it is written.
__device__ __forceinline__ cf dn_gate(float re, float im, float& m, float thr, float inv, float floor, float att,
                                      float rel) {
    const float P = stft::power(re, im, inv);
    const float tg = P > thr ? 1.0f : floor;              // strict; a NaN P compares false
    const float c = tg > m ? att : rel;
    m = __fmaf_rn(c, __fsub_rn(m, tg), tg);
    return fft::mk(__fmul_rn(m, re), __fmul_rn(m, im));
}

// Grid: x = group of four pairs.  in: [n][T][B], only read.  out: [n][T][B].  hist: [T][1023].  acc: [T][1024] as
// resynthesis_kernel's.  mask, thr: [T][513].  params: [T][3].  wa, ws: [1024].  Frame f ends `first_end + f H` samples
// behind the call's first (1 <= first_end <= H; the last end <= n B), and its 1024 synthesised samples start at output
// sample `first_end + f H` of the call.
__global__ __launch_bounds__(256, 2) void denoise_kernel(const float* __restrict__ in, float* __restrict__ out, float* hist,
                                                     float* __restrict__ acc, float* __restrict__ mask,
                                                     const float* __restrict__ thr, const float* __restrict__ params,
                                                     const float* __restrict__ wa, const float* __restrict__ ws,
                                                     const cf* __restrict__ tw, int T, int B, int n_buffers, int H,
                                                     int first_end, int frames, float inv_edge, float inv_mid) {
    __shared__ cf lds[4 * stft::kImg];
    __shared__ float rings[4 * 2 * stft::kN];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    float* const ra = rings + w * 2 * stft::kN;
    float* const rb = ra + stft::kN;
    const int q = (int)blockIdx.x * 4 + w;
    const int ta = 2 * q, tb = 2 * q + 1;
    if (ta >= T) return;                                   // whole wave; no barriers below
    const bool hasb = tb < T;
    const bool one_buffer = n_buffers == 1;
    const int L = n_buffers * B;                           // (the host holds it below 2^31 - 1024)

    // One table of twiddles serves both directions: the inverse multiplies by the conjugates of the same values.  In
    // the two-register form, whose passes re-form the powers (the same values): with the sixteen-register form the
    // kernel does not fit two waves a SIMD without scratch.
    using FWD = fft::WaveFFT1024<false>;
    using INV = fft::WaveFFT1024<true>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);
    int base = 0;                                          // the ring slot of the oldest sample that is not out yet
    int c = 0;                                             // samples of the call that are out

    // Samples [c, e) of the call (e - c <= 1024, wave-uniform) from the ring's front to d_out; their slots become zero
    // by a store, so whatever they held (a NaN too) is gone.
    auto emit = [&](int e) {
        const int m = e - c;
        for (int idx = lane; idx < m; idx += 64) {
            const int s = (base + idx) & (stft::kN - 1);
            const int i = c + idx;
            size_t o;
            if (one_buffer) {
                o = (size_t)ta * B + i;
            } else {
                const unsigned nb = (unsigned)i / (unsigned)B, sb = (unsigned)i - nb * (unsigned)B;
                o = ((size_t)nb * T + ta) * B + sb;
            }
            out[o] = ra[s];
            ra[s] = 0.0f;
            if (hasb) out[o + B] = rb[s];
            rb[s] = 0.0f;
        }
        base = (base + m) & (stft::kN - 1);
        c = e;
        stft::wave_sync();
    };

    // the pair's state and tables of the lane's bins k = lane + 64 r: r < 8, and bin 512 in lane 0
    float ma[9], mb[9], tha[9], thb[9];
    float* const maska = mask + (size_t)ta * stft::kBins;
    const float* const thra = thr + (size_t)ta * stft::kBins;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        ma[r] = mb[r] = 1.0f;
        tha[r] = thb[r] = 0.0f;
        if (k <= stft::kN / 2) {
            ma[r] = maska[k];
            tha[r] = thra[k];
            if (hasb) {
                mb[r] = maska[stft::kBins + k];
                thb[r] = thra[stft::kBins + k];
            }
        }
    }
    const float* const pa = params + (size_t)ta * kDnFields;
    const float floora = pa[0], atta = pa[1], rela = pa[2];
    const float floorb = hasb ? pa[3] : 1.0f, attb = hasb ? pa[4] : 0.0f, relb = hasb ? pa[5] : 0.0f;
    float wn[16], g[16];
    float* const acca = acc + (size_t)ta * stft::kN;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = lane + 64 * r;
        wn[r] = wa[n];
        g[r] = ws[n];
        ra[n] = acca[n];
        rb[n] = hasb ? acca[stft::kN + n] : 0.0f;
    }
    stft::wave_sync();
    for (int f = 0; f < frames; ++f) {
        const int end = first_end + f * H;
        emit(end);                                         // the ring's front is now the frame's first output sample
        // ---- analysis (spectrum_kernel): gather, window, transform, unpack ----
        const int start = end - stft::kN;
        cf z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = lane + 64 * r;
            const float sa = stft::sample(in, hist, T, B, one_buffer, ta, start + n);
            const float sb = hasb ? stft::sample(in, hist, T, B, one_buffer, tb, start + n) : 0.0f;
            z[r] = fft::mk(__fmul_rn(wn[r], sa), __fmul_rn(wn[r], sb));
        }
        FWD::run(z, img, t, lane);                         // EXEC is all ones here: every loop above has reconverged
        // partner Z[(N - k) mod N], k = lane + 64 r: bins 0..512 are r < 8 plus (r = 8, lane 0)
        const unsigned rbase = (unsigned)lane + ((unsigned)lane >> 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) img[rbase + 68 * r] = z[r];
        __builtin_amdgcn_wave_barrier();
        cf xa[9], xb[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            xa[r] = fft::mk(0.0f, 0.0f);
            xb[r] = fft::mk(0.0f, 0.0f);
            if (k <= stft::kN / 2) {
                const cf zp = fft::conj(img[fft::Pad<16>::at((stft::kN - k) & (stft::kN - 1))]);
                const cf s = fft::cadd(z[r], zp), d = fft::csub(z[r], zp);
                xa[r] = fft::mk(0.5f * s.x, 0.5f * s.y);
                xb[r] = fft::mk(0.5f * d.y, -0.5f * d.x);
            }
        }
        // ---- the gate on the rows' bits; the row of a track that is not there is zeros, as the resynthesiser reads it ----
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            const float inv = (k == 0 || k == stft::kN / 2) ? inv_edge : inv_mid;
            if (k <= stft::kN / 2) {
                xa[r] = dn_gate(xa[r].x, xa[r].y, ma[r], tha[r], inv, floora, atta, rela);
                if (hasb) xb[r] = dn_gate(xb[r].x, xb[r].y, mb[r], thb[r], inv, floorb, attb, relb);
                else xb[r] = fft::mk(0.0f, 0.0f);
            }
        }
        stft::wave_sync();                                    // every lane has read its partners: the image is free
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = lane + 64 * r;
            if (k <= stft::kN / 2) {
                img[k] = xa[r];
                img[stft::kImgB + k] = xb[r];
            }
        }
        stft::wave_sync();
        // ---- synthesis (resynthesis_kernel): Z[k] = Xa[k] + i Xb[k] (k <= 512), conj(Xa[N - k]) + i conj(Xb[N - k])
        // (k > 512); the imaginary parts of bins 0 and 512 are read as zero ----
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = lane + 64 * r;
            const bool mirror = k > stft::kN / 2;
            cf a, b;
            if (r < 8) {
                a = xa[r];
                b = xb[r];
            } else {
                const int kk = mirror ? stft::kN - k : k;      // (r = 8, lane 0: bin 512, the lane's own)
                a = img[kk];
                b = img[stft::kImgB + kk];
            }
            if (k == 0 || k == stft::kN / 2) {
                a.y = 0.0f;
                b.y = 0.0f;
            }
            z[r] = mirror ? fft::mk(__fadd_rn(a.x, b.y), __fsub_rn(b.x, a.y))
                          : fft::mk(__fsub_rn(a.x, b.y), __fadd_rn(a.y, b.x));
        }
        stft::wave_sync();                                    // every lane has its mirrored bins: the image is free again
        INV::run(z, img, t, lane);                         // EXEC is all ones here too
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int s = (base + lane + 64 * r) & (stft::kN - 1);
            ra[s] = __fadd_rn(ra[s], __fmul_rn(g[r], __fmul_rn(z[r].x, 0x1p-10f)));
            rb[s] = __fadd_rn(rb[s], __fmul_rn(g[r], __fmul_rn(z[r].y, 0x1p-10f)));
        }
        stft::wave_sync();
    }
    emit(L);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = lane + 64 * r;
        const int s = (base + n) & (stft::kN - 1);
        acca[n] = ra[s];
        if (hasb) acca[stft::kN + n] = rb[s];
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        if (k <= stft::kN / 2) {
            maska[k] = ma[r];
            if (hasb) maska[stft::kBins + k] = mb[r];
        }
    }
    // hist becomes the last 1023 samples of hist ++ the call's n B samples.  Only this wave reads or writes its pair's
    // rows, and every value is in a register (the wait) before any is written.
    float va[16], vb[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int col = lane + 64 * r;                     // the new row's column: sample L - 1023 + col of the call
        va[r] = vb[r] = 0.0f;
        if (col < stft::kHist) {
            va[r] = stft::sample(in, hist, T, B, one_buffer, ta, L - stft::kHist + col);
            if (hasb) vb[r] = stft::sample(in, hist, T, B, one_buffer, tb, L - stft::kHist + col);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);                         // vmcnt(0): every load above has returned
    stft::wave_sync();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int col = lane + 64 * r;
        if (col < stft::kHist) {
            hist[(size_t)ta * stft::kHist + col] = va[r];
            if (hasb) hist[(size_t)tb * stft::kHist + col] = vb[r];
        }
    }
}

// Grid: x = 256 (track, bin) values, contiguous along k.  rin, rout: [frames][T][513] complex, equal or apart.
__global__ __launch_bounds__(256) void denoise_rows_kernel(const float2* rin, float2* rout, float* __restrict__ mask,
                                                          const float* __restrict__ thr,
                                                          const float* __restrict__ params, int T, int frames,
                                                          float inv_edge, float inv_mid) {
    const size_t per_frame = (size_t)T * stft::kBins;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_frame) return;
    const size_t t = i / stft::kBins;
    const int k = (int)(i - t * stft::kBins);
    const float inv = stft::inv_of(k, inv_edge, inv_mid);
    const float floor = params[t * kDnFields], att = params[t * kDnFields + 1], rel = params[t * kDnFields + 2];
    const float th = thr[i];
    float m = mask[i];
    for (int f = 0; f < frames; ++f) {
        const float2 x = rin[(size_t)f * per_frame + i];
        const cf y = dn_gate(x.x, x.y, m, th, inv, floor, att, rel);
        rout[(size_t)f * per_frame + i] = make_float2(y.x, y.y);
    }
    mask[i] = m;
}

// src: [n_tracks][513].  Every value >= 0 or +inf; a NaN fails the comparison.
struct DenoiseThrRule {
    __device__ bool refuses(const float* src, size_t i) const { return !(src[i] >= 0.0f); }
    std::string refusal(unsigned i, int first_track) const {
        return "track " + std::to_string(first_track + (int)(i / stft::kBins)) + " bin " +
               std::to_string((int)(i % stft::kBins)) + " (threshold) must be >= 0 or +inf, not a NaN; the plan keeps its thresholds";
    }
};

const char* const kDnFieldNames[kDnFields] = {"floor", "att", "rel"};
const char* const kDnFieldRules[kDnFields] = {"must be within [0, 1]", "must be within [0, 1)", "must be within [0, 1)"};

// src: [n_tracks][3] (a NaN fails every comparison)
struct DenoiseParamRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i % kDnFields);
        return !(v >= 0.0f) || (field == 0 ? !(v <= 1.0f) : !(v < 1.0f));
    }
    std::string refusal(unsigned i, int first_track) const {
        const int field = (int)(i % kDnFields);
        return row_refusal(i, kDnFields, first_track, kDnFieldNames[field], kDnFieldRules[field]);
    }
};

}  // namespace
}  // namespace gab

struct gab_dn_plan {
    int tracks = 0, bufsize = 0, hop = 0;
    int phase = 0;                     // samples since the reset, mod hop
    float inv_edge = 0.0f, inv_mid = 0.0f;     // (float)(1 / S^2), (float)(4 / S^2), S the analysis window's sum
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::DeviceBuf<float> analysis;    // [1024]
    gab::DeviceBuf<float> synthesis;   // [1024]
    gab::DeviceBuf<float> hist;        // [T][1023]
    gab::DeviceBuf<float> acc;         // [T][1024]
    gab::DeviceBuf<float> mask;        // [T][513]
    gab::DeviceBuf<float> thr;         // [T][513]
    gab::DeviceBuf<float> params;      // [T][3]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// 1.0f in every mask value, on s
void dn_open_mask(gab_dn_plan* p, hipStream_t s) {
    GAB_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->mask.get()), 0x3f800000, p->mask.size(), s));
}

// n buffers in one launch on s, from the plan's position; nothing is allocated, nothing waits.
int dn_launch(gab_dn_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    if (int rc = stft::check_length(who, *p, n_buffers)) return rc;
    if (overlaps(d_in, d_out, (size_t)n_buffers * p->bufsize * p->tracks)) return refuse(who, "d_in and d_out overlap");
    const long long frames = stft::count(*p, n_buffers);
    const unsigned groups = (unsigned)(((p->tracks + 1) / 2 + 3) / 4);
    denoise_kernel<<<dim3(groups), 256, 0, s>>>(d_in, d_out, p->hist.get(), p->acc.get(), p->mask.get(), p->thr.get(),
                                                p->params.get(), p->analysis.get(), p->synthesis.get(), p->tw, p->tracks,
                                                p->bufsize, n_buffers, p->hop, stft::first_end(*p), (int)frames,
                                                p->inv_edge, p->inv_mid);
    if (int rc = launch_status("denoise_kernel")) return rc;
    stft::advance(*p, n_buffers);
    return GAB_OK;
}

int dn_set_thresholds(gab_dn_plan* p, const float* d_thr, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t n = (size_t)n_tracks * stft::kBins;
    return check_then(p->flag, s, who, d_thr, n, DenoiseThrRule{}, first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->thr.get() + (size_t)first_track * stft::kBins, d_thr, n * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
}

int dn_set_params(gab_dn_plan* p, const float* d_params, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t n = (size_t)n_tracks * kDnFields;
    return check_then(p->flag, s, who, d_params, n, DenoiseParamRule{}, first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->params.get() + (size_t)first_track * kDnFields, d_params, n * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_dn_create(gab_dn_plan** out, int tracks, int bufsize, int hop) {
    return gab::create_entry("gab_dn_create", out, tracks, bufsize, [&] {
        if (int rc = gab::stft::check_hop("gab_dn_create", hop)) return rc;
        if (tracks > gab::kDnMaxTracks)
            return gab::bad_arg("gab_dn_create: more than 2^23 workgroups (tracks / 8) in one launch");
        return GAB_OK;
    }, [&](gab_dn_plan& p) {
        p.hop = hop;
        p.tw = gab::fft::device_twiddles();
        p.analysis.alloc(gab::stft::kN);
        p.synthesis.alloc(gab::stft::kN);
        p.hist.alloc((size_t)tracks * gab::stft::kHist);
        p.acc.alloc((size_t)tracks * gab::stft::kN);
        p.mask.alloc((size_t)tracks * gab::stft::kBins);
        p.thr.alloc((size_t)tracks * gab::stft::kBins);
        p.params.alloc((size_t)tracks * gab::kDnFields);
        p.flag.alloc(1);
        // the spectrum plan's periodic Hann window and the resynthesis plan's dual of it at this hop; thresholds of
        // zero under {floor, att, rel} = {1, 0, 0}: transparent
        const std::vector<float> w = gab::stft_hann(), g = gab::stft_hann_dual(hop);
        gab::stft::scale(p, gab::stft_window_sum(w));
        std::vector<float> rows((size_t)tracks * gab::kDnFields, 0.0f);
        for (int t = 0; t < tracks; ++t) rows[(size_t)t * gab::kDnFields] = 1.0f;
        GAB_HIP_CHECK(hipMemcpy(p.analysis.get(), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemcpy(p.synthesis.get(), g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemcpy(p.params.get(), rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.hist.get(), 0, p.hist.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.acc.get(), 0, p.acc.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.thr.get(), 0, p.thr.size() * sizeof(float)));
        gab::dn_open_mask(&p, nullptr);
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_dn_destroy(gab_dn_plan* plan) { return gab::destroy_plan(plan, "gab_dn_destroy: null pointer"); }

// check, then commit (gab_plan.hpp): a refused table leaves the plan's as it was
int gab_dn_set_thresholds(gab_dn_plan* plan, const float* d_thr, int first_track, int n_tracks, gab_stream_t stream) {
    return gab::set_entry("gab_dn_set_thresholds", gab::dn_set_thresholds, plan, d_thr, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_dn_set_params(gab_dn_plan* plan, const float* d_params, int first_track, int n_tracks, gab_stream_t stream) {
    return gab::set_entry("gab_dn_set_params", gab::dn_set_params, plan, d_params, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

// both windows are checked before either is written: on the device value by value, then on the host the analysis sum
int gab_dn_set_windows(gab_dn_plan* plan, const float* d_analysis, const float* d_synthesis, gab_stream_t stream) {
    const char* const who = "gab_dn_set_windows";
    return gab::entry(who, {plan, d_analysis, d_synthesis}, [&]() -> int {
        hipStream_t s = gab::as_stream(stream);
        const size_t bytes = gab::stft::kN * sizeof(float);
        int rc_synthesis = GAB_OK;
        bool zero_sum = false;
        const int rc = gab::check_then(plan->flag, s, who, d_analysis, (size_t)gab::stft::kN, gab::stft::WindowRule{1}, 0, [&] {
            rc_synthesis = gab::check_then(plan->flag, s, who, d_synthesis, (size_t)gab::stft::kN,
                                           gab::stft::WindowRule{2}, 0, [&] {
                std::vector<float> w(gab::stft::kN);
                GAB_HIP_CHECK(hipMemcpyAsync(w.data(), d_analysis, bytes, hipMemcpyDeviceToHost, s));
                GAB_HIP_CHECK(hipStreamSynchronize(s));
                const double S = gab::stft_window_sum(w);
                if (S == 0.0) { zero_sum = true; return; }
                GAB_HIP_CHECK(hipMemcpyAsync(plan->analysis.get(), d_analysis, bytes, hipMemcpyDeviceToDevice, s));
                GAB_HIP_CHECK(hipMemcpyAsync(plan->synthesis.get(), d_synthesis, bytes, hipMemcpyDeviceToDevice, s));
                GAB_HIP_CHECK(hipStreamSynchronize(s));
                gab::stft::scale(*plan, S);
            });
        });
        if (rc) return rc;
        if (rc_synthesis) return rc_synthesis;
        if (zero_sum) return gab::refuse(who, "the analysis window's sum is zero; the plan keeps its windows");
        return GAB_OK;
    });
}

int gab_dn_reset(gab_dn_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_dn_reset", {plan}, [&] {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->hist.get(), 0, plan->hist.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->acc.get(), 0, plan->acc.size() * sizeof(float), s));
        gab::dn_open_mask(plan, s);
        plan->phase = 0;
        return GAB_OK;
    });
}

int gab_dn_process(gab_dn_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_dn_process", {plan, d_in, d_out}, [&] {
        return gab::dn_launch(plan, d_in, d_out, 1, gab::as_stream(stream), "gab_dn_process");
    });
}

int gab_dn_process_batch(gab_dn_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_dn_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::dn_launch(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_dn_process_batch");
    });
}

int gab_dn_process_rows(gab_dn_plan* plan, const float* d_rows_in, float* d_rows_out, int n_frames, gab_stream_t stream) {
    const char* const who = "gab_dn_process_rows";
    return gab::entry(who, {plan, d_rows_in, d_rows_out}, [&]() -> int {
        if (n_frames < 0) return gab::refuse(who, "n_frames must be >= 0");
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_rows_in), o0 = reinterpret_cast<uintptr_t>(d_rows_out);
        if (i0 & 7u) return gab::refuse(who, "d_rows_in must lie on an 8-byte boundary");
        if (o0 & 7u) return gab::refuse(who, "d_rows_out must lie on an 8-byte boundary");
        const size_t per_frame = (size_t)plan->tracks * gab::stft::kBins;
        const uintptr_t bytes = (uintptr_t)n_frames * per_frame * 2 * sizeof(float);
        if (i0 != o0 && i0 < o0 + bytes && o0 < i0 + bytes)
            return gab::refuse(who, "d_rows_in and d_rows_out overlap in part; they are the same rows or apart");
        if (n_frames == 0) return GAB_OK;
        gab::denoise_rows_kernel<<<dim3((unsigned)((per_frame + 255) / 256)), 256, 0, gab::as_stream(stream)>>>(
            reinterpret_cast<const float2*>(d_rows_in), reinterpret_cast<float2*>(d_rows_out), plan->mask.get(),
            plan->thr.get(), plan->params.get(), plan->tracks, n_frames, plan->inv_edge, plan->inv_mid);
        return gab::launch_status("denoise_rows_kernel");
    });
}

int gab_dn_state(gab_dn_plan* plan, float** d_hist, float** d_acc, float** d_mask, int* position_mod_hop) {
    return gab::entry("gab_dn_state", {plan, d_hist, d_acc, d_mask, position_mod_hop}, [&] {
        *d_hist = plan->hist.get();
        *d_acc = plan->acc.get();
        *d_mask = plan->mask.get();
        *position_mod_hop = plan->phase;
        return GAB_OK;
    });
}

int gab_dn_tables(gab_dn_plan* plan, float** d_thr, float** d_params) {
    return gab::entry("gab_dn_tables", {plan, d_thr, d_params}, [&] {
        *d_thr = plan->thr.get();
        *d_params = plan->params.get();
        return GAB_OK;
    });
}

int gab_dn_latency(gab_dn_plan* plan, int* samples) {
    return gab::entry("gab_dn_latency", {plan, samples}, [&] {
        *samples = gab::stft::kN;
        return GAB_OK;
    });
}

}  // extern "C"
