// gab_stft.hpp — what the short-time Fourier plans (spectrum, resynthesis, denoise) share.  The fused
// denoise kernel uses the constants, sample, power, wave_sync and the host side, and keeps analyse, pack and the Ring
// written out in its own body (k_denoise.hip says why); the fdaf plan (k_fdaf.hip) holds its frames in registers and
// uses spectra, pack_rows, tap_spectrum and wave_sync, and so does the matrix-convolution plan (k_mconv.hip):
//   device   the sample fetch, the analysis of a pair's frame (its gather, and spectra() behind it), the power of a bin, the packing of a pair's rows, the
//            overlap-add ring, the history update, the wave's hand-over fence
//   host     the two default windows, the hop grid and what the plans refuse of it, the power factors, the window rule
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "gab_fft.hpp"
#include "gab_plan.hpp"

namespace gab {
namespace stft {

using fft::cf;

constexpr int kN = 1024;                                  // the transform, and the floats of a track's accumulator
constexpr int kBins = kN / 2 + 1;                         // 513
constexpr int kHist = kN - 1;                             // samples carried per track
constexpr int kMinHop = 32;
constexpr int kImg = fft::Pad<16>::size(kN);              // cf entries of a wave's LDS image (1088)
constexpr int kImgB = 544;                                // track b's bins in the image: [544, 544 + 513) <= 1088

// ---- device ----
// The lanes of a wave hand LDS words to one another (ring slots, powers, gated bins): LDS instructions of a wave
// execute in order, and this keeps the compiler from moving them across the hand-over.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Sample i (relative to the call's first sample; -1023 <= i < n_buffers B) of track t.  in: [n][T][B].  hist: [T][1023].
__device__ __forceinline__ float sample(const float* __restrict__ in, const float* hist, int T, int B, bool one_buffer,
                                        int t, int i) {
    if (i < 0) return hist[(size_t)t * kHist + (kHist + i)];
    if (one_buffer) return in[(size_t)t * B + i];
    const unsigned nb = (unsigned)i / (unsigned)B, s = (unsigned)i - nb * (unsigned)B;
    return in[((size_t)nb * T + t) * B + s];
}

// analyse() behind its gather, for a plan that holds its frames in registers (the fdaf plan, where a window of ones is
// no product at all): lane j enters with z[r] = a[j + 64 r] + i b[j + 64 r], the packed frame of a pair, which goes
// through the wave-held forward transform and is unpacked as fft_r2c_1024_kernel does.  xa[r], xb[r]: bin k = lane + 64 r
// of either track; bins 0..512 are r < 8 plus (r = 8, lane 0), and zero above.  z is left holding the packed transform.
// The partner reads of img are not fenced off here.
template <class TW>
__device__ __forceinline__ void spectra(cf (&z)[16], cf* img, const TW& t, int lane, cf (&xa)[9], cf (&xb)[9]) {
    fft::WaveFFT1024<false>::run(z, img, t, lane);        // EXEC is all ones here: every loop of the caller has reconverged
    // partner Z[(N - k) mod N], k = lane + 64 r
    const unsigned rb = (unsigned)lane + ((unsigned)lane >> 4);
#pragma unroll
    for (int r = 0; r < 16; ++r) img[rb + 68 * r] = z[r];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        xa[r] = fft::mk(0.0f, 0.0f);
        xb[r] = fft::mk(0.0f, 0.0f);
        if (k <= kN / 2) {
            const cf zp = fft::conj(img[fft::Pad<16>::at((kN - k) & (kN - 1))]);
            const cf s = fft::cadd(z[r], zp), d = fft::csub(z[r], zp);
            xa[r] = fft::mk(0.5f * s.x, 0.5f * s.y);
            xb[r] = fft::mk(0.5f * d.y, -0.5f * d.x);
        }
    }
}

// The frame of tracks ta and ta + 1 (hasb: the second is there) that starts at sample `start` of the call: lane j
// gathers s[start + j + 64 r], multiplies by wn[r] = w[j + 64 r] in one rounded product, and hands the packed frame to
// spectra().
template <class TW>
__device__ __forceinline__ void analyse(const float* __restrict__ in, const float* hist, int T, int B, bool one_buffer,
                                        int ta, bool hasb, int start, const float (&wn)[16], cf* img, const TW& t,
                                        int lane, cf (&xa)[9], cf (&xb)[9]) {
    cf z[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = lane + 64 * r;
        const float sa = sample(in, hist, T, B, one_buffer, ta, start + n);
        const float sb = hasb ? sample(in, hist, T, B, one_buffer, ta + 1, start + n) : 0.0f;
        z[r] = fft::mk(__fmul_rn(wn[r], sa), __fmul_rn(wn[r], sb));
    }
    spectra(z, img, t, lane, xa, xb);
}

// P[k] = (re re + im im) inv_k, every operation rounded once; inv_k is (float)(1 / S^2) at bins 0 and 512, else
// (float)(4 / S^2)
__device__ __forceinline__ float inv_of(int k, float inv_edge, float inv_mid) {
    return (k == 0 || k == kN / 2) ? inv_edge : inv_mid;
}
__device__ __forceinline__ float power(float re, float im, float inv) {
    return __fmul_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), inv);
}

// Entry k of the inverse transform of a pair: Z[k] = Xa[k] + i Xb[k] (k <= 512), conj(Xa[N - k]) + i conj(Xb[N - k])
// (k > 512), where a and b are bin k of the two rows, above 512 bin N - k; the imaginary parts of bins 0 and 512 are
// read as zero.
__device__ __forceinline__ cf pack(cf a, cf b, int k) {
    if (k == 0 || k == kN / 2) {
        a.y = 0.0f;
        b.y = 0.0f;
    }
    return k > kN / 2 ? fft::mk(__fadd_rn(a.x, b.y), __fsub_rn(b.x, a.y))
                      : fft::mk(__fsub_rn(a.x, b.y), __fadd_rn(a.y, b.x));
}

// pack() of a pair's rows held in registers (a[r], b[r]: bin k = lane + 64 r, as spectra() leaves them): the bins above
// 512 are bin N - k of another lane, so the rows go through the image (which must be free), and z becomes the pair's
// packed spectrum, entry k = lane + 64 r.  Ends with the image free again.
__device__ __forceinline__ void pack_rows(const cf (&a)[9], const cf (&b)[9], cf* img, int lane, cf (&z)[16]) {
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        if (k <= kN / 2) {
            img[k] = a[r];
            img[kImgB + k] = b[r];
        }
    }
    wave_sync();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = lane + 64 * r;
        if (r < 8) {
            z[r] = pack(a[r], b[r], k);
        } else {
            const int kk = kN - k;                         // (r = 8, lane 0: bin 512 itself)
            z[r] = pack(img[kk], img[kImgB + kk], k);
        }
    }
    wave_sync();
}

// The half-spectrum of one partition of time-domain taps, [h[0 .. 512) | 512 zeros], alone in its transform (the
// partner's half is zeros), to dst[0 .. 513): what the fdaf and the matrix-convolution plans' set_taps store.
template <class TW>
__device__ __forceinline__ void tap_spectrum(const float* __restrict__ h, cf* __restrict__ dst, cf* img, const TW& t,
                                             int lane) {
    cf z[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        z[j] = fft::mk(h[lane + 64 * j], 0.0f);
        z[j + 8] = fft::mk(0.0f, 0.0f);
    }
    cf xa[9], xb[9];
    spectra(z, img, t, lane, xa, xb);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        if (k <= kN / 2) dst[k] = xa[r];
    }
}

// A pair's accumulator in the wave's two LDS rows of 1024 floats, indexed from a moving base.  acc: the pair's rows
// of [T][1024]: acc[i] is the partial sum of the output sample i places behind the plan's position.  out: [n][T][B].
// The caller puts a wave_sync() behind fill() and behind add(); emit() ends in one.
struct Ring {
    float* const ra;
    float* const rb;
    float* const out;
    const int T, B, ta, lane;
    const bool one_buffer, hasb;
    int base = 0;                                          // the ring slot of the oldest sample that is not out yet
    int c = 0;                                             // samples of the call that are out

    __device__ __forceinline__ void fill(const float* acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = lane + 64 * r;
            ra[n] = acc[n];
            rb[n] = hasb ? acc[kN + n] : 0.0f;
        }
    }
    // Samples [c, e) of the call (e - c <= 1024, wave-uniform) from the ring's front to out; their slots become zero
    // by a store, so whatever they held (a NaN too) is gone.
    __device__ __forceinline__ void emit(int e) {
        const int m = e - c;
        for (int idx = lane; idx < m; idx += 64) {
            const int s = (base + idx) & (kN - 1);
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
        base = (base + m) & (kN - 1);
        c = e;
        wave_sync();
    }
    // The frame at the ring's front: the inverse transform's z scaled by 2^-10, times the window g, one rounded
    // addition per slot.
    __device__ __forceinline__ void add(const cf (&z)[16], const float (&g)[16]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int s = (base + lane + 64 * r) & (kN - 1);
            ra[s] = __fadd_rn(ra[s], __fmul_rn(g[r], __fmul_rn(z[r].x, 0x1p-10f)));
            rb[s] = __fadd_rn(rb[s], __fmul_rn(g[r], __fmul_rn(z[r].y, 0x1p-10f)));
        }
    }
    // back to acc, from the base
    __device__ __forceinline__ void store(float* acc) const {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = lane + 64 * r;
            const int s = (base + n) & (kN - 1);
            acc[n] = ra[s];
            if (hasb) acc[kN + n] = rb[s];
        }
    }
};

// Track t's history becomes the last 1023 samples of hist ++ the call's L samples, in two steps: every value into a
// register (v[r]: the new row's column lane + 64 r, sample L - 1023 + column of the call; zero for a track that is not
// `there`), and, once every lane that reads the row has its values, the row.
__device__ __forceinline__ void hist_read(float (&v)[16], const float* __restrict__ in, const float* hist, int T, int B,
                                          bool one_buffer, int t, bool there, int L, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int col = lane + 64 * r;
        v[r] = 0.0f;
        if (there && col < kHist) v[r] = sample(in, hist, T, B, one_buffer, t, L - kHist + col);
    }
}
__device__ __forceinline__ void hist_write(const float (&v)[16], float* hist, int t, int lane) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int col = lane + 64 * r;
        if (col < kHist) hist[(size_t)t * kHist + col] = v[r];
    }
}

// src: [1024].  of: 0 the plan's one window, 1 and 2 the analysis and the synthesis window of a plan with two.  One type
// for the three files on purpose: check_kernel<float, WindowRule> is then one kernel that each of them instantiates.
struct WindowRule {
    int of;
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int) const {
        const char* const which[] = {"", "analysis ", "synthesis "};
        return std::string(which[of]) + "window value " + std::to_string(i) + " is not finite; the plan keeps its window" +
               (of ? "s" : "");
    }
};

// ---- host: the hop grid ----
// A plan P holds bufsize, hop and phase, the samples since the reset mod hop.  Frame j ends (the analysis) or starts (the
// synthesis) j hop samples behind the reset; a call takes the frames whose mark lies inside it.
template <class P>
long long count(const P& p, int n_buffers) {              // frames of a call of n buffers from the plan's position
    return ((long long)p.phase + (long long)n_buffers * p.bufsize) / p.hop;
}
template <class P>
int first_end(const P& p) { return p.hop - p.phase; }     // the first mark, in samples behind the call's first
template <class P>
void advance(P& p, int n_buffers) { p.phase = (int)(((long long)p.phase + (long long)n_buffers * p.bufsize) % p.hop); }

inline int check_hop(const char* who, int hop) {
    return hop < kMinHop || hop > kN ? refuse(who, "hop must be 32..1024") : GAB_OK;
}
// (a frame's samples are indexed in an int, up to 1024 past the call's last)
template <class P>
int check_length(const char* who, const P& p, int n_buffers) {
    return (long long)n_buffers * p.bufsize > 0x7fffffffLL - kN ? refuse(who, "n_buffers * bufsize must be below 2^31 - 1024")
                                                                 : GAB_OK;
}
// the body of gab_X_frames: the most frames a call of n buffers can take, ceil(n B / H)
template <class P>
int capacity(const char* who, const P& p, int n_buffers, int* capacity) {
    const long long cap = ((long long)n_buffers * p.bufsize + p.hop - 1) / p.hop;
    if (cap > 0x7fffffffLL) return refuse(who, "n_buffers * bufsize is too large");
    *capacity = (int)cap;
    return GAB_OK;
}

// S = sum of the analysis window in float64, ascending n; the two factors of a power
template <class P>
void scale(P& p, double S) {
    p.inv_edge = (float)(1.0 / (S * S));
    p.inv_mid = (float)(4.0 / (S * S));
}

}  // namespace stft

// ---- host: the two default windows, made once so that the three plans hold the same bits ----
// The periodic Hann window 0.5 - 0.5 cos(2 pi n / N): float64, rounded once.
inline std::vector<float> stft_hann() {
    const double pi = 3.14159265358979323846;
    std::vector<float> w((size_t)stft::kN);
    for (int n = 0; n < stft::kN; ++n) w[(size_t)n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)n / (double)stft::kN));
    return w;
}

// S: the float64 sum of the float32 values, added in ascending n.
inline double stft_window_sum(const std::vector<float>& w) {
    double S = 0.0;
    for (int n = 0; n < stft::kN; ++n) S += (double)w[(size_t)n];
    return S;
}

// The least-squares dual of stft_hann() at hop H: g[n] = w[n] / sum_m w[n + m H]^2, m over every index inside 0..1023 in
// ascending order, 0 where the sum is 0: float64 on the float32 values of w, rounded once.
inline std::vector<float> stft_hann_dual(int H) {
    const std::vector<float> wf = stft_hann();
    std::vector<double> w((size_t)stft::kN);
    for (int n = 0; n < stft::kN; ++n) w[(size_t)n] = (double)wf[(size_t)n];
    std::vector<float> g((size_t)stft::kN);
    for (int n = 0; n < stft::kN; ++n) {
        double s = 0.0;
        for (int i = n % H; i < stft::kN; i += H) s += w[(size_t)i] * w[(size_t)i];
        g[(size_t)n] = s == 0.0 ? 0.0f : (float)(w[(size_t)n] / s);
    }
    return g;
}

}  // namespace gab
