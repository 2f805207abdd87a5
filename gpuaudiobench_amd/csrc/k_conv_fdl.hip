// k_conv_fdl.hip — long impulse responses: uniformly partitioned overlap-save with a frequency-domain delay line
// (SURVEY.md section 7), the plan scheme GAB_CONV_SCHEME_FDL of gab_conv_create_scheme.
//
// Partition size P = B (the buffer), transform N = 2B, K = ceil(L / B) partitions; partition p holds taps
// [pB, pB + B).  Per channel the plan keeps
//   H_p   K half-spectra of the taps (B + 1 bins, 1/N folded in), made by ONE launch over (pairs x K);
//   X     a ring of input half-spectra (the delay line), one per buffer, and the previous time-domain block.
// A buffer is three launches:
//   forward   window [previous block | new block] of a channel pair, one N-point transform of the pair packed as
//             x_a + i x_b, split into the two channels' half-spectra (partner exchange), written to the newest slot;
//   MAC       Y[bin] = sum_{p<K} X[newest - p][bin] * H_p[bin], one thread per (channel, bin);
//   inverse   Y_a + i Y_b back to a pair, one N-point inverse, the last B samples out sample-major ([s*T + t]).
// Partition 0 meets the new block; every other partition meets only spectra of earlier buffers, which are exact
// zeros after a reset: a first buffer (and every stateless call) is the truncated-IR golden to rounding.
//
// Summation order.  The K partitions are cut into G = ceil(K / kGroup) groups of kGroup consecutive partitions, a cut
// that depends on K alone.  A group's sum runs p ascending from zero (one complex FMA per term); the groups' sums are
// added g ascending.  Whether one thread walks all groups (many channels: the (channel, bin) plane fills the device) or
// a thread per group writes its partial sum and the inverse adds them (few channels) is a launch choice that does not
// change one operation, so every launch form — one buffer, a batch of any n, pinned host buffers, a channel shard of
// the plan — gives the same bits.  No atomics.
//
// Batch.  The forward transforms of n buffers do not depend on any output, so a batch runs them first (n per launch,
// up to kChunk), then ONE MAC launch in which a thread reads each H_p once for all n buffers: a block convolution along
// the buffer axis with a sliding window of n input spectra in registers (per chunk K H-reads and K + n - 1 X-reads
// instead of n K of each).  The ring holds K + kChunk - 1 spectra so that a chunk's new slots never overwrite what its
// own oldest buffer still reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <type_traits>

#include "gab_fft.hpp"
#include "gab_plan.hpp"
#include "k_conv_fdl.hpp"

namespace gab {
namespace fdl {

using fft::cf;
using fft::mk;

namespace {

constexpr int kGroup = 32;                 // partitions per group of the fixed summation order
constexpr int kChunk = 16;                 // buffers per batch launch (the MAC's register window)
constexpr int kMacThreads = 256;
constexpr size_t kSpreadBelow = 1u << 18;  // (channel, bin) planes smaller than this spread the groups over threads

// Radix per transform size: N must be a power of R (BlockFFT), N / R threads per workgroup.
template <int N> struct Radix;
template <> struct Radix<256> { static constexpr int R = 4; };     // 64 threads, 4 passes
template <> struct Radix<512> { static constexpr int R = 8; };     // 64 threads, 3 passes
template <> struct Radix<1024> { static constexpr int R = 4; };    // 256 threads, 5 passes
template <> struct Radix<2048> { static constexpr int R = 2; };    // 1024 threads, 11 passes (no radix 4/8/16 divides it evenly)
template <> struct Radix<4096> { static constexpr int R = 16; };   // 256 threads, 3 passes

// Packed pair spectrum Z (k = tid + r NT, zp = conj Z[N-k]) -> the two channels' bins k <= N/2, times `sc`.
template <int N, int R>
__device__ __forceinline__ void split_store(const cf (&z)[R], const cf (&zp)[R], float sc, cf* __restrict__ da,
                                            cf* __restrict__ db, int tid) {
    constexpr int NT = N / R;
#pragma unroll
    for (int r = 0; r <= R / 2; ++r) {
        const int k = tid + r * NT;
        if (k <= N / 2) {
            const cf s = fft::cadd(z[r], zp[r]), d = fft::csub(z[r], zp[r]);
            da[k] = mk(sc * s.x, sc * s.y);                        // (Z + conj Z[N-k]) / 2
            if (db) db[k] = mk(sc * d.y, -sc * d.x);              // (Z - conj Z[N-k]) / 2i
        }
    }
}

// H_p of every pair: grid (pairs, K).  Taps [pB, pB + B) at window positions [0, B), zero-padded to N.
template <int N>
__global__ __launch_bounds__(N / Radix<N>::R) void fdl_ir_spectra_kernel(
    const float* __restrict__ ir, cf* __restrict__ H, const cf* __restrict__ tw, int T, int L, size_t plane) {
    constexpr int R = Radix<N>::R, NT = N / R, B = N / 2, BINS = B + 1;
    using F = fft::BlockFFT<N, R, false>;
    __shared__ cf lds[2 * fft::Pad<R>::size(N)];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, p = blockIdx.y;
    const int ta = 2 * q, tb = ta + 1;
    const bool hasb = tb < T;
    const float* const ia = ir + (size_t)ta * L;
    const float* const ib = ir + (size_t)tb * L;
    cf z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = p * B + tid + r * NT;
        z[r] = (r < R / 2 && j < L) ? mk(ia[j], hasb ? ib[j] : 0.0f) : mk(0.0f, 0.0f);
    }
    typename F::Bases t;
    F::load_twiddles(t, tw, tid);
    F::run(z, lds, lds + fft::Pad<R>::size(N), t, tid);
    __syncthreads();                                        // the transform's last readers are done with lds
    cf zp[R];
    fft::partner_exchange<N, R>(z, zp, lds, tid);
    cf* const hp = H + (size_t)p * plane;
    split_store<N, R>(z, zp, 0.5f / N, hp + (size_t)ta * BINS, hasb ? hp + (size_t)tb * BINS : nullptr, tid);
}

// Forward: grid (pairs, n).  Buffer j's window is [buffer j-1 | buffer j]; buffer -1 is `prev` (null: zeros).  Its
// spectrum goes to ring slot (slot0 + j) mod ring; the workgroup of the last buffer copies that buffer to `prev_next`
// (a different array than `prev`: the workgroups of one launch run in any order).
template <int N>
__global__ __launch_bounds__(N / Radix<N>::R) void fdl_forward_kernel(
    const float* __restrict__ in, const float* __restrict__ prev, float* __restrict__ prev_next,
    cf* __restrict__ X, const cf* __restrict__ tw, int T, unsigned slot0, unsigned ring, size_t plane) {
    constexpr int R = Radix<N>::R, NT = N / R, B = N / 2, BINS = B + 1;
    using F = fft::BlockFFT<N, R, false>;
    __shared__ cf lds[2 * fft::Pad<R>::size(N)];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, j = blockIdx.y;
    const int ta = 2 * q, tb = ta + 1;
    const bool hasb = tb < T;
    const size_t TB = (size_t)T * B;
    const float* const cur = in + (size_t)j * TB;
    const float* const old = j == 0 ? prev : in + (size_t)(j - 1) * TB;
    cf z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = tid + r * NT;
        if (r < R / 2) {
            z[r] = old ? mk(old[(size_t)ta * B + n], hasb ? old[(size_t)tb * B + n] : 0.0f) : mk(0.0f, 0.0f);
        } else {
            z[r] = mk(cur[(size_t)ta * B + n - B], hasb ? cur[(size_t)tb * B + n - B] : 0.0f);
        }
    }
    if (prev_next && j == (int)gridDim.y - 1) {
#pragma unroll
        for (int r = R / 2; r < R; ++r) {
            const int s = tid + r * NT - B;
            prev_next[(size_t)ta * B + s] = z[r].x;
            if (hasb) prev_next[(size_t)tb * B + s] = z[r].y;
        }
    }
    typename F::Bases t;
    F::load_twiddles(t, tw, tid);
    F::run(z, lds, lds + fft::Pad<R>::size(N), t, tid);
    __syncthreads();
    cf zp[R];
    fft::partner_exchange<N, R>(z, zp, lds, tid);
    unsigned slot = slot0 + (unsigned)j;
    if (slot >= ring) slot -= ring;
    cf* const xp = X + (size_t)slot * plane;
    split_store<N, R>(z, zp, 0.5f, xp + (size_t)ta * BINS, hasb ? xp + (size_t)tb * BINS : nullptr, tid);
}

struct MacArgs {
    const cf* X;          // [ring][plane]
    const cf* H;          // [K][plane]
    cf* Y;                // spread: [G][n][plane] partial sums; else [n][plane] sums
    size_t plane;         // channels x bins
    int K, G, n;
    unsigned ring, slot0; // slot0: ring slot of the chunk's first buffer
    int spread;
};

// MAC: grid (plane / 256, spread ? G : 1).  Thread = one (channel, bin); NB = the launch's largest n.  win[j] is the
// spectrum of buffer (chunk start + j - p) at step p: one new spectrum enters per step, the window slides.
template <int NB>
__global__ __launch_bounds__(kMacThreads) void fdl_mac_kernel(MacArgs a) {
    const size_t idx = (size_t)blockIdx.x * kMacThreads + threadIdx.x;
    if (idx >= a.plane) return;
    const int g0 = a.spread ? (int)blockIdx.y : 0;
    const int g1 = a.spread ? g0 + 1 : a.G;
    cf tot[NB];
    for (int g = g0; g < g1; ++g) {
        const int p0 = g * kGroup, p1 = min(a.K, p0 + kGroup);
        unsigned sx = a.slot0 + a.ring - (unsigned)p0;        // slot of buffer (chunk start - p0); p0 < K <= ring
        if (sx >= a.ring) sx -= a.ring;
        cf acc[NB];
        if constexpr (NB == 1) {
            // One buffer: a step's two loads do not depend on the sum, so kSteps steps' loads are issued ahead of their
            // multiply-adds (the same operations in the same order).  One step per iteration kept too few loads in
            // flight: the MAC moved 4.7 TB/s, 0.59 of 8 (profiles/r07_conv_fdl.txt).
            constexpr int kSteps = 8;
            acc[0] = mk(0.0f, 0.0f);
            int p = p0;
            for (; p + kSteps <= p1; p += kSteps) {
                cf x[kSteps], h[kSteps];
#pragma unroll
                for (int u = 0; u < kSteps; ++u) {
                    x[u] = a.X[(size_t)sx * a.plane + idx];
                    h[u] = a.H[(size_t)(p + u) * a.plane + idx];
                    sx = sx == 0 ? a.ring - 1 : sx - 1;
                }
#pragma unroll
                for (int u = 0; u < kSteps; ++u) acc[0] = fft::cfma(x[u], h[u], acc[0]);
            }
            for (; p < p1; ++p) {
                acc[0] = fft::cfma(a.X[(size_t)sx * a.plane + idx], a.H[(size_t)p * a.plane + idx], acc[0]);
                sx = sx == 0 ? a.ring - 1 : sx - 1;
            }
        } else {
            cf win[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                acc[j] = mk(0.0f, 0.0f);
                unsigned s = sx + (unsigned)j;
                if (s >= a.ring) s -= a.ring;
                win[j] = j < a.n ? a.X[(size_t)s * a.plane + idx] : mk(0.0f, 0.0f);
            }
            for (int p = p0; p < p1; ++p) {
                const cf h = a.H[(size_t)p * a.plane + idx];
                sx = sx == 0 ? a.ring - 1 : sx - 1;
                const cf xn = p + 1 < p1 ? a.X[(size_t)sx * a.plane + idx] : mk(0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[j] = fft::cfma(win[j], h, acc[j]);
#pragma unroll
                for (int j = NB - 1; j > 0; --j) win[j] = win[j - 1];
                win[0] = xn;
            }
        }
        if (a.spread) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j < a.n) a.Y[((size_t)g * a.n + j) * a.plane + idx] = acc[j];
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) tot[j] = g == g0 ? acc[j] : fft::cadd(tot[j], acc[j]);
        }
    }
    if (!a.spread) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (j < a.n) a.Y[(size_t)j * a.plane + idx] = tot[j];
    }
}

// Inverse: grid (pairs, n).  Adds the `parts` partial sums of each bin (g ascending), packs Y_a + i Y_b over all N
// bins (the upper half from the Hermitian symmetry), one inverse transform, the last B samples to out[j][s*T + t].
template <int N>
__global__ __launch_bounds__(N / Radix<N>::R) void fdl_inverse_kernel(
    const cf* __restrict__ Y, float* __restrict__ out, const cf* __restrict__ tw, int T, int parts, int n, size_t plane) {
    constexpr int R = Radix<N>::R, NT = N / R, B = N / 2, BINS = B + 1;
    using Fi = fft::BlockFFT<N, R, true>;
    __shared__ cf lds[2 * fft::Pad<R>::size(N)];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, j = blockIdx.y;
    const int ta = 2 * q, tb = ta + 1;
    const bool hasb = tb < T;
    cf z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = tid + r * NT;
        const int kk = k <= B ? k : N - k;
        const cf* ya = Y + (size_t)j * plane + (size_t)ta * BINS + kk;
        cf a = ya[0], b = hasb ? ya[BINS] : mk(0.0f, 0.0f);
        for (int g = 1; g < parts; ++g) {
            const cf* yg = ya + (size_t)g * n * plane;
            a = fft::cadd(a, yg[0]);
            if (hasb) b = fft::cadd(b, yg[BINS]);
        }
        if (k > B) { a = fft::conj(a); b = fft::conj(b); }
        z[r] = mk(a.x - b.y, a.y + b.x);                    // Y_a + i Y_b
    }
    typename Fi::Bases t;
    Fi::load_twiddles(t, tw, tid);
    Fi::run(z, lds, lds + fft::Pad<R>::size(N), t, tid);
    float* const o = out + (size_t)j * T * B;
#pragma unroll
    for (int r = R / 2; r < R; ++r) {
        const int s = tid + r * NT - B;
        o[(size_t)s * T + ta] = z[r].x;
        if (hasb) o[(size_t)s * T + tb] = z[r].y;
    }
}

// f(std::integral_constant<int, 2B>) for the plan's buffer size
template <class Fn>
void with_n(int B, Fn&& f) {
    switch (B) {
        case 128: f(std::integral_constant<int, 256>()); break;
        case 256: f(std::integral_constant<int, 512>()); break;
        case 512: f(std::integral_constant<int, 1024>()); break;
        case 1024: f(std::integral_constant<int, 2048>()); break;
        case 2048: f(std::integral_constant<int, 4096>()); break;
        default: throw std::invalid_argument("the fdl scheme: buffer size must be a power of two in [128, 2048]");
    }
}

void check_launch(const char* kernel) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw std::runtime_error(std::string(kernel) + " launch failed: " + hipGetErrorString(e));
}

}  // namespace

struct Plan {
    int T = 0, B = 0, L = 0, K = 0, G = 0, pairs = 0, bins = 0;
    size_t plane = 0;           // T x bins
    unsigned ring = 0;          // K + kChunk - 1 slots
    unsigned pos = 0;           // ring slot of the next buffer
    bool spread = false;
    int cur = 0;                // prev[cur] holds the previous block
    const cf* tw = nullptr;
    DeviceBuf<cf> H;            // [K][plane]
    DeviceBuf<cf> X;            // [ring][plane]
    DeviceBuf<cf> Xs;           // [plane]: a stateless call's spectrum (the delay line is not touched)
    DeviceBuf<cf> Y;            // [spread ? G : 1][kChunk][plane]
    DeviceBuf<float> prev[2];   // [T][B], taken in turn
};

bool shape_ok(int tracks, int bufsize, int ir_len) {
    return tracks >= 1 && bufsize >= 128 && bufsize <= 2048 && (bufsize & (bufsize - 1)) == 0 &&
           ir_len >= 1 && ir_len <= (1 << 21);
}

void destroy(Plan* f) { delete f; }

Plan* create(int tracks, int bufsize, int ir_len) {
    if (!shape_ok(tracks, bufsize, ir_len)) throw std::invalid_argument("the fdl scheme: unsupported shape");
    auto f = std::make_unique<Plan>();      // a throw below frees what has been allocated
    f->T = tracks; f->B = bufsize; f->L = ir_len;
    f->pairs = (tracks + 1) / 2;
    f->bins = bufsize + 1;
    f->K = (ir_len + bufsize - 1) / bufsize;
    f->G = (f->K + kGroup - 1) / kGroup;
    f->plane = (size_t)tracks * f->bins;
    f->ring = (unsigned)(f->K + kChunk - 1);
    f->spread = f->G > 1 && f->plane < kSpreadBelow;
    f->tw = fft::device_twiddles();
    f->H.alloc(f->plane * f->K);
    f->X.alloc(f->plane * f->ring);
    f->Xs.alloc(f->plane);
    f->Y.alloc(f->plane * kChunk * (f->spread ? f->G : 1));
    for (auto& pv : f->prev) pv.alloc((size_t)tracks * bufsize);
    GAB_HIP_CHECK(hipMemset(f->X.get(), 0, sizeof(cf) * f->X.size()));
    for (auto& pv : f->prev) GAB_HIP_CHECK(hipMemset(pv.get(), 0, sizeof(float) * pv.size()));
    GAB_HIP_CHECK(hipMemset(f->H.get(), 0, sizeof(cf) * f->H.size()));
    return f.release();
}

void set_ir(Plan* f, const float* d_ir, hipStream_t s) {
    with_n(f->B, [&](auto nc) {
        constexpr int N = decltype(nc)::value;
        fdl_ir_spectra_kernel<N><<<dim3(f->pairs, f->K), dim3(N / Radix<N>::R), 0, s>>>(d_ir, f->H.get(), f->tw, f->T, f->L,
                                                                                        f->plane);
    });
    check_launch("fdl_ir_spectra_kernel");
}

void reset(Plan* f, hipStream_t s) {
    GAB_HIP_CHECK(hipMemsetAsync(f->X.get(), 0, sizeof(cf) * f->plane * f->ring, s));
    for (auto& pv : f->prev) GAB_HIP_CHECK(hipMemsetAsync(pv.get(), 0, sizeof(float) * (size_t)f->T * f->B, s));
    f->pos = 0;
    f->cur = 0;
}

namespace {

// n <= kChunk buffers of one stream position: forward, MAC, inverse.  stateless: n == 1, zero history, the spectrum
// in Xs, partition 0 only.
void run_chunk(Plan* f, const float* in, float* out, int n, bool stateless, hipStream_t s) {
    MacArgs a;
    a.H = f->H.get();
    a.plane = f->plane;
    a.n = n;
    if (stateless) {
        a.X = f->Xs.get(); a.Y = f->Y.get(); a.K = 1; a.G = 1; a.ring = 1; a.slot0 = 0; a.spread = 0;
    } else {
        a.X = f->X.get(); a.Y = f->Y.get(); a.K = f->K; a.G = f->G; a.ring = f->ring; a.slot0 = f->pos;
        a.spread = f->spread ? 1 : 0;
    }
    const int parts = a.spread ? a.G : 1;
    with_n(f->B, [&](auto nc) {
        constexpr int N = decltype(nc)::value;
        const dim3 grid(f->pairs, n), block(N / Radix<N>::R);
        if (stateless)
            fdl_forward_kernel<N><<<grid, block, 0, s>>>(in, nullptr, nullptr, f->Xs.get(), f->tw, f->T, 0u, 1u,
                                                         f->plane);
        else
            fdl_forward_kernel<N><<<grid, block, 0, s>>>(in, f->prev[f->cur].get(), f->prev[f->cur ^ 1].get(),
                                                         f->X.get(), f->tw, f->T, f->pos, f->ring, f->plane);
        check_launch("fdl_forward_kernel");
        const dim3 mgrid((unsigned)((f->plane + kMacThreads - 1) / kMacThreads), parts);
        if (n == 1) fdl_mac_kernel<1><<<mgrid, dim3(kMacThreads), 0, s>>>(a);
        else fdl_mac_kernel<kChunk><<<mgrid, dim3(kMacThreads), 0, s>>>(a);
        check_launch("fdl_mac_kernel");
        fdl_inverse_kernel<N><<<grid, block, 0, s>>>(f->Y.get(), out, f->tw, f->T, parts, n, f->plane);
        check_launch("fdl_inverse_kernel");
    });
    if (!stateless) {
        f->pos = (f->pos + (unsigned)n) % f->ring;
        f->cur ^= 1;
    }
}

}  // namespace

void process(Plan* f, const float* in, float* out, bool streaming, hipStream_t s) {
    run_chunk(f, in, out, 1, !streaming, s);
}

void process_batch(Plan* f, const float* in, float* out, int n, hipStream_t s) {
    const size_t step = (size_t)f->T * f->B;
    for (int done = 0; done < n;) {
        const int c = std::min(kChunk, n - done);
        run_chunk(f, in + done * step, out + done * step, c, false, s);
        done += c;
    }
}

void state_bytes(const Plan* f, size_t* spectra, size_t* history) {
    if (spectra) *spectra = sizeof(cf) * f->plane * f->K;
    if (history) *history = sizeof(cf) * f->plane * f->ring + sizeof(float) * (size_t)f->T * f->B;
}

}  // namespace fdl
}  // namespace gab
