// k_eq.hip — per-track biquad cascades (a parametric equaliser plan): `sections` second-order sections in series on
// every track, each (track, section) with its own coefficients, the DF-II state (z1, z2 of gab_iir) carried from
// buffer to buffer.  No counterpart in the reference, whose IIR benchmark runs one shared biquad (cuda/bench_iir.cu).
//
//   eq_scan_kernel<M, H>    the hot path: iir_scan_kernel's wave scan, once per section, on samples that stay in
//                           registers — one read and one write of the audio per buffer whatever the section count;
//   eq_sequential_kernel    the anchor: one lane per track in the ordered form (one rounding per operation), any shape;
//   eq_consts_kernel        checks a set of coefficients and makes the scan's constants in float64 on the device.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kEqMaxSections = 16;

// What one (track, section) needs, as the scan kernel reads it: the five coefficients, the w-response of sample i to a
// state entering the lane (alpha, beta: the first row of A^(i+1)), and (A^M)^(2^k) for the six combine steps,
// row-major 2x2 — IirScanConsts plus the coefficients, as a table row instead of a kernel argument.  29 + 2M words,
// padded to 16 bytes.  A wave reads its track's rows with scalar loads: the row lives in SGPRs.
// The scan's state is not (z1, z2) but (u, d) = (z1, z1 - z2).  A section with poles near z = 1 (anything below a
// few hundred hertz) has A^n ~ [n+1 -n; n -(n-1)] and z1 ~ z2 hundreds of times the signal: (n+1) z1 - n z2 in
// float32 loses n eps |z|, measured 64 times the ordered form's own round-off on a 240 Hz high-pass.  On (u, d) the
// same map is ~ [1 n; small 1] acting on a large u and a small d: no cancellation.  alpha, beta and p are stored
// for that basis (formed in float64 from the (z1, z2) powers).
template <int M>
struct alignas(16) EqRow {
    float b0, b1, b2, a1, a2;
    float alpha[M], beta[M];
    float p[6][4];
};
constexpr int eq_row_words(int M) { return (29 + 2 * M + 3) / 4 * 4; }
static_assert(sizeof(EqRow<1>) == 4 * eq_row_words(1) && sizeof(EqRow<2>) == 4 * eq_row_words(2) &&
              sizeof(EqRow<4>) == 4 * eq_row_words(4) && sizeof(EqRow<8>) == 4 * eq_row_words(8), "row layout");

// ---------------------------------------------------------------------------
// The table.  One thread per (track, section) of the range [first_track, first_track + n_tracks).
//   commit = 0: check only — a section outside the stability triangle (|a2| < 1, |a1| < 1 + a2) or with a value that
//               is not finite lowers *flag to its index in the range (so the host names the FIRST one);
//   commit = 1: write the rows (make_scan_consts' arithmetic, k_recursive.hip: float64, the (u, d) basis, rounded once).
// src: [n_tracks][S][5] = {b0, b1, b2, a1, a2}; null: the identity filter.
// The matrix powers are NOT formed in the hot kernel by float32 squaring: an error of 2^k eps in A^(M 2^k) multiplies
// states that a low-frequency section makes hundreds of times larger than the signal.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eq_consts_kernel(const float* __restrict__ src, float* __restrict__ table,
                                                       unsigned* __restrict__ flag, int first_track, int n_tracks,
                                                       int S, int M, int row_words, int commit) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_tracks * S) return;
    float c[5] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (src)
        for (int k = 0; k < 5; ++k) c[k] = src[(size_t)idx * 5 + k];
    if (!commit) {
        bool ok = true;
        for (int k = 0; k < 5; ++k) ok = ok && !not_finite(__float_as_uint(c[k]));
        const double a1 = c[3], a2 = c[4];
        ok = ok && fabs(a2) < 1.0 && fabs(a1) < 1.0 + a2;
        if (!ok) atomicMin(flag, (unsigned)idx);
        return;
    }
    float* row = table + ((size_t)first_track * S + idx) * row_words;
    for (int k = 0; k < 5; ++k) row[k] = c[k];
    // state map per sample on (z1, z2): z1' = -a1 z1 - a2 z2 (+x), z2' = z1
    const double A0 = -(double)c[3], A1 = -(double)c[4];
    double P0 = 1.0, P1 = 0.0, P2 = 0.0, P3 = 1.0;
    for (int i = 0; i < M; ++i) {           // P = A P = A^(i+1); its first row is w[i]'s response to (z1, z2)
        const double n0 = A0 * P0 + A1 * P2, n1 = A0 * P1 + A1 * P3;
        P2 = P0; P3 = P1; P0 = n0; P1 = n1;
        row[5 + i] = (float)(P0 + P1);      // ... to (u, d): z1 = u, z2 = u - d
        row[5 + M + i] = (float)(-P1);
    }
    for (int s = 0; s < 6; ++s) {           // A^M, squared five times; stored as it acts on (u, d): T P T, T = [1 0; 1 -1]
        float* p = row + 5 + 2 * M + 4 * s;
        p[0] = (float)(P0 + P1); p[1] = (float)(-P1);
        p[2] = (float)((P0 + P1) - (P2 + P3)); p[3] = (float)(P3 - P1);
        const double q0 = P0 * P0 + P1 * P2, q1 = P0 * P1 + P1 * P3, q2 = P2 * P0 + P3 * P2, q3 = P2 * P1 + P3 * P3;
        P0 = q0; P1 = q1; P2 = q2; P3 = q3;
    }
    for (int k = 29 + 2 * M; k < row_words; ++k) row[k] = 0.0f;
}

// ---------------------------------------------------------------------------
// The scan form.  One wavefront per track, four tracks per workgroup; a buffer is H segments of 64 M samples, lane l
// owns M consecutive samples of each (iir_scan_kernel's cut and its 16-byte accesses).  All H segments are requested,
// then for every section: local pass from zero state (lane 0 from the section's carried state), six Kogge-Stone steps
// over the outgoing states with the row's powers, homogeneous correction, the three output taps — and the y values
// take the x values' registers: section s's output is section s + 1's input without touching memory.
//   * The track is wave-uniform, so a section's row comes in through scalar loads and costs no vector registers; the
//     next section's row is requested before this section is scanned.  Two rows in flight are 2 (29 + 2M) SGPRs of a
//     wave's 102: M <= 8.
//   * The carried states of the track's sections live in lanes 0..S-1 of two registers for the whole launch (read once,
//     written once): a batch of buffers is more segments of the same scan, and nothing is read back from memory that
//     this launch wrote.
//   * The multiply-adds are fused (fmaf): this form re-associates the recurrence anyway, and the section is bound by
//     its instruction count.
// in == out is allowed: a wave has read all its samples of a buffer before it writes any.
// ---------------------------------------------------------------------------
template <int M, int H>
__global__ __launch_bounds__(256) void eq_scan_kernel(const float* in, float* out, float* __restrict__ state,
                                                     const EqRow<M>* __restrict__ table, int T, int S, int n_buffers) {
    constexpr int SEG = 64 * M;                  // samples per segment
    constexpr int B = SEG * H;
    const int lane = threadIdx.x & 63;
    const int track = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (track >= T) return;
    const EqRow<M>* const rows = table + (size_t)track * S;
    float2* const st = reinterpret_cast<float2*>(state) + (size_t)track * S;
    float st1 = 0.0f, st2 = 0.0f;               // lane s: the state of section s
    if (lane < S) { const float2 v = st[lane]; st1 = v.x; st2 = v.y; }
    for (int n = 0; n < n_buffers; ++n) {
        const size_t base = ((size_t)n * T + track) * B + lane * M;
        const float* x = in + base;
        float xs[H][M];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            if constexpr (M % 4 == 0) {
#pragma unroll
                for (int i = 0; i < M / 4; ++i) {
                    const float4 v = reinterpret_cast<const float4*>(x + h * SEG)[i];
                    xs[h][4 * i] = v.x; xs[h][4 * i + 1] = v.y; xs[h][4 * i + 2] = v.z; xs[h][4 * i + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < M; ++i) xs[h][i] = x[h * SEG + i];
            }
        }
        EqRow<M> next = rows[0];
        for (int s = 0; s < S; ++s) {
            const EqRow<M> k = next;
            next = rows[s + 1 < S ? s + 1 : s];          // in flight while this section is scanned
            // the state entering the segment (uniform)
            float in1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st1), s));
            float in2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st2), s));
#pragma unroll
            for (int h = 0; h < H; ++h) {
                float w[M];
                // 1. local pass
                float z1 = 0.0f, z2 = 0.0f;
                if (lane == 0) { z1 = in1; z2 = in2; }
                const float z1_in0 = z1, z2_in0 = z2;
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const float wv = fmaf(-k.a2, z2, fmaf(-k.a1, z1, xs[h][i]));
                    z2 = z1; z1 = wv; w[i] = wv;
                }
                // 2. inclusive scan of outgoing states, as (u, d) = (z1, z1 - z2): E_l = c_l + A^M E_{l-1}
                float e1 = z1, e2 = z1 - z2;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const int d = 1 << q;
                    const float u1 = __shfl_up(e1, d, 64), u2 = __shfl_up(e2, d, 64);
                    if (lane >= d) {
                        e1 = fmaf(k.p[q][1], u2, fmaf(k.p[q][0], u1, e1));
                        e2 = fmaf(k.p[q][3], u2, fmaf(k.p[q][2], u1, e2));
                    }
                }
                // state entering this lane (lane 0 already started from the carried state)
                float s1 = __shfl_up(e1, 1, 64), s2 = __shfl_up(e2, 1, 64);
                if (lane == 0) { s1 = 0.0f; s2 = 0.0f; }
                // 3. homogeneous correction
#pragma unroll
                for (int i = 0; i < M; ++i) w[i] = fmaf(k.beta[i], s2, fmaf(k.alpha[i], s1, w[i]));
                // 4. output taps need w[n-1], w[n-2]: the previous lane's last two (or the carried state)
                float p1 = __shfl_up(w[M - 1], 1, 64);
                float p2 = (M >= 2) ? __shfl_up(w[M >= 2 ? M - 2 : 0], 1, 64) : __shfl_up(w[0], 2, 64);
                if (lane == 0) { p1 = z1_in0; p2 = z2_in0; }
                if (M == 1 && lane == 1) p2 = in1;       // lane 0's incoming z1
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const float wm1 = (i >= 1) ? w[i - 1] : p1;
                    const float wm2 = (i >= 2) ? w[i - 2] : (i == 1 ? p1 : p2);
                    xs[h][i] = fmaf(k.b2, wm2, fmaf(k.b1, wm1, k.b0 * w[i]));
                }
                // the state leaving the segment: the last lane's last two w
                const float out1 = w[M - 1], out2 = (M >= 2) ? w[M >= 2 ? M - 2 : 0] : p1;
                in1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(out1), 63));
                in2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(out2), 63));
            }
            if (lane == s) { st1 = in1; st2 = in2; }
        }
        float* o = out + base;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            if constexpr (M % 4 == 0) {
#pragma unroll
                for (int i = 0; i < M / 4; ++i)
                    reinterpret_cast<float4*>(o + h * SEG)[i] =
                        make_float4(xs[h][4 * i], xs[h][4 * i + 1], xs[h][4 * i + 2], xs[h][4 * i + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < M; ++i) o[h * SEG + i] = xs[h][i];
            }
        }
    }
    if (lane < S) st[lane] = make_float2(st1, st2);
}

// ---------------------------------------------------------------------------
// The ordered form: iir_biquad_kernel's tiles (64 tracks x 64 samples through LDS, wave 0 owns the recurrences, the
// other three waves fetch the next chunk), every section in turn on the 64-sample chunk a lane holds in registers.
// Operation order and rounding per section are the golden's (cuda/bench_iir.cu:170-197): no fused multiply-adds.
// The sections' states wait in LDS between chunks (a lane's own column: no barrier).  Any bufsize >= 1, any alignment;
// in == out is allowed (a chunk's columns are stored after they were loaded, and no other workgroup has these tracks).
// ---------------------------------------------------------------------------
constexpr int kEqTracks = 64;
constexpr int kEqChunk = 64;
constexpr int kEqPitch = 68;      // row pitch in floats: 16-byte aligned rows, conflict-free b128 access

__global__ __launch_bounds__(256) void eq_sequential_kernel(const float* in, float* out, float* __restrict__ state,
                                                           const float* __restrict__ table, int row_words, int T,
                                                           int B, int S) {
    __shared__ __attribute__((aligned(16))) float tile[2][kEqTracks][kEqPitch];
    __shared__ float zs[kEqMaxSections][2][kEqTracks];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t0 = blockIdx.x * kEqTracks;
    const int my_track = t0 + lane;
    const bool owner = (w == 0) && (my_track < T);
    if (owner) {
        for (int s = 0; s < S; ++s) {
            zs[s][0][lane] = state[((size_t)my_track * S + s) * 2];
            zs[s][1][lane] = state[((size_t)my_track * S + s) * 2 + 1];
        }
    }
    // Row movers: 16 rows per wave, all requests issued before the first is consumed.
    auto load_rows = [&](int buf, int s0, int first, int step) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int r = first + k * step, t = t0 + r, s = s0 + lane;
            v[k] = (r < kEqTracks && t < T && s < B) ? in[(size_t)t * B + s] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int r = first + k * step;
            if (r < kEqTracks) tile[buf][r][lane] = v[k];
        }
    };
    auto store_rows = [&](int buf, int s0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int r = w + 4 * k, t = t0 + r, s = s0 + lane;
            if (t < T && s < B) out[(size_t)t * B + s] = tile[buf][r][lane];
        }
    };
    const int nchunks = (B + kEqChunk - 1) / kEqChunk;
    load_rows(0, 0, w, 4);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1, s0 = ch * kEqChunk;
        const int n = (B - s0) < kEqChunk ? (B - s0) : kEqChunk;     // valid samples in this chunk
        if (w == 0) {
            if (owner) {
                float x[kEqChunk];
                float4* row = reinterpret_cast<float4*>(&tile[buf][lane][0]);
#pragma unroll
                for (int i = 0; i < kEqChunk / 4; ++i) {
                    float4 v = row[i];
                    x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
                }
                for (int s = 0; s < S; ++s) {
                    const float* c = table + ((size_t)my_track * S + s) * row_words;
                    const float b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[3], a2 = c[4];
                    float z1 = zs[s][0][lane], z2 = zs[s][1][lane];
#pragma unroll
                    for (int i = 0; i < kEqChunk; ++i) {
                        if (i < n) {     // wave-uniform: a ragged last chunk must not run on padding
                            float wv = __fsub_rn(__fsub_rn(x[i], __fmul_rn(a1, z1)), __fmul_rn(a2, z2));
                            float y = __fadd_rn(__fadd_rn(__fmul_rn(b0, wv), __fmul_rn(b1, z1)), __fmul_rn(b2, z2));
                            z2 = z1;
                            z1 = wv;
                            x[i] = y;
                        }
                    }
                    zs[s][0][lane] = z1;
                    zs[s][1][lane] = z2;
                }
#pragma unroll
                for (int i = 0; i < kEqChunk / 4; ++i)
                    row[i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
            }
        } else if (ch + 1 < nchunks) {
            // the other three waves fetch the next chunk meanwhile (rows w-1, w+2, ...)
            load_rows(buf ^ 1, s0 + kEqChunk, w - 1, 3);
            load_rows(buf ^ 1, s0 + kEqChunk, w - 1 + 48, 3);
        }
        __syncthreads();
        store_rows(buf, s0);
        __syncthreads();
    }
    if (owner) {
        for (int s = 0; s < S; ++s) {
            state[((size_t)my_track * S + s) * 2] = zs[s][0][lane];
            state[((size_t)my_track * S + s) * 2 + 1] = zs[s][1][lane];
        }
    }
}

// Which scan a plan runs: from (bufsize, sections) alone — never from the track count, so a track's bits do not depend
// on how many other tracks the plan holds.  Up to two sections the launch is bound by its bytes and takes gab_iir's
// tidy accesses (M = 4: a wave's load instruction covers one contiguous KiB); from three sections on it is bound by
// its instructions and takes the longest lane run the scalar registers allow (M = 8: half the scans per sample).
// (0, 0): no scan for this buffer size.
inline void eq_pick_form(int bufsize, int sections, int* M, int* H) {
    *M = 0; *H = 0;
    if (bufsize < 64 || bufsize > 2048 || (bufsize & (bufsize - 1)) != 0) return;
    const int m = bufsize / 64;
    if (m <= 4) { *M = m; *H = 1; return; }
    *M = sections <= 2 ? 4 : 8;
    *H = m / *M;
}

}  // namespace
}  // namespace gab

struct gab_eq_plan {
    int tracks = 0, bufsize = 0, sections = 0;
    int M = 0, H = 0;                  // the scan's form; 0, 0: the sequential kernel only
    int row_words = 0;
    gab::DeviceBuf<float> table;       // [T][S][row_words]
    gab::DeviceBuf<float> state;       // [T][S][2]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

int eq_launch_scan(const gab_eq_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s) {
    const dim3 grid((p->tracks + 3) / 4);
    const int T = p->tracks, S = p->sections;
#define GAB_EQ_SCAN(MV, HV)                                                                                      \
    eq_scan_kernel<MV, HV><<<grid, 256, 0, s>>>(d_in, d_out, p->state.get(),                                    \
                                                reinterpret_cast<const EqRow<MV>*>(p->table.get()), T, S, n_buffers)
    switch (p->M * 16 + p->H) {
        case 1 * 16 + 1: GAB_EQ_SCAN(1, 1); break;
        case 2 * 16 + 1: GAB_EQ_SCAN(2, 1); break;
        case 4 * 16 + 1: GAB_EQ_SCAN(4, 1); break;
        case 4 * 16 + 2: GAB_EQ_SCAN(4, 2); break;
        case 4 * 16 + 4: GAB_EQ_SCAN(4, 4); break;
        case 4 * 16 + 8: GAB_EQ_SCAN(4, 8); break;
        case 8 * 16 + 1: GAB_EQ_SCAN(8, 1); break;
        case 8 * 16 + 2: GAB_EQ_SCAN(8, 2); break;
        case 8 * 16 + 4: GAB_EQ_SCAN(8, 4); break;
        default: return bad_arg("gab_eq_process: the plan has no scan form");
    }
#undef GAB_EQ_SCAN
    return launch_status("eq_scan_kernel");
}

int eq_launch_sequential(const gab_eq_plan* p, const float* d_in, float* d_out, hipStream_t s) {
    const dim3 grid((p->tracks + kEqTracks - 1) / kEqTracks);
    eq_sequential_kernel<<<grid, 256, 0, s>>>(d_in, d_out, p->state.get(), p->table.get(), p->row_words,
                                              p->tracks, p->bufsize, p->sections);
    return launch_status("eq_sequential_kernel");
}

// check, then commit (gab_plan.hpp): a refused set leaves the table as it was.  src null: the identity filter.
int eq_set_range(gab_eq_plan* p, const float* d_coeffs, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const int S = p->sections;
    const long long n = (long long)n_tracks * S;
    auto launch = [&](int commit) {
        eq_consts_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(
            d_coeffs, p->table.get(), p->flag.get(), first_track, n_tracks, S, p->M ? p->M : 1, p->row_words, commit);
    };
    if (d_coeffs) {
        unsigned first_bad = kNoneRefused;
        if (int rc = first_refused(p->flag, s, "eq_consts_kernel", [&] { launch(0); }, &first_bad)) return rc;
        if (first_bad != kNoneRefused) {
            set_last_error(std::string(who) + ": track " + std::to_string(first_track + (int)(first_bad / (unsigned)S)) +
                           " section " + std::to_string((int)(first_bad % (unsigned)S)) +
                           " is unstable (needs |a2| < 1 and |a1| < 1 + a2) or not finite; the plan keeps its coefficients");
            return GAB_ERR_INVALID_ARG;
        }
    }
    launch(1);
    if (int rc = launch_status("eq_consts_kernel")) return rc;
    GAB_HIP_CHECK(hipStreamSynchronize(s));
    return GAB_OK;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_eq_create(gab_eq_plan** out, int tracks, int bufsize, int sections) {
    return gab::create_entry("gab_eq_create", out, tracks, bufsize, [&] {
        if (sections < 1 || sections > gab::kEqMaxSections) return gab::bad_arg("gab_eq_create: sections must be 1..16");
        return GAB_OK;
    }, [&](gab_eq_plan& p) {
        p.sections = sections;
        gab::eq_pick_form(bufsize, sections, &p.M, &p.H);
        p.row_words = gab::eq_row_words(p.M ? p.M : 1);
        const size_t n = (size_t)tracks * sections;
        p.table.alloc(n * p.row_words);
        p.state.alloc(n * 2);
        p.flag.alloc(1);
        GAB_HIP_CHECK(hipMemset(p.state.get(), 0, n * 2 * sizeof(float)));
        return gab::eq_set_range(&p, nullptr, 0, tracks, "gab_eq_create", nullptr);      // identity
    });
}

int gab_eq_destroy(gab_eq_plan* plan) { return gab::destroy_plan(plan, "gab_eq_destroy: null plan"); }

int gab_eq_set_coeffs_tracks(gab_eq_plan* plan, const float* d_coeffs, int first_track, int n_tracks, gab_stream_t stream) {
    return gab::set_entry("gab_eq_set_coeffs_tracks", gab::eq_set_range, plan, d_coeffs, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_eq_set_coeffs(gab_eq_plan* plan, const float* d_coeffs, gab_stream_t stream) {
    return gab::set_entry("gab_eq_set_coeffs", gab::eq_set_range, plan, d_coeffs, true, 0, 0, gab::as_stream(stream));
}

int gab_eq_reset(gab_eq_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_eq_reset", {plan}, [&] {
        GAB_HIP_CHECK(hipMemsetAsync(plan->state.get(), 0, plan->state.size() * sizeof(float), gab::as_stream(stream)));
        return GAB_OK;
    }, "null plan");
}

int gab_eq_process_sequential(gab_eq_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_eq_process_sequential", {plan, d_in, d_out},
                      [&] { return gab::eq_launch_sequential(plan, d_in, d_out, gab::as_stream(stream)); });
}

int gab_eq_process(gab_eq_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_eq_process", {plan, d_in, d_out}, [&] {
        if (plan->M == 0 || !gab::all_aligned16({d_in, d_out}))
            return gab::eq_launch_sequential(plan, d_in, d_out, gab::as_stream(stream));
        return gab::eq_launch_scan(plan, d_in, d_out, 1, gab::as_stream(stream));
    });
}

int gab_eq_process_batch(gab_eq_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_eq_process_batch", {plan, d_in, d_out}, n_buffers, [&]() -> int {
        if (plan->M != 0 && gab::all_aligned16({d_in, d_out}))
            return gab::eq_launch_scan(plan, d_in, d_out, n_buffers, gab::as_stream(stream));
        // no scan for this shape: the ordered kernel, one launch per buffer
        const size_t stride = (size_t)plan->tracks * plan->bufsize;
        for (int n = 0; n < n_buffers; ++n)
            if (int rc = gab::eq_launch_sequential(plan, d_in + n * stride, d_out + n * stride, gab::as_stream(stream)))
                return rc;
        return GAB_OK;
    });
}

int gab_eq_state(gab_eq_plan* plan, float** d_state, size_t* n_floats) {
    return gab::entry("gab_eq_state", {plan, d_state, n_floats}, [&] {
        *d_state = plan->state.get();
        *n_floats = plan->state.size();
        return GAB_OK;
    });
}

int gab_eq_form(const gab_eq_plan* plan, int* samples_per_lane, int* segments) {
    return gab::entry("gab_eq_form", {plan, samples_per_lane, segments}, [&] {
        *samples_per_lane = plan->M;
        *segments = plan->H;
        return GAB_OK;
    });
}

}  // extern "C"
