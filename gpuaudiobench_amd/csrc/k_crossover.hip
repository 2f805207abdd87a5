// k_crossover.hip — the crossover plan: a Linkwitz-Riley (fourth-order) split of every track into K = 2..4 bands, made
// of trapezoidal state-variable sections whose arithmetic the header fixes (include/gab_c_api.h, gab_xover_*).  No
// counterpart in the reference.
//
//   xover_kernel<K, VEC>   a workgroup is ONE wave and owns 64 / G tracks for the whole launch, every buffer of a batch
//                          included; G = 1, 2, 4 for K = 2, 3, 4.  The G lanes of a track are the STAGES of a pipeline,
//                          lane q of a track being split q: it runs A_q, B_q and C_q and the compensating all-passes
//                          D_{i,q}, i < q, all on split q's row, so every lane runs the same program (three sections
//                          and S - 1 all-pass slots, of which q are real).  Stage q works on sample n - q while stage 0
//                          works on n; what it needs of stage q - 1 (r_q and the lows so far) comes from the lane before
//                          it by a DPP row shift, once a step.  (K = 4: three stages in quads, the fourth lane idle.)
//                          The wave walks the stream in chunks of 64 samples:
//                            0. the NEXT chunk's loads are issued, into registers of their own;
//                            1. the chunk held in registers goes into the input tile, a lane per 4 samples of a row;
//                            2. the steps: 64 + S - 1 of them (the pipeline is drained at the end of every chunk, so a
//                               chunk's bands are whole when it is stored), stage 0 reading its track's row of the input
//                               tile, stage S - 1 writing the K band tiles;
//                            3. the band tiles go out, a lane per 4 samples of a row.
//                          The block is read once and K blocks are written.  Nothing meets at a barrier.
//   XoverRule              refuses a row that is no g > 0's row, naming the first (gab_plan.hpp's check kernel).
//
// Every section is a deterministic recurrence of its own input, so which lane runs it and when decides no bit; the
// sequence of roundings is the header's.  Why this cut: DESIGN.md §4j.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kXoverChunk = 64;           // samples of a chunk
constexpr int kXoverPitch = 65;           // row pitch in words: odd, so that a column of rows and a row's words are both
                                          // spread over the banks (every LDS access here is one word wide)
constexpr float kXoverK = GAB_XOVER_K32;  // the section's damping, (float)sqrt(2)
constexpr float kXoverK2 = 2.0f * GAB_XOVER_K32;

constexpr int xover_sections(int bands) { return 3 * (bands - 1) + (bands - 1) * (bands - 2) / 2; }
constexpr int xover_group(int bands) { return bands == 2 ? 1 : bands == 3 ? 2 : 4; }
// The first section of split j in the state array: A_j, B_j, C_j, D_{j,j+1} .. D_{j,S-1}, split after split.
constexpr int xover_base(int bands, int j) { return j == 0 ? 0 : xover_base(bands, j - 1) + 3 + (bands - 2 - (j - 1)); }

// A hand-off through LDS inside the wave (k_gate.hip's).
__device__ __forceinline__ void xover_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The point at which a load must have landed (k_gate.hip's).
__device__ __forceinline__ void xover_landed(float& v) { asm volatile("" : "+v"(v)); }

// The value of the lane before this one in its row of 16 lanes; 0 in a row's first lane (which is a stage 0).
__device__ __forceinline__ float xover_from_before(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}

struct XoverSection {
    float ic1, ic2;
};

// One sample of one section, the header's sequence: v1 (band) and v2 (low) out, the state moved on.
__device__ __forceinline__ void xover_step(XoverSection& s, float a1, float a2, float a3, float v0, float& v1, float& v2) {
    const float v3 = __fsub_rn(v0, s.ic2);
    v1 = fmaf(a2, v3, __fmul_rn(a1, s.ic1));
    v2 = fmaf(a3, v3, fmaf(a2, s.ic1, s.ic2));
    s.ic1 = fmaf(2.0f, v1, -s.ic1);
    s.ic2 = fmaf(2.0f, v2, -s.ic2);
}

__device__ __forceinline__ float xover_high(float v0, float v1, float v2) { return __fsub_rn(fmaf(-kXoverK, v1, v0), v2); }

// Grid: x = group of 64 / G tracks, one wave.  in: [n][T][B]; out: [n][K][T][B], no overlap with in.  state:
// [T][sections][2]; rows: [T][S][3].  VEC: both blocks 16-byte aligned and B a multiple of 4.
template <int K, bool VEC>
__global__ __launch_bounds__(64) void xover_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                   float* __restrict__ state, const float* __restrict__ rows, int T, int B,
                                                   int n_buffers) {
    constexpr int S = K - 1, G = xover_group(K), TW = 64 / G, NSEC = xover_sections(K), ND = S > 1 ? S - 1 : 1;
    constexpr int NR = TW / 4;                                        // rows of a lane in the pointwise phases
    // Band 0's tile is the input's: column n of a row is read (by stage 0, a step ahead) before it is written (by stage
    // S - 1, S - 1 steps behind), and what is written there is computed from what was read there, through the lanes
    // between: the order of the two is a data dependence, not a matter of scheduling.
    constexpr int TILES = K, IN_TILE = 0;
    __shared__ float tile[TILES][TW][kXoverPitch];
    const int lane = threadIdx.x;
    const int tr = lane / G, q = lane % G;                            // the lane's track within the wave, its stage
    const int t0 = blockIdx.x * TW;
    const int track = t0 + tr;
    const bool staged = q < S;                                        // (K = 4: the fourth lane of a quad has no stage)
    const bool owner = staged && track < T;
    const size_t tc = (size_t)(track < T ? track : T - 1);            // a lane without a track: the last one's, never stored

    // ---- the lane's sections and its row ----
    XoverSection sa = {0.0f, 0.0f}, sb = {0.0f, 0.0f}, sc = {0.0f, 0.0f}, sd[ND];
    int d_at[ND];                                                     // where D_{i,q} sits in the track's state
    float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    int base_q = 0;
#pragma unroll
    for (int j = 0; j < S; ++j)
        if (q == j) base_q = xover_base(K, j);
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        sd[i] = {0.0f, 0.0f};
        d_at[i] = xover_base(K, i) + 3 + (q - i - 1);
    }
    float* const st = state + tc * NSEC * 2;
    if (owner) {
        const float* row = rows + (tc * S + q) * 3;
        a1 = row[0]; a2 = row[1]; a3 = row[2];
        sa = {st[2 * base_q], st[2 * base_q + 1]};
        sb = {st[2 * base_q + 2], st[2 * base_q + 3]};
        sc = {st[2 * base_q + 4], st[2 * base_q + 5]};
#pragma unroll
        for (int i = 0; i < ND; ++i)
            if (S > 1 && i < q) sd[i] = {st[2 * d_at[i]], st[2 * d_at[i] + 1]};
    }
    xover_landed(a1); xover_landed(a2); xover_landed(a3);
    xover_landed(sa.ic1); xover_landed(sa.ic2); xover_landed(sb.ic1); xover_landed(sb.ic2);
    xover_landed(sc.ic1); xover_landed(sc.ic2);
#pragma unroll
    for (int i = 0; i < ND; ++i) { xover_landed(sd[i].ic1); xover_landed(sd[i].ic2); }

    // ---- the pointwise phases: the lane's rows 4 it + (lane / 16), its four samples 4 (lane % 16) + j ----
    const int pr = lane >> 4, pc = (lane & 15) * 4;
    size_t row_at[NR];
    bool row_live[NR];
#pragma unroll
    for (int it = 0; it < NR; ++it) {
        const int t = t0 + 4 * it + pr;
        row_live[it] = t < T;
        row_at[it] = (size_t)(t < T ? t : T - 1) * B;
    }
    // Every load is unconditional, so that all of them are in flight before the first is used: a row below the last
    // track reads the last track's, a sample behind the buffer's end the chunk's first.  Such a value is never stored
    // and enters no recurrence of a track that exists.
    auto load = [&](float (&v)[NR][4], const float* x, int s0) {
        const int len = B - s0 < kXoverChunk ? B - s0 : kXoverChunk;
        const int qc = pc < len ? pc : 0;                             // VEC: len is a multiple of 4
#pragma unroll
        for (int it = 0; it < NR; ++it) {
            const size_t at = row_at[it] + s0;
            if constexpr (VEC) {
                const float4 f = *reinterpret_cast<const float4*>(x + at + qc);
                v[it][0] = f.x; v[it][1] = f.y; v[it][2] = f.z; v[it][3] = f.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[it][j] = x[at + (pc + j < len ? pc + j : 0)];
            }
        }
    };
    auto landed = [&](float (&v)[NR][4]) {
#pragma unroll
        for (int it = 0; it < NR; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) xover_landed(v[it][j]);
    };

    const size_t block = (size_t)T * B;
    float r_out = 0.0f, low_out[ND];                                  // what the next stage takes, a step later
#pragma unroll
    for (int i = 0; i < ND; ++i) low_out[i] = 0.0f;
    float ch[NR][4], nx[NR][4];
    load(ch, in, 0);
    landed(ch);
    for (int nb = 0; nb < n_buffers; ++nb) {
        const float* x = in + nb * block;
        float* y = out + (size_t)nb * K * block;
        for (int s0 = 0; s0 < B; s0 += kXoverChunk) {
            const int len = B - s0 < kXoverChunk ? B - s0 : kXoverChunk;
            // ---- 0. the next chunk's loads, of this buffer or of the next ----
            if (s0 + kXoverChunk < B) load(nx, x, s0 + kXoverChunk);
            else if (nb + 1 < n_buffers) load(nx, x + block, 0);
            // ---- 1. the chunk into the input tile ----
#pragma unroll
            for (int it = 0; it < NR; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) tile[IN_TILE][4 * it + pr][pc + j] = ch[it][j];
            xover_wave_order();
            // ---- 2. the steps: stage q takes sample step - q ----
            // (stage 0 reads the sample of the step after this one before it works on this one's: the read's latency
            // is then behind a step's arithmetic and not in front of it)
            float x_cur = 0.0f;
            if (q == 0) x_cur = tile[IN_TILE][tr][0];
            for (int step = 0; step < len + S - 1; ++step) {
                float r_in = 0.0f, low_in[ND], x_next = 0.0f;
                if (q == 0 && step + 1 < len) x_next = tile[IN_TILE][tr][step + 1];
                if constexpr (G > 1) {                                // outside the branch below: every lane takes part
                    r_in = xover_from_before(r_out);
#pragma unroll
                    for (int i = 0; i < ND; ++i) low_in[i] = xover_from_before(low_out[i]);
                }
                const int n = step - q;
                if (staged && (unsigned)n < (unsigned)len) {
                    if (q == 0) r_in = x_cur;
                    float bp, l, lq, h;
                    xover_step(sa, a1, a2, a3, r_in, bp, l);
                    h = xover_high(r_in, bp, l);
                    xover_step(sb, a1, a2, a3, l, bp, lq);
                    float cb, cl;
                    xover_step(sc, a1, a2, a3, h, cb, cl);
                    r_out = xover_high(h, cb, cl);
                    if constexpr (S > 1) {
#pragma unroll
                        for (int i = 0; i < ND; ++i) {
                            // slot i: real on stages behind split i; stage i puts its own low there; the rest is unused
                            float db, dl;
                            XoverSection d = sd[i];
                            xover_step(d, a1, a2, a3, low_in[i], db, dl);
                            const bool real = i < q;
                            sd[i].ic1 = real ? d.ic1 : sd[i].ic1;
                            sd[i].ic2 = real ? d.ic2 : sd[i].ic2;
                            low_out[i] = real ? fmaf(-kXoverK2, db, low_in[i]) : lq;
                        }
                    }
                    if (q == S - 1) {
#pragma unroll
                        for (int i = 0; i < S - 1; ++i) tile[i][tr][n] = low_out[i];
                        tile[S - 1][tr][n] = lq;
                        tile[S][tr][n] = r_out;
                    }
                }
                x_cur = x_next;
            }
            xover_wave_order();
            // ---- 3. the bands out; the next chunk's loads are waited for in front of the stores (k_gate.hip) ----
            landed(nx);
#pragma unroll
            for (int b = 0; b < K; ++b) {
                float* yb = y + (size_t)b * block + s0 + pc;
#pragma unroll
                for (int it = 0; it < NR; ++it) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = tile[b][4 * it + pr][pc + j];
                    if constexpr (VEC) {
                        if (row_live[it] && pc < len) *reinterpret_cast<float4*>(yb + row_at[it]) = make_float4(o[0], o[1], o[2], o[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (row_live[it] && pc + j < len) yb[row_at[it] + j] = o[j];
                    }
                }
            }
            xover_wave_order();                                       // the tiles are free for the next chunk
#pragma unroll
            for (int it = 0; it < NR; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) ch[it][j] = nx[it][j];
        }
    }
    if (owner) {
        st[2 * base_q] = sa.ic1; st[2 * base_q + 1] = sa.ic2;
        st[2 * base_q + 2] = sb.ic1; st[2 * base_q + 3] = sb.ic2;
        st[2 * base_q + 4] = sc.ic1; st[2 * base_q + 5] = sc.ic2;
#pragma unroll
        for (int i = 0; i < ND; ++i)
            if (S > 1 && i < q) { st[2 * d_at[i]] = sd[i].ic1; st[2 * d_at[i] + 1] = sd[i].ic2; }
    }
}

const char* const kXoverFields[GAB_XOVER_FIELDS] = {"a1", "a2", "a3"};
const char* const kXoverRules[GAB_XOVER_FIELDS] = {
    "must be within (0, 1]", "must be within [0, 1)",
    "must be within [0, 1), with a1 + K32 a2 + a3 within 2^-20 of 1 and a2 a2 within 2^-18 of a1 a3: the row of some g"};

// src: [n_rows][3] (a NaN fails every comparison).  a3 is held against the a1 and a2 of its own row, the two before it.
struct XoverRule {
    __device__ bool refuses(const float* src, size_t i) const {
        const float v = src[i];
        const int field = (int)(i % GAB_XOVER_FIELDS);
        bool bad = not_finite(__float_as_uint(v));
        if (field == 0) bad = bad || !(v > 0.0f && v <= 1.0f);
        if (field == 1) bad = bad || !(v >= 0.0f && v < 1.0f);
        if (field == 2) {
            const float a1 = src[i - 2], a2 = src[i - 1];
            bad = bad || !(v >= 0.0f && v < 1.0f);
            bad = bad || !(fabsf(__fsub_rn(__fadd_rn(fmaf(kXoverK, a2, a1), v), 1.0f)) <= 0x1p-20f);
            bad = bad || !(fabsf(fmaf(a2, a2, -__fmul_rn(a1, v))) <= __fmul_rn(0x1p-18f, __fmul_rn(a2, a2)));
        }
        return bad;
    }
    std::string refusal(unsigned i, int first_track) const {
        // a row here is a track's S splits: the field named is the value's place in it, (split, a) = (field / 3, field % 3)
        const int field = (int)(i % GAB_XOVER_FIELDS);
        return row_refusal(i, row, first_track, kXoverFields[field], kXoverRules[field]);
    }
    unsigned row;                                                     // 3 S: the values of a track
};

}  // namespace
}  // namespace gab

struct gab_xover_plan {
    int tracks = 0, bufsize = 0, bands = 0;
    bool have_rows = false;            // a set has been accepted
    gab::DeviceBuf<float> rows;        // [T][S][3]
    gab::DeviceBuf<float> state;       // [T][sections][2]
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// n buffers in one launch.  Nothing is allocated and nothing waits here.
int xover_process(gab_xover_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    if (!p->have_rows) return refuse(who, "no splits have been set: gab_xover_set_splits comes first");
    const size_t in_floats = (size_t)n_buffers * p->tracks * p->bufsize;
    // the two blocks differ in length: do [d_in, +n) and [d_out, +K n) share a byte?
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (a < b + in_floats * p->bands * sizeof(float) && b < a + in_floats * sizeof(float))
        return refuse(who, "d_out may not overlap d_in");
    const bool vec = all_aligned16({d_in, d_out}) && p->bufsize % 4 == 0;
    const int tw = 64 / xover_group(p->bands);
    const dim3 grid((unsigned)((p->tracks + tw - 1) / tw));
#define GAB_XOVER(KK)                                                                                              \
    do {                                                                                                           \
        if (vec) xover_kernel<KK, true><<<grid, 64, 0, s>>>(d_in, d_out, p->state.get(), p->rows.get(), p->tracks, \
                                                            p->bufsize, n_buffers);                                \
        else xover_kernel<KK, false><<<grid, 64, 0, s>>>(d_in, d_out, p->state.get(), p->rows.get(), p->tracks,    \
                                                         p->bufsize, n_buffers);                                   \
    } while (0)
    switch (p->bands) {
        case 2: GAB_XOVER(2); break;
        case 3: GAB_XOVER(3); break;
        default: GAB_XOVER(4); break;
    }
#undef GAB_XOVER
    return launch_status("xover_kernel");
}

// check, then commit (gab_plan.hpp): a refused set leaves the table as it was.  The state is kept: it is the
// integrators' own and means the same under any row.
int xover_set_range(gab_xover_plan* p, const float* d_rows, int first_track, int n_tracks, const char* who, hipStream_t s) {
    const size_t per_track = (size_t)(p->bands - 1) * GAB_XOVER_FIELDS;
    const size_t n = (size_t)n_tracks * per_track;
    return check_then(p->flag, s, who, d_rows, n, XoverRule{(unsigned)per_track}, first_track, [&] {
        GAB_HIP_CHECK(hipMemcpyAsync(p->rows.get() + (size_t)first_track * per_track, d_rows, n * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
        GAB_HIP_CHECK(hipStreamSynchronize(s));
        // before the first whole set a ranged one leaves rows that were never given: {1, 0, 0}, the row of g = 0
        p->have_rows = true;
    });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_xover_sections(int bands) { return bands < 2 || bands > 4 ? 0 : gab::xover_sections(bands); }

int gab_xover_create(gab_xover_plan** out, int tracks, int bufsize, int bands) {
    return gab::create_entry("gab_xover_create", out, tracks, bufsize, [&] {
        if (bands < 2 || bands > 4) return gab::bad_arg("gab_xover_create: bands must be 2..4");
        return GAB_OK;
    }, [&](gab_xover_plan& p) {
        p.bands = bands;
        p.rows.alloc((size_t)tracks * (bands - 1) * GAB_XOVER_FIELDS);
        p.state.alloc((size_t)tracks * gab::xover_sections(bands) * 2);
        p.flag.alloc(1);
        std::vector<float> init;
        for (size_t i = 0; i < p.rows.size(); i += GAB_XOVER_FIELDS) init.insert(init.end(), {1.0f, 0.0f, 0.0f});
        GAB_HIP_CHECK(hipMemcpy(p.rows.get(), init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
        GAB_HIP_CHECK(hipMemset(p.state.get(), 0, p.state.size() * sizeof(float)));
        return GAB_OK;
    });
}

int gab_xover_destroy(gab_xover_plan* plan) { return gab::destroy_plan(plan, "gab_xover_destroy: null pointer"); }

int gab_xover_set_splits(gab_xover_plan* plan, const float* d_rows, gab_stream_t stream) {
    return gab::set_entry("gab_xover_set_splits", gab::xover_set_range, plan, d_rows, true, 0, 0, gab::as_stream(stream));
}

int gab_xover_set_splits_tracks(gab_xover_plan* plan, const float* d_rows, int first_track, int n_tracks,
                                gab_stream_t stream) {
    return gab::set_entry("gab_xover_set_splits_tracks", gab::xover_set_range, plan, d_rows, false, first_track, n_tracks,
                          gab::as_stream(stream));
}

int gab_xover_reset(gab_xover_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_xover_reset", {plan}, [&] {
        GAB_HIP_CHECK(hipMemsetAsync(plan->state.get(), 0, plan->state.size() * sizeof(float), gab::as_stream(stream)));
        return GAB_OK;
    });
}

int gab_xover_process(gab_xover_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_xover_process", {plan, d_in, d_out}, [&] {
        return gab::xover_process(plan, d_in, d_out, 1, gab::as_stream(stream), "gab_xover_process");
    });
}

int gab_xover_process_batch(gab_xover_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_xover_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::xover_process(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_xover_process_batch");
    });
}

int gab_xover_splits(gab_xover_plan* plan, float** d_rows, size_t* n_floats) {
    return gab::entry("gab_xover_splits", {plan, d_rows, n_floats}, [&] {
        *d_rows = plan->rows.get();
        *n_floats = plan->rows.size();
        return GAB_OK;
    });
}

int gab_xover_state(gab_xover_plan* plan, float** d_state, size_t* n_floats) {
    return gab::entry("gab_xover_state", {plan, d_state, n_floats}, [&] {
        *d_state = plan->state.get();
        *n_floats = plan->state.size();
        return GAB_OK;
    });
}

}  // extern "C"
