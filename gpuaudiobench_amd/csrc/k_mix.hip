// k_mix.hip — the mix bus: `tracks` channels summed into `buses` buses with a gain per (track, bus) that can be ramped
// over one buffer, in a summation order that is a function of the indices alone (include/gab_c_api.h, gab_mix_*).
// No counterpart in the reference, whose kernels are per track.
//
//   mix_kernel<V, MT, SM>   a wave owns one leaf: a chain of leaf_tracks fused multiply-adds per output on 64 V samples
//                           of MT buses, the track's gains in scalar registers; a workgroup owns one group: its waves'
//                           leaves meet in LDS and are added in ascending order.  SM: sample-major input, turned
//                           through a 256-track x 64-sample LDS tile first, then the same chains.
//   mix_groups_kernel       the final pass: the groups' partial sums, fetched side by side, added in ascending order (not launched when the
//                           plan has one group: the workgroup's sums are the outputs).
//   MixRule                 refuses a gain that is not finite, naming the first (gab_plan.hpp's check kernel).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <memory>
#include <string>

#include "gab_plan.hpp"

namespace gab {
namespace {

constexpr int kMixMaxBuses = 64;
constexpr int kMixGroupTracks = 256;      // leaf_tracks * group_leaves, whatever the form
constexpr int kMixBatchChunk = 64;        // buffers of a batch per launch, at most

// The form: from (bufsize, buses) alone.  A group is always 256 tracks, one workgroup.  Up to 32 buses it is eight
// waves with a leaf of 32 tracks each; above, a lane's accumulators (one per bus) and the LDS the leaves meet in
// (group_leaves x buses x 64 samples) allow four waves, so the leaf is 64 tracks.  bufsize does not enter.
constexpr int mix_leaf_tracks(int buses) { return buses > 32 ? 64 : 32; }
inline void mix_pick_form(int /*bufsize*/, int buses, int* leaf_tracks, int* group_leaves) {
    *leaf_tracks = mix_leaf_tracks(buses);
    *group_leaves = kMixGroupTracks / *leaf_tracks;
}

template <int V>
__device__ __forceinline__ void mix_load(float (&x)[V], const float* p, bool live) {
    if constexpr (V == 4) {
        const float4 v = live ? *reinterpret_cast<const float4*>(p) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else if constexpr (V == 2) {
        const float2 v = live ? *reinterpret_cast<const float2*>(p) : make_float2(0.0f, 0.0f);
        x[0] = v.x; x[1] = v.y;
    } else {
        x[0] = live ? *p : 0.0f;
    }
}

// One track into the lane's chains.  tg / cg: the track's rows of target and current (wave-uniform: scalar loads).
// EXACT: the plan's bus count is the tile's.  Otherwise the tile's other buses get zero gains; their chains are never
// stored.
template <int V, int MT, bool RAMP, bool EXACT>
__device__ __forceinline__ void mix_track(float (&acc)[V][MT], const float (&x)[V], const float* __restrict__ tg,
                                          const float* __restrict__ cg, int M, const float (&rv)[V]) {
    float g[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) g[m] = (EXACT || m < M) ? tg[m] : 0.0f;
    if constexpr (RAMP) {
        float c[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) c[m] = (EXACT || m < M) ? cg[m] : 0.0f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float d = __fsub_rn(g[m], c[m]);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v][m] = fmaf(fmaf(d, rv[v], c[m]), x[v], acc[v][m]);
        }
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v][m] = fmaf(g[m], x[v], acc[v][m]);
    }
}

// The leaf: nt tracks in ascending order.  xp: the lane's first sample of the leaf's first track, xstride floats from
// one track to the next.  With the tile's own bus count, U loads are requested before the first is consumed; any other
// bus count takes the plain loop (its guarded gain loads, unrolled, are most of a megabyte of code).
template <int V, int MT, bool RAMP, int U>
__device__ __forceinline__ void mix_chain(float (&acc)[V][MT], const float* xp, size_t xstride, int nt,
                                          const float* __restrict__ tg, const float* __restrict__ cg, int M,
                                          const float (&rv)[V], bool live) {
    if (M != MT) {
        for (int j = 0; j < nt; ++j) {
            float x1[V];
            mix_load<V>(x1, xp + (size_t)j * xstride, live);
            mix_track<V, MT, RAMP, false>(acc, x1, tg + (size_t)j * M, cg + (size_t)j * M, M, rv);
        }
        return;
    }
    int j = 0;
    for (; j + U <= nt; j += U) {
        float xs[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) mix_load<V>(xs[u], xp + (size_t)(j + u) * xstride, live);
#pragma unroll
        for (int u = 0; u < U; ++u)
            mix_track<V, MT, RAMP, true>(acc, xs[u], tg + (size_t)(j + u) * MT, cg + (size_t)(j + u) * MT, MT, rv);
    }
    for (; j < nt; ++j) {
        float x1[V];
        mix_load<V>(x1, xp + (size_t)j * xstride, live);
        mix_track<V, MT, RAMP, true>(acc, x1, tg + (size_t)j * MT, cg + (size_t)j * MT, MT, rv);
    }
}

// ---------------------------------------------------------------------------
// Grid: x = column (64 V samples) + n_cols * group (256 tracks), z = buffer of a batch.  Wave w of the workgroup owns
// leaf w of the group.  dst: [n][n_groups][M][B] — the partial sums, or with one group the outputs themselves.
// ramp_first: the batch's first buffer is mixed with g = fmaf(target - current, r[s], current).
//   V > 1 needs in 4 V-byte aligned and B a multiple of V; V = 1 takes any shape and any alignment.
//   SM (V = 1): in is [s*T + t].  The workgroup's 64 samples x 256 tracks come in as rows of 256 consecutive tracks and
//   are written to LDS track by track (tile[t][s ^ (t & 63)]: both the writes, 64 tracks of one sample, and the reads,
//   64 samples of one track, touch 64 banks); the chains then read LDS where the track-major form reads memory.
// ---------------------------------------------------------------------------
template <int V, int MT, bool SM>
__global__ __launch_bounds__(kMixGroupTracks / mix_leaf_tracks(MT) * 64) void mix_kernel(
    const float* __restrict__ in, float* __restrict__ dst, const float* __restrict__ cur, const float* __restrict__ tgt,
    const float* __restrict__ ramp, int T, int B, int M, int n_cols, int n_groups, int ramp_first) {
    constexpr int L = mix_leaf_tracks(MT), G = kMixGroupTracks / L, W = 64 * V, NT = 64 * G;
    constexpr int kComb = G * MT * W, kTile = SM ? kMixGroupTracks * 64 : 0;
    static_assert(!SM || V == 1, "the turned form owns one sample per lane");
    __shared__ __attribute__((aligned(16))) float lds[kComb > kTile ? kComb : kTile];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = blockIdx.x % n_cols, grp = blockIdx.x / n_cols, n = blockIdx.z;
    const int s0 = col * W, t0 = grp * kMixGroupTracks;
    const float* x = in + (size_t)n * T * B;
    const int sl = lane * V;
    const bool live = s0 + sl < B;
    const int t_begin = t0 + w * L;
    const int nt = T - t_begin < L ? (T - t_begin > 0 ? T - t_begin : 0) : L;

    if constexpr (SM) {
#pragma unroll 8
        for (int e = threadIdx.x; e < kTile; e += NT) {
            const int ss = e >> 8, tt = e & 255;
            const bool ok = s0 + ss < B && t0 + tt < T;
            lds[tt * 64 + (ss ^ (tt & 63))] = ok ? x[(size_t)(s0 + ss) * T + t0 + tt] : 0.0f;
        }
        __syncthreads();
    }

    float acc[V][MT];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[v][m] = 0.0f;
    float rv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) rv[v] = 0.0f;

    if (nt > 0) {
        const float* tg = tgt + (size_t)t_begin * M;
        const float* cg = cur + (size_t)t_begin * M;
        if constexpr (SM) {
            // lane = sample: track tt's row starts at tt * 64, the lane's word in it is lane ^ (tt & 63)
            const bool ramping = ramp_first && n == 0;
            if (ramping && live) rv[0] = ramp[s0 + sl];
            for (int j = 0; j < nt; ++j) {
                const int tt = w * L + j;
                const float x1[1] = {lds[tt * 64 + (lane ^ (tt & 63))]};
                const float* tj = tg + (size_t)j * M;
                const float* cj = cg + (size_t)j * M;
                if (M == MT) {
                    if (ramping) mix_track<1, MT, true, true>(acc, x1, tj, cj, M, rv);
                    else mix_track<1, MT, false, true>(acc, x1, tj, cj, M, rv);
                } else {
                    if (ramping) mix_track<1, MT, true, false>(acc, x1, tj, cj, M, rv);
                    else mix_track<1, MT, false, false>(acc, x1, tj, cj, M, rv);
                }
            }
        } else {
            constexpr int U = (V == 1 && MT <= 16) ? 16 : 8;
            const float* xp = x + (size_t)t_begin * B + s0 + sl;
            if (ramp_first && n == 0) {
                if (live)
#pragma unroll
                    for (int v = 0; v < V; ++v) rv[v] = ramp[s0 + sl + v];
                mix_chain<V, MT, true, U>(acc, xp, (size_t)B, nt, tg, cg, M, rv, live);
            } else {
                mix_chain<V, MT, false, U>(acc, xp, (size_t)B, nt, tg, cg, M, rv, live);
            }
        }
    }
    if constexpr (SM) __syncthreads();       // every wave has read its tracks: the tile's words become the leaves'

    // the leaves meet: comb[leaf][bus][sample]
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int v = 0; v < V; ++v) lds[(w * MT + m) * W + sl + v] = acc[v][m];
    __syncthreads();
    const int t_end = T - t0 < kMixGroupTracks ? T - t0 : kMixGroupTracks;      // tracks of this group
    const int n_leaves = (t_end + L - 1) / L;
    float* out = dst + ((size_t)n * n_groups + grp) * M * B;
    for (int e = threadIdx.x; e < M * W; e += NT) {
        const int m = e / W, s = e % W;
        float sum = lds[m * W + s];
        for (int j = 1; j < n_leaves; ++j) sum = __fadd_rn(sum, lds[(j * MT + m) * W + s]);
        if (s0 + s < B) out[(size_t)m * B + s0 + s] = sum;
    }
}

// The final pass: out[n][m][s] = the groups' sums in ascending order, from the first group's value.  The adds of one
// output are a chain, but the loads are not: a workgroup of sixteen waves owns 64 outputs, every wave fetches rows of
// 64 partial sums (up to 128 rows in flight per workgroup) into LDS, and wave 0 adds them in order from there.  One
// thread per output walking its column took 64 us at 65 536 tracks (256 dependent round trips to memory).
constexpr int kMixRows = 128;       // rows of partial sums per pass through LDS
__global__ __launch_bounds__(1024) void mix_groups_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                         size_t MB, int n_groups, size_t total) {
    __shared__ float rows[kMixRows][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t e = (size_t)blockIdx.x * 64 + lane;
    const bool valid = e < total;
    const size_t n = valid ? e / MB : 0, r = valid ? e % MB : 0;
    const float* p = part + n * n_groups * MB + r;
    float sum = 0.0f;
    for (int g0 = 0; g0 < n_groups; g0 += kMixRows) {
        const int cnt = n_groups - g0 < kMixRows ? n_groups - g0 : kMixRows;
        float v[kMixRows / 16];
#pragma unroll
        for (int k = 0; k < kMixRows / 16; ++k) {
            const int g = w + 16 * k;
            v[k] = (valid && g < cnt) ? p[(size_t)(g0 + g) * MB] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kMixRows / 16; ++k) rows[w + 16 * k][lane] = v[k];
        __syncthreads();
        if (w == 0) {
            int g = 0;
            if (g0 == 0) { sum = rows[0][lane]; g = 1; }
            for (; g < cnt; ++g) sum = __fadd_rn(sum, rows[g][lane]);
        }
        __syncthreads();
    }
    if (w == 0 && valid) out[e] = sum;
}

// src: [n_rows][buses]
struct MixRule {
    unsigned buses;                 // for the text only
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int first_track) const {
        return "the gain of track " + std::to_string(first_track + (int)(i / buses)) + " bus " +
               std::to_string((int)(i % buses)) + " is not finite; the plan keeps its gains";
    }
};

}  // namespace
}  // namespace gab

struct gab_mix_plan {
    int tracks = 0, bufsize = 0, buses = 0;
    int leaf_tracks = 0, group_leaves = 0;
    int n_groups = 0;
    gab::RampedTable gains;            // current, target: [T][M]
    gab::DeviceBuf<float> part;        // [part_buffers][n_groups][M][B]: the groups' partial sums (n_groups > 1 only)
    int part_buffers = 0;              // fixed at creation: how many buffers of a batch one launch takes
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

int mix_tile(int buses) {
    int mt = 1;
    while (mt < buses) mt *= 2;
    return mt;
}

// n buffers (at most part_buffers) in one launch of mix_kernel, then the final pass if the plan has more than one group.
// Nothing is allocated and nothing waits here: the calls can be captured into a graph.
int mix_launch(gab_mix_plan* p, const float* d_in, float* d_out, int n, int layout, bool ramp_first, hipStream_t s) {
    const int T = p->tracks, B = p->bufsize, M = p->buses, MT = mix_tile(M);
    const bool one = p->n_groups == 1;
    float* dst = one ? d_out : p->part.get();
    // Samples per lane: speed only, the bits do not depend on it.  As wide as the alignment, the buffer size and the
    // tile allow (V x tile <= 16: beyond that the unrolled tracks' gains no longer fit the scalar registers), but
    // narrower while the launch would have fewer than 512 workgroups: two for each of the MI355X's 256 compute units
    // (a constant, not a device query: it moves time only, and a plan's launches are the same on every box).
    int V = 1;
    if (layout == GAB_MIX_TRACK_MAJOR) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_in);
        const int vmax = MT <= 4 ? 4 : (MT == 8 ? 2 : 1);
        for (int v = vmax; v > 1; v /= 2) {
            const long long wgs = (long long)((B + 64 * v - 1) / (64 * v)) * p->n_groups * n;
            if (B % v == 0 && a % (4 * v) == 0 && wgs >= 512) { V = v; break; }
        }
    }
    const int n_cols = (B + 64 * V - 1) / (64 * V);
    const dim3 grid((unsigned)(n_cols * p->n_groups), 1, (unsigned)n);
    const int threads = p->group_leaves * 64;
#define GAB_MIX(VV, MM, SS)                                                                                      \
    mix_kernel<VV, MM, SS><<<grid, threads, 0, s>>>(d_in, dst, p->gains.current.get(), p->gains.target.get(),    \
                                                    p->gains.ramp.get(), T, B, M, n_cols, p->n_groups,           \
                                                    ramp_first ? 1 : 0)
    if (layout == GAB_MIX_SAMPLE_MAJOR) {
        switch (MT) {
            case 1: GAB_MIX(1, 1, true); break;
            case 2: GAB_MIX(1, 2, true); break;
            case 4: GAB_MIX(1, 4, true); break;
            case 8: GAB_MIX(1, 8, true); break;
            case 16: GAB_MIX(1, 16, true); break;
            case 32: GAB_MIX(1, 32, true); break;
            default: GAB_MIX(1, 64, true); break;
        }
    } else {
        switch (MT * 8 + V) {
            case 1 * 8 + 1: GAB_MIX(1, 1, false); break;
            case 1 * 8 + 2: GAB_MIX(2, 1, false); break;
            case 1 * 8 + 4: GAB_MIX(4, 1, false); break;
            case 2 * 8 + 1: GAB_MIX(1, 2, false); break;
            case 2 * 8 + 2: GAB_MIX(2, 2, false); break;
            case 2 * 8 + 4: GAB_MIX(4, 2, false); break;
            case 4 * 8 + 1: GAB_MIX(1, 4, false); break;
            case 4 * 8 + 2: GAB_MIX(2, 4, false); break;
            case 4 * 8 + 4: GAB_MIX(4, 4, false); break;
            case 8 * 8 + 1: GAB_MIX(1, 8, false); break;
            case 8 * 8 + 2: GAB_MIX(2, 8, false); break;
            case 16 * 8 + 1: GAB_MIX(1, 16, false); break;
            case 32 * 8 + 1: GAB_MIX(1, 32, false); break;
            default: GAB_MIX(1, 64, false); break;
        }
    }
#undef GAB_MIX
    if (int rc = launch_status("mix_kernel")) return rc;
    if (!one) {
        const size_t MB = (size_t)M * B, total = MB * n;
        if ((total + 63) / 64 > (size_t)INT_MAX) return bad_arg("gab_mix_process_batch: the batch is too large for one launch");
        mix_groups_kernel<<<dim3((unsigned)((total + 63) / 64)), 1024, 0, s>>>(p->part.get(), d_out, MB, p->n_groups, total);
        if (int rc = launch_status("mix_groups_kernel")) return rc;
    }
    return GAB_OK;
}

int mix_process(gab_mix_plan* p, const float* d_in, float* d_out, int n_buffers, int layout, hipStream_t s,
                const char* who) {
    if (layout != GAB_MIX_TRACK_MAJOR && layout != GAB_MIX_SAMPLE_MAJOR)
        return refuse(who, "layout must be GAB_MIX_TRACK_MAJOR or GAB_MIX_SAMPLE_MAJOR");
    const size_t in_stride = (size_t)p->tracks * p->bufsize, out_stride = (size_t)p->buses * p->bufsize;
    const bool ramp = p->gains.pending;
    for (int done = 0; done < n_buffers;) {
        const int n = n_buffers - done < p->part_buffers ? n_buffers - done : p->part_buffers;
        if (int rc = mix_launch(p, d_in + done * in_stride, d_out + done * out_stride, n, layout, ramp && done == 0, s))
            return rc;
        done += n;
    }
    if (ramp) p->gains.snap(s);     // the ramp has run through its buffer: current := target, exactly
    return GAB_OK;
}

// check, then commit (gab_plan.hpp): a refused set leaves both matrices and a pending ramp as they were.
int mix_set_range(gab_mix_plan* p, const float* d_gains, int first_track, int n_tracks, const char* who, int ramp,
                  hipStream_t s) {
    const size_t M = (size_t)p->buses, n = (size_t)n_tracks * M;
    return check_then(p->flag, s, who, d_gains, n, MixRule{(unsigned)M}, first_track,
                      [&] { p->gains.commit(d_gains, (size_t)first_track * M, n, ramp != 0, s); });
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_mix_create(gab_mix_plan** out, int tracks, int bufsize, int buses) {
    const long long n_groups = ((long long)tracks + gab::kMixGroupTracks - 1) / gab::kMixGroupTracks;
    return gab::create_entry("gab_mix_create", out, tracks, bufsize, [&] {
        if (buses < 1 || buses > gab::kMixMaxBuses) return gab::bad_arg("gab_mix_create: buses must be 1..64");
        if (n_groups * (((long long)bufsize + 63) / 64) > INT_MAX)
            return gab::bad_arg("gab_mix_create: tracks x bufsize is too large for one launch");
        return GAB_OK;
    }, [&](gab_mix_plan& p) {
        p.buses = buses;
        gab::mix_pick_form(bufsize, buses, &p.leaf_tracks, &p.group_leaves);
        p.n_groups = (int)n_groups;
        p.gains.create((size_t)tracks * buses, bufsize);
        p.flag.alloc(1);
        // The workspace of the final pass: as many buffers' partial sums as fit 32 MiB, at least one and at most
        // kMixBatchChunk.  A longer batch is that many buffers per launch, one launch after the other.
        const size_t per_buffer = (size_t)p.n_groups * buses * bufsize * sizeof(float);
        size_t chunk = ((size_t)32 << 20) / per_buffer;
        chunk = chunk < 1 ? 1 : (chunk > (size_t)gab::kMixBatchChunk ? (size_t)gab::kMixBatchChunk : chunk);
        p.part_buffers = p.n_groups > 1 ? (int)chunk : gab::kMixBatchChunk;
        if (p.n_groups > 1) p.part.alloc(chunk * per_buffer / sizeof(float));
        p.gains.fill(std::vector<float>((size_t)buses, 0.0f), tracks);      // silence
        return GAB_OK;
    });
}

int gab_mix_destroy(gab_mix_plan* plan) { return gab::destroy_plan(plan, "gab_mix_destroy: null pointer"); }

int gab_mix_set_gains(gab_mix_plan* plan, const float* d_gains, int ramp, gab_stream_t stream) {
    return gab::set_entry("gab_mix_set_gains", gab::mix_set_range, plan, d_gains, true, 0, 0, ramp, gab::as_stream(stream));
}

int gab_mix_set_gains_tracks(gab_mix_plan* plan, const float* d_gains, int first_track, int n_tracks, int ramp,
                             gab_stream_t stream) {
    return gab::set_entry("gab_mix_set_gains_tracks", gab::mix_set_range, plan, d_gains, false, first_track, n_tracks, ramp,
                          gab::as_stream(stream));
}

int gab_mix_reset(gab_mix_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_mix_reset", {plan}, [&] {
        plan->gains.snap(gab::as_stream(stream));
        return GAB_OK;
    });
}

int gab_mix_process(gab_mix_plan* plan, const float* d_in, float* d_out, int layout, gab_stream_t stream) {
    return gab::entry("gab_mix_process", {plan, d_in, d_out}, [&] {
        return gab::mix_process(plan, d_in, d_out, 1, layout, gab::as_stream(stream), "gab_mix_process");
    });
}

int gab_mix_process_batch(gab_mix_plan* plan, const float* d_in, float* d_out, int n_buffers, int layout,
                          gab_stream_t stream) {
    return gab::batch_entry("gab_mix_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::mix_process(plan, d_in, d_out, n_buffers, layout, gab::as_stream(stream), "gab_mix_process_batch");
    });
}

int gab_mix_gains(gab_mix_plan* plan, float** d_current, float** d_target, size_t* n_floats) {
    return gab::expose_entry("gab_mix_gains", plan, &gab_mix_plan::gains, d_current, d_target, n_floats);
}

int gab_mix_form(const gab_mix_plan* plan, int* leaf_tracks, int* group_leaves) {
    return gab::entry("gab_mix_form", {plan, leaf_tracks, group_leaves}, [&] {
        *leaf_tracks = plan->leaf_tracks;
        *group_leaves = plan->group_leaves;
        return GAB_OK;
    });
}

}  // extern "C"
