// k_mconv.hip — the matrix-convolution plan: I inputs summed into O outputs through a partitioned FIR filter per
// (output, input): K partitions of 512 taps, 1024-point overlap-save transforms (include/gab_c_api.h, gab_mconv_*).
// What O fdaf plans with mu = 0 behind O mix plans compose, with O / 2 inverse transforms a block where those take
// O I / 2, and every input spectrum formed once.  No counterpart in the reference.
//
// A call is rounds of at most `round` blocks (16, fewer where the partials of 16 would pass kMconvPartBytes); a round is
// three launches on the stream, and a fourth on the blocks of a ramp buffer:
//   mconv_forward_kernel   a wave per (input pair, block), four a workgroup, no workgroup barrier: the window
//                          [block before | block] of the pair through stft::spectra into the ring slot of the block.
//                          The wave of the call's first block also moves prev: read first, written last.
//   mconv_product_kernel   a wave per (output pair, group of 32 inputs, run of 64 bins, block): a lane owns one bin and
//                          runs the header's chain for both outputs of the pair, i ascending and inside it p ascending
//                          from +0, each X word read once for the two.  Eight (i, p) steps' loads are issued before
//                          their multiply-adds (DESIGN.md §7b found that for the fdl product).  The group partial goes
//                          to the plan's scratch [block][O][G][513]; no atomics.  On a ramp block it runs twice, against
//                          `target` and against `current`.
//   mconv_inverse_kernel   a workgroup of nine waves per (output pair, block): a thread per bin adds the pair's partials in
//                          ascending g (a chain by contract: 128 long at 4096 inputs, which one wave walked in 80 us),
//                          the pair's Y goes through LDS to the first wave: stft::pack_rows, the inverse, the fmaf by
//                          2^-10; on a ramp block the same for `current` and the blend.  One thread of the launch moves
//                          count, which the two launches before it read.
//   mconv_taps_kernel      set_taps: a wave per (output, input, partition), stft::tap_spectrum, as the fdaf plan's.
//   MconvTapRule           refuses a tap that is not finite, naming the first.
//
// Output bits depend on the samples, the taps and the state alone: not on bufsize, the cut into calls, batches or
// rounds, the alignment, or which plan holds an output pair.  Registers, LDS, occupancy and cost: DESIGN.md §4s.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>

#include "gab_fft.hpp"
#include "gab_plan.hpp"
#include "gab_stft.hpp"

namespace gab {
namespace {

using fft::cf;

constexpr int kMconvBlock = stft::kN / 2;                 // 512: the block, and the taps of a partition
constexpr int kMconvMaxI = 4096, kMconvMaxO = 64, kMconvMaxK = 32, kMconvMaxCells = 65536;
constexpr int kMconvGroup = 32;                           // inputs of a group partial: a cut that depends on I alone
constexpr int kMconvRound = 16;                           // blocks of a round at most; the ring holds K + 15 slots
constexpr int kMconvRuns = (stft::kBins + 63) / 64;       // 9 runs of 64 bins; the last is bin 512 alone
constexpr int kMconvAhead = 8;                            // (i, p) steps whose loads go out before their multiply-adds
constexpr int kMconvSumThreads = 576;                     // the last launch's workgroup: nine waves, a thread a bin in the sums
constexpr int kMconvSumAhead = 16;                        // group partials whose loads go out before their additions
constexpr size_t kMconvPartBytes = (size_t)64 << 20;      // the partials of a round and table stay below this

// Grid: x = group of four input pairs, y = block of the round.  in: [n][I][B], B a multiple of 512.  X: [S][I][513].
// prev: [I][512].  first_block: the round's first block, counted from the call's first; call_blocks: the call's.
__global__ __launch_bounds__(256) void mconv_forward_kernel(const float* __restrict__ in, cf* __restrict__ X, float* prev,
                                                            const unsigned* __restrict__ count,
                                                            const cf* __restrict__ tw, int I, int B, int S, int first_block,
                                                            int call_blocks) {
    __shared__ cf lds[4 * stft::kImg];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    cf* const img = lds + w * stft::kImg;
    const int ia = ((int)blockIdx.x * 4 + w) * 2;
    if (ia >= I) return;                                   // whole wave; no workgroup barrier anywhere below
    const bool hasb = ia + 1 < I;                          // an odd last input: beside zero samples
    const int g = first_block + (int)blockIdx.y, per = B / kMconvBlock;
    const auto row = [&](int gg) {                         // input ia's block gg of the call, this lane's first sample
        const int nb = gg / per;
        return ((size_t)nb * I + ia) * B + (size_t)(gg - nb * per) * kMconvBlock + lane;
    };
    using FWD = fft::WaveFFT1024<false>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);
    const float* const cur = in + row(g);
    const float* const bef = g == 0 ? prev + (size_t)ia * kMconvBlock + lane : in + row(g - 1);
    const size_t bef_b = g == 0 ? (size_t)kMconvBlock : (size_t)B;
    cf z[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        z[j] = fft::mk(bef[64 * j], hasb ? bef[bef_b + 64 * j] : 0.0f);
        z[j + 8] = fft::mk(cur[64 * j], hasb ? cur[(size_t)B + 64 * j] : 0.0f);
    }
    cf xa[9], xb[9];
    stft::spectra(z, img, t, lane, xa, xb);
    const unsigned slot = (count[0] + blockIdx.y) % (unsigned)S;
    cf* const Xa = X + ((size_t)slot * I + ia) * stft::kBins;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        if (k <= stft::kN / 2) {
            Xa[k] = xa[r];
            if (hasb) Xa[stft::kBins + k] = xb[r];
        }
    }
    // prev := the call's last block, by the one wave that read prev (its values went through the transform above)
    if (g == 0) {
        const float* const last = in + row(call_blocks - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            prev[(size_t)ia * kMconvBlock + lane + 64 * j] = last[64 * j];
            if (hasb) prev[(size_t)(ia + 1) * kMconvBlock + lane + 64 * j] = last[(size_t)B + 64 * j];
        }
    }
}

// Grid: x = group of four (input group, run of bins), y = output pair, z = block of the round.  H: [O][I][K][513].
// part: [round][O][G][513].
__global__ __launch_bounds__(256) void mconv_product_kernel(const cf* __restrict__ X, const cf* __restrict__ H,
                                                            cf* __restrict__ part, const unsigned* __restrict__ count,
                                                            int I, int O, int K, int S, int G) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int flat = (int)blockIdx.x * 4 + w;
    if (flat >= G * kMconvRuns) return;
    const int g = flat / kMconvRuns, k = (flat - g * kMconvRuns) * 64 + lane;
    const int oa = 2 * (int)blockIdx.y;
    const bool hasb = oa + 1 < O;
    const int i0 = g * kMconvGroup, total = (I - i0 < kMconvGroup ? I - i0 : kMconvGroup) * K;
    const int newest = (int)((count[0] + blockIdx.z) % (unsigned)S);
    if (k > stft::kN / 2) return;                          // no lane hands anything to another below
    const size_t plane = (size_t)I * K * stft::kBins;
    const cf* const Ha = H + ((size_t)oa * I + i0) * K * stft::kBins + k;
    const cf* const Xk = X + (size_t)i0 * stft::kBins + k;
    cf acca = fft::mk(0.0f, 0.0f), accb = fft::mk(0.0f, 0.0f);
    int i = 0, p = 0;                                      // step n = i K + p of the chain
    for (int n0 = 0; n0 < total; n0 += kMconvAhead) {
        cf x[kMconvAhead], ha[kMconvAhead], hb[kMconvAhead];
#pragma unroll
        for (int j = 0; j < kMconvAhead; ++j) {
            x[j] = ha[j] = hb[j] = fft::mk(0.0f, 0.0f);
            if (n0 + j < total) {
                const int sp = newest - p < 0 ? newest - p + S : newest - p;
                x[j] = Xk[((size_t)sp * I + i) * stft::kBins];
                ha[j] = Ha[(size_t)(n0 + j) * stft::kBins];
                if (hasb) hb[j] = Ha[plane + (size_t)(n0 + j) * stft::kBins];
                if (++p == K) {
                    p = 0;
                    ++i;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kMconvAhead; ++j) {
            if (n0 + j < total) {
                acca = fft::cfma(x[j], ha[j], acca);
                if (hasb) accb = fft::cfma(x[j], hb[j], accb);
            }
        }
    }
    cf* const Pa = part + (((size_t)blockIdx.z * O + oa) * G + g) * stft::kBins + k;
    Pa[0] = acca;
    if (hasb) Pa[(size_t)G * stft::kBins] = accb;
}

// Y of a pair's two outputs at bin k: ((P_0 + P_1) + P_2) ..., g ascending, re and im by one rounded addition each.
// P: output a's [G][513], output b's behind it.  The additions are a chain by contract; the loads of kMconvSumAhead
// groups go out before their additions.
__device__ __forceinline__ void mconv_sum(const cf* __restrict__ P, int G, bool hasb, int k, cf& ya, cf& yb) {
    const cf* const Pa = P + k;
    const cf* const Pb = Pa + (size_t)G * stft::kBins;
    ya = Pa[0];
    yb = hasb ? Pb[0] : fft::mk(0.0f, 0.0f);
    for (int g0 = 1; g0 < G; g0 += kMconvSumAhead) {
        cf a[kMconvSumAhead], b[kMconvSumAhead];
#pragma unroll
        for (int j = 0; j < kMconvSumAhead; ++j) {
            a[j] = b[j] = fft::mk(0.0f, 0.0f);
            if (g0 + j < G) {
                a[j] = Pa[(size_t)(g0 + j) * stft::kBins];
                if (hasb) b[j] = Pb[(size_t)(g0 + j) * stft::kBins];
            }
        }
#pragma unroll
        for (int j = 0; j < kMconvSumAhead; ++j) {
            if (g0 + j < G) {
                ya = fft::cadd(ya, a[j]);
                if (hasb) yb = fft::cadd(yb, b[j]);
            }
        }
    }
}

// The 512 samples of a pair's block out of its two spectra (Y: output a's bins at [k], output b's at [kImgB + k]): the
// packing, the inverse, fmaf(z, 2^-10, +0) (a -0 out of a transform of zeros becomes +0).  The image must be free, and
// is left to be fenced off by the caller.
template <class TW>
__device__ __forceinline__ void mconv_block(const cf* Y, cf* img, const TW& t, int lane, float (&ya)[8], float (&yb)[8]) {
    cf sa[9], sb[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = lane + 64 * r;
        sa[r] = sb[r] = fft::mk(0.0f, 0.0f);
        if (k <= stft::kN / 2) {
            sa[r] = Y[k];
            sb[r] = Y[stft::kImgB + k];
        }
    }
    cf z[16];
    stft::pack_rows(sa, sb, img, lane, z);
    fft::WaveFFT1024<true>::run(z, img, t, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ya[j] = fmaf(z[j + 8].x, 0x1p-10f, 0.0f);
        yb[j] = fmaf(z[j + 8].y, 0x1p-10f, 0.0f);
    }
}

// Grid: x = output pair, y = block of the round; nine waves.  partT, partC: [round][O][G][513], the partials against
// target and (the round's first ramp_blocks blocks only) against current.  ramp: [B].  out: [n][O][B].
__global__ __launch_bounds__(kMconvSumThreads) void mconv_inverse_kernel(const cf* __restrict__ partT,
                                                                         const cf* __restrict__ partC,
                                                                         const float* __restrict__ ramp,
                                                                         float* __restrict__ out, unsigned* count,
                                                                         const cf* __restrict__ tw, int O, int B, int G,
                                                                         int first_block, int n_blocks, int ramp_blocks) {
    __shared__ cf sums[2][2 * stft::kImgB];                // per table the pair's Y: a's bins, b's from kImgB
    __shared__ cf img[stft::kImg];
    const int tid = (int)threadIdx.x;
    // the launches that read count are behind this one's stream predecessors and in front of its successors
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) count[0] += (unsigned)n_blocks;
    const int oa = 2 * (int)blockIdx.x;
    const bool hasb = oa + 1 < O;                          // an odd last output: beside a zero spectrum
    const int blk = (int)blockIdx.y, g = first_block + blk, per = B / kMconvBlock;
    const bool ramped = blk < ramp_blocks;                 // the ramp buffer is the call's first: g < per
    const size_t po = ((size_t)blk * O + oa) * G * stft::kBins;
    // ---- the sums: a thread a bin, for both outputs (a group of 128 partials is a walk too long for one wave) ----
    if (tid <= stft::kN / 2) {
        mconv_sum(partT + po, G, hasb, tid, sums[0][tid], sums[0][stft::kImgB + tid]);
        if (ramped) mconv_sum(partC + po, G, hasb, tid, sums[1][tid], sums[1][stft::kImgB + tid]);
    }
    __syncthreads();
    if (tid >= 64) return;                                 // the first wave alone goes on: no barrier below
    // ---- the inverse, the blend and the store ----
    const int lane = tid;
    using FWD = fft::WaveFFT1024<false>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);
    float ya[8], yb[8];
    mconv_block(sums[0], img, t, lane, ya, yb);
    if (ramped) {
        float ca[8], cb[8];
        stft::wave_sync();                                 // the image is free again
        mconv_block(sums[1], img, t, lane, ca, cb);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = ramp[(size_t)g * kMconvBlock + lane + 64 * j];
            ya[j] = fmaf(__fsub_rn(ya[j], ca[j]), r, ca[j]);
            yb[j] = fmaf(__fsub_rn(yb[j], cb[j]), r, cb[j]);
        }
    }
    const int nb = g / per;
    float* const oa_row = out + ((size_t)nb * O + oa) * B + (size_t)(g - nb * per) * kMconvBlock + lane;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        oa_row[64 * j] = ya[j];
        if (hasb) oa_row[(size_t)B + 64 * j] = yb[j];
    }
}

// Grid: x = group of four (output, input, partition) of the range, a wave each.  taps: [n_out][n_in][512 K].
// H: the plan's [O][I][K][513].
__global__ __launch_bounds__(256) void mconv_taps_kernel(const float* __restrict__ taps, cf* __restrict__ H,
                                                         const cf* __restrict__ tw, int I, int K, int first_out, int n_out,
                                                         int first_in, int n_in) {
    __shared__ cf lds[4 * stft::kImg];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long idx = (long long)blockIdx.x * 4 + w;
    if (idx >= (long long)n_out * n_in * K) return;        // whole wave; no workgroup barrier below
    const int cell = (int)(idx / K), p = (int)(idx - (long long)cell * K);
    const int oo = cell / n_in, ii = cell - oo * n_in;
    using FWD = fft::WaveFFT1024<false>;
    FWD::Lean t;
    FWD::load_twiddles(t, tw, lane);
    stft::tap_spectrum(taps + (size_t)idx * kMconvBlock,
                       H + (((size_t)(first_out + oo) * I + first_in + ii) * K + p) * stft::kBins, lds + w * stft::kImg, t,
                       lane);
}

// src: [n_out][n_in][L]
struct MconvTapRule {
    unsigned L, n_in;
    int first_out;
    __device__ bool refuses(const float* src, size_t i) const { return not_finite(__float_as_uint(src[i])); }
    std::string refusal(unsigned i, int first_in) const {
        const unsigned cell = i / L;
        return "output " + std::to_string(first_out + (int)(cell / n_in)) + " input " +
               std::to_string(first_in + (int)(cell % n_in)) + " tap " + std::to_string((int)(i % L)) +
               " must be finite; the plan keeps its taps";
    }
};

}  // namespace
}  // namespace gab

struct gab_mconv_plan {
    int tracks = 0, bufsize = 0;       // tracks: the inputs (what create_entry and set_entry call them)
    int outputs = 0, partitions = 0, slots = 0, groups = 0, round = 0;
    const gab::fft::cf* tw = nullptr;  // the device's twiddle table (the library's, not the plan's)
    gab::RampedTable H;                // [O][I][K][513][2] each: the taps' half-spectra
    gab::DeviceBuf<float> X;           // [S][I][513][2]: the ring of input spectra, block b in slot b mod S
    gab::DeviceBuf<float> prev;        // [I][512]: the input block before
    gab::DeviceBuf<unsigned> count;    // [1]: blocks since the reset
    gab::DeviceBuf<float> part;        // [2][round][O][G][513][2]: the group partials against target, against current
    gab::DeviceBuf<unsigned> flag;
};

namespace gab {
namespace {

// Do a[0, na) and b[0, nb) share a byte?
bool mconv_overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb * sizeof(float) && pb < pa + na * sizeof(float);
}

// n buffers as rounds of launches on s.  Nothing is allocated and nothing waits here.
int mconv_process(gab_mconv_plan* p, const float* d_in, float* d_out, int n_buffers, hipStream_t s, const char* who) {
    if (int rc = stft::check_length(who, *p, n_buffers)) return rc;
    const size_t frames = (size_t)n_buffers * p->bufsize;
    if (mconv_overlap(d_in, frames * p->tracks, d_out, frames * p->outputs)) return refuse(who, "d_out may not overlap d_in");
    const int I = p->tracks, O = p->outputs, K = p->partitions, S = p->slots, G = p->groups, B = p->bufsize;
    const int per = B / kMconvBlock, blocks = n_buffers * per;
    const bool ramp = p->H.pending;
    cf* const X = reinterpret_cast<cf*>(p->X.get());
    cf* const partT = reinterpret_cast<cf*>(p->part.get());
    cf* const partC = partT + p->part.size() / 4;
    const unsigned in_quads = (unsigned)(((I + 1) / 2 + 3) / 4), out_pairs = (unsigned)((O + 1) / 2);
    const dim3 product((unsigned)((G * kMconvRuns + 3) / 4), out_pairs, 1);
    for (int done = 0; done < blocks; done += p->round) {
        const int nblk = std::min(p->round, blocks - done);
        const int nramp = ramp ? std::max(0, std::min(nblk, per - done)) : 0;     // the ramp buffer is the first
        mconv_forward_kernel<<<dim3(in_quads, (unsigned)nblk), 256, 0, s>>>(d_in, X, p->prev.get(), p->count.get(), p->tw,
                                                                            I, B, S, done, blocks);
        if (int rc = launch_status("mconv_forward_kernel")) return rc;
        mconv_product_kernel<<<dim3(product.x, product.y, (unsigned)nblk), 256, 0, s>>>(
            X, reinterpret_cast<const cf*>(p->H.target.get()), partT, p->count.get(), I, O, K, S, G);
        if (int rc = launch_status("mconv_product_kernel")) return rc;
        if (nramp) {
            mconv_product_kernel<<<dim3(product.x, product.y, (unsigned)nramp), 256, 0, s>>>(
                X, reinterpret_cast<const cf*>(p->H.current.get()), partC, p->count.get(), I, O, K, S, G);
            if (int rc = launch_status("mconv_product_kernel")) return rc;
        }
        mconv_inverse_kernel<<<dim3(out_pairs, (unsigned)nblk), kMconvSumThreads, 0, s>>>(
            partT, partC, p->H.ramp.get(), d_out, p->count.get(), p->tw, O, B, G, done, nblk, nramp);
        if (int rc = launch_status("mconv_inverse_kernel")) return rc;
    }
    if (ramp) p->H.snap(s);            // the ramp has run through its buffer: current := target, exactly
    return GAB_OK;
}

// The taps of outputs [first_out, first_out + n_out) x inputs [first_in, first_in + n_in), in time: finite or refused
// (check, then commit: gab_plan.hpp); then their partitions' spectra into target, and into current unless they are
// ramped in.  The ring, prev and count stay.
int mconv_set_taps(gab_mconv_plan* p, const float* d_taps, int first_out, int n_out, int first_in, int n_in, int ramped,
                   const char* who, hipStream_t s) {
    if (!track_range_ok(p->outputs, first_out, n_out)) return refuse(who, "the output range is outside the plan");
    const size_t L = (size_t)p->partitions * kMconvBlock, n = (size_t)n_out * n_in * L;
    int rc_launch = GAB_OK;
    const int rc = check_then(p->flag, s, who, d_taps, n, MconvTapRule{(unsigned)L, (unsigned)n_in, first_out}, first_in, [&] {
        const long long waves = (long long)n_out * n_in * p->partitions;
        float* const tables[2] = {p->H.target.get(), ramped ? nullptr : p->H.current.get()};
        for (float* H : tables) {
            if (!H || rc_launch) continue;
            mconv_taps_kernel<<<dim3((unsigned)((waves + 3) / 4)), 256, 0, s>>>(d_taps, reinterpret_cast<cf*>(H), p->tw,
                                                                               p->tracks, p->partitions, first_out, n_out,
                                                                               first_in, n_in);
            rc_launch = launch_status("mconv_taps_kernel");
        }
        if (ramped && !rc_launch) p->H.pending = true;
        GAB_HIP_CHECK(hipStreamSynchronize(s));
    });
    return rc ? rc : rc_launch;
}

}  // namespace
}  // namespace gab

extern "C" {

int gab_mconv_create(gab_mconv_plan** out, int inputs, int bufsize, int outputs, int partitions) {
    return gab::create_entry("gab_mconv_create", out, inputs, bufsize, [&] {
        const char* const who = "gab_mconv_create";
        if (inputs > gab::kMconvMaxI) return gab::refuse(who, "inputs must be 1..4096");
        if (outputs < 1 || outputs > gab::kMconvMaxO) return gab::refuse(who, "outputs must be 1..64");
        if (partitions < 1 || partitions > gab::kMconvMaxK) return gab::refuse(who, "partitions must be 1..32");
        if ((long long)inputs * outputs * partitions > gab::kMconvMaxCells)
            return gab::refuse(who, "inputs * outputs * partitions must be at most 65536");
        if (bufsize % gab::kMconvBlock != 0) return gab::refuse(who, "bufsize must be a multiple of 512");
        return GAB_OK;
    }, [&](gab_mconv_plan& p) {
        p.outputs = outputs;
        p.partitions = partitions;
        p.slots = partitions + gab::kMconvRound - 1;
        p.groups = (inputs + gab::kMconvGroup - 1) / gab::kMconvGroup;
        const size_t block_part = (size_t)outputs * p.groups * gab::stft::kBins * 2;       // floats
        p.round = (int)std::min<size_t>(gab::kMconvRound, std::max<size_t>(1, gab::kMconvPartBytes / (block_part * sizeof(float))));
        p.tw = gab::fft::device_twiddles();
        p.H.create((size_t)outputs * inputs * partitions * gab::stft::kBins * 2, bufsize);
        p.X.alloc((size_t)p.slots * inputs * gab::stft::kBins * 2);
        p.prev.alloc((size_t)inputs * gab::kMconvBlock);
        p.count.alloc(1);
        p.part.alloc(2 * (size_t)p.round * block_part);
        p.flag.alloc(1);
        // zero taps, an empty ring: the output is all +0
        GAB_HIP_CHECK(hipMemset(p.H.current.get(), 0, p.H.current.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.H.target.get(), 0, p.H.target.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.X.get(), 0, p.X.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.prev.get(), 0, p.prev.size() * sizeof(float)));
        GAB_HIP_CHECK(hipMemset(p.count.get(), 0, sizeof(unsigned)));
        GAB_HIP_CHECK(hipStreamSynchronize(nullptr));
        return GAB_OK;
    });
}

int gab_mconv_destroy(gab_mconv_plan* plan) { return gab::destroy_plan(plan, "gab_mconv_destroy: null pointer"); }

int gab_mconv_set_taps(gab_mconv_plan* plan, const float* d_taps, int ramped, gab_stream_t stream) {
    const auto set = [&](gab_mconv_plan* p, const float* d, int first_in, int n_in, const char* who) {
        return gab::mconv_set_taps(p, d, 0, p->outputs, first_in, n_in, ramped, who, gab::as_stream(stream));
    };
    return gab::set_entry("gab_mconv_set_taps", set, plan, d_taps, true, 0, 0);
}

int gab_mconv_set_taps_range(gab_mconv_plan* plan, const float* d_taps, int first_output, int n_outputs, int first_input,
                             int n_inputs, int ramped, gab_stream_t stream) {
    const auto set = [&](gab_mconv_plan* p, const float* d, int first_in, int n_in, const char* who) {
        return gab::mconv_set_taps(p, d, first_output, n_outputs, first_in, n_in, ramped, who, gab::as_stream(stream));
    };
    return gab::set_entry("gab_mconv_set_taps_range", set, plan, d_taps, false, first_input, n_inputs);
}

int gab_mconv_reset(gab_mconv_plan* plan, gab_stream_t stream) {
    return gab::entry("gab_mconv_reset", {plan}, [&]() -> int {
        hipStream_t s = gab::as_stream(stream);
        GAB_HIP_CHECK(hipMemsetAsync(plan->X.get(), 0, plan->X.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->prev.get(), 0, plan->prev.size() * sizeof(float), s));
        GAB_HIP_CHECK(hipMemsetAsync(plan->count.get(), 0, sizeof(unsigned), s));
        plan->H.snap(s);               // the taps stay; a pending ramp is dropped
        return GAB_OK;
    });
}

int gab_mconv_process(gab_mconv_plan* plan, const float* d_in, float* d_out, gab_stream_t stream) {
    return gab::entry("gab_mconv_process", {plan, d_in, d_out}, [&] {
        return gab::mconv_process(plan, d_in, d_out, 1, gab::as_stream(stream), "gab_mconv_process");
    });
}

int gab_mconv_process_batch(gab_mconv_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream) {
    return gab::batch_entry("gab_mconv_process_batch", {plan, d_in, d_out}, n_buffers, [&] {
        return gab::mconv_process(plan, d_in, d_out, n_buffers, gab::as_stream(stream), "gab_mconv_process_batch");
    });
}

int gab_mconv_state(gab_mconv_plan* plan, float** d_H_current, float** d_H_target, float** d_X, float** d_prev,
                    unsigned** d_count, int* slots) {
    return gab::entry("gab_mconv_state", {plan, d_H_current, d_H_target, d_X, d_prev, d_count, slots}, [&] {
        *d_H_current = plan->H.current.get();
        *d_H_target = plan->H.target.get();
        *d_X = plan->X.get();
        *d_prev = plan->prev.get();
        *d_count = plan->count.get();
        *slots = plan->slots;
        return GAB_OK;
    });
}

}  // extern "C"
