/*
 * gab_c_api.h — C ABI of libgab_hip.so, the MI355X (gfx950) implementation of
 * the gpuaudiobench hot path.
 *
 * The reference (tskare/gpuaudiobench, cuda/) has no FFI of its own: its
 * boundary is the C++ class GPUABenchmark (cuda/bench_base.cuh:18-139) plus one
 * __global__ kernel (or cuFFT pipeline) per benchmark.  This header is what a
 * binding for that path would import:
 *   - section K: one entry point per reference kernel / vendor-library call
 *     site, taking DEVICE pointers, sizes and a HIP stream;
 *   - section P: plan objects for the two stateful pipelines (FFT convolution,
 *     FDTD3D);
 *   - section H: the harness itself (create/setup/run/validate by registry
 *     name), mirroring main.cu's runSelectedBenchmark (cuda/main.cu:117-164).
 * C++ users include include/gab/ *.hpp instead and get the reference's class
 * surface directly.
 *
 * Conventions: plain pointers and sizes only; every function returns GAB_OK (0),
 * a positive hipError_t value, or a negative GAB_ERR_*; no exception crosses
 * this boundary (gab_last_error() holds the text, thread-local).  All kernels
 * are asynchronous on `stream` (a hipStream_t cast to void*; NULL = default
 * stream) unless stated otherwise.  Layouts follow the reference:
 * "track-major" = [t*B + s], "sample-major" = [T*s + t].
 */
#ifndef GAB_C_API_H
#define GAB_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAB_OK 0
#define GAB_ERR_INVALID_ARG (-1)
#define GAB_ERR_RUNTIME     (-2)
#define GAB_ERR_UNSUPPORTED (-3)

typedef void* gab_stream_t;

int         gab_version(void);            /* 10000*major + 100*minor + patch   */
const char* gab_last_error(void);
int         gab_device_count(int* count); /* cuda/main.cu:307-314              */

/* ===================================================================== */
/* K. kernels                                                            */
/* ===================================================================== */

/* NoOpKernel (cuda/bench_noop.cu:9-16): out[i] = in[i], i < n.  (The
 * reference launch covers only ceil(T/256)*256 elements; this copies all n.) */
int gab_noop(const float* d_in, float* d_out, size_t n, gab_stream_t stream);

/* GainKernel (cuda/bench_gain.cu:6-24): out[i] = gain * in[i].  Bit-exact.   */
int gab_gain(const float* d_in, float* d_out, size_t n, float gain,
             gab_stream_t stream);

/* GainStatsKernel (cuda/bench_gainstats.cu:7-31): out = gain*in (track-major
 * T x B); stats[2t] = mean of the INPUT track, stats[2t+1] = max (from -1e9). */
int gab_gainstats(const float* d_in, float* d_out, float* d_stats, int tracks,
                  int bufsize, float gain, gab_stream_t stream);

/* DataTransferKernel (cuda/bench_datatransfer.cu:15-25):
 * out[i] = i < in_size ? in[i] : 0.5f + 0.5f*sinf(0.001f*i), i < out_size.    */
int gab_datatransfer(const float* d_in, float* d_out, int in_size, int out_size,
                     gab_stream_t stream);

/* The same operation with both link directions busy at once (replaces the reference's H2D -> kernel -> D2H
 * sequence around DataTransferKernel, cuda/bench_datatransfer.cu:62-75, in one call).  h_in [in_size] is any
 * host memory hipMemcpyAsync accepts (pinned for the overlap; pageable memory is uploaded completely before the
 * launch); h_out [out_size] MUST be pinned (hipHostMalloc) or
 * device memory: the kernel writes it itself while ONE engine copy of h_in lands in the plan's staging buffer.
 * Returns when h_out is complete AND the whole input has been uploaded; bit-identical to gab_datatransfer on the
 * uploaded input.  in_size <= the plan's max_in_size.  The call blocks (it is the benchmark's timed unit); `stream`
 * carries the kernel.  One call at a time per plan.  GAB_ERR_RUNTIME: a wait inside the launch ran out (about a
 * second) — h_out is then invalid and the plan has been re-armed for the next call.                              */
typedef struct gab_link_plan gab_link_plan;
int gab_link_plan_create(int max_in_size, gab_link_plan** out);
void gab_link_plan_destroy(gab_link_plan* plan);
int gab_datatransfer_round_trip(gab_link_plan* plan, const float* h_in, float* h_out, int in_size, int out_size,
                                gab_stream_t stream);
/* The kernel takes input words while the upload is still running: that rests on engine writes landing whole and once (an
 * observation).  Since round 6 a second, small launch behind every call — ordered behind the upload's completion event —
 * compares what the kernel took with what the COMPLETED upload left and puts the staging buffer back; it costs the call
 * nothing (the call returns on the main launch's end).  Its verdict is read by the plan's NEXT call (which returns
 * GAB_ERR_RUNTIME: the PREVIOUS call's output was wrong) or by this function (waits a few microseconds for the check).   */
int gab_datatransfer_round_trip_check(gab_link_plan* plan);

/* ---- keep-warm (additive; no counterpart in the reference, whose iterations run back to back) ---------------------
 * A device left idle for a DAW slot (512 / 48000 s = 10.667 ms) answers the next call later than one that has just been
 * busy: at C3 gab_conv_round_trip's p50 is 76-81 us one call per slot against 67-70 us back to back on the same box — and
 * 67-68 us per slot with EIGHT idle waves resident beside (profiles/r05_paced_keep_warm.txt: one wave buys nothing — the
 * workgroups of a launch go round the eight XCDs, eight wake them all; 64 waves and more cost, their looks cross the link
 * the round trip is using).  A gab_keep_warm is that launch: `workgroups` single-wave workgroups that sleep and look at a
 * pinned word every ~64 us (no LDS, no memory traffic but the look), on a highest-priority stream of their own.
 * gab_keep_warm_kick starts the launch if none is there and pushes its end out otherwise: the launch ends by itself
 * `idle_seconds` after the last kick (and at destroy, at once).  Kick once per slot.
 * Opt-in, because it costs what resident waves cost (power, one wave slot on `workgroups` compute units) and because,
 * like the engine below, the launch is THERE: hipDeviceSynchronize, hipFree and hipHostFree — which wait for every launch
 * on the device — return only once it has ended (up to idle_seconds after the last kick), and work queued on another
 * stream that the runtime maps to the same hardware queue stands behind it for as long (streams of the default priority
 * never share a queue with it: profiles/r05_incident_engine_queue_sharing.txt).  Keep idle_seconds short: a few slots.
 * gab_conv_round_trip_keep_warm(plan, 1) makes every gab_conv_round_trip of that plan end with a kick (0: no more kicks,
 * the launch ends idle_seconds later; the plan owns the object: 8 workgroups, idle limit = eight buffer periods at
 * 44.1 kHz, at least 0.05 s).
 * NOT beside a resident engine, and the library enforces it (it makes every keep-warm launch and every engine, so it knows):
 * gab_conv_engine_start needs every compute unit whole (its workgroup fills the register files) — with keep-warm waves on eight of
 * them its first buffer waited out their idle limit (484 ms on record).  gab_conv_engine_start drops the plan's OWN keep-warm and
 * returns GAB_ERR_INVALID_ARG while any other keep-warm launch is running on the device (destroy the object, or let it run out);
 * gab_keep_warm_kick returns GAB_ERR_INVALID_ARG when it would have to START a launch while an engine is resident on the device.
 * The engine keeps the device awake itself.
 * Workgroup 0 of the launch alone decides that it has been idle long enough; the other waves leave when it says so.
 * One thread at a time per object (like a plan).  gab_keep_warm_running: is the launch on the device right now?
 * gab_keep_warm_placement: where the waves of the current (or last) launch landed — for each wave that has started, the raw
 * HW_ID register (gfx9 layout: bits 3:0 wave slot, 5:4 SIMD, 11:8 compute unit, 12 shader array, 15:13 shader engine) and the
 * XCC_ID register (bits 3:0: the XCD); `*started` = how many have (of `workgroups`); at most `capacity` pairs are written.
 * Eight waves are meant to sit on eight XCDs: a paced measurement that prints this beside its p50 classifies itself.          */
typedef struct gab_keep_warm gab_keep_warm;
int gab_keep_warm_create(gab_keep_warm** out, int workgroups, double idle_seconds);
int gab_keep_warm_kick(gab_keep_warm* warm);
int gab_keep_warm_running(gab_keep_warm* warm, int* running);
int gab_keep_warm_placement(gab_keep_warm* warm, unsigned* hw_id, unsigned* xcc_id, int capacity, int* started);
int gab_keep_warm_destroy(gab_keep_warm* warm);

/* IIRFilterKernel (cuda/bench_iir.cu:10-44): DF-II biquad per track,
 * coeffs = {b0,b1,b2,a1,a2} (HOST pointer, 5 floats), d_state = T x {z1,z2}
 * read and written back.
 * gab_iir: one wavefront per track, wave-level scan of the state recurrence
 * (bufsize in {64,128,256,512,1024}, 16-byte aligned buffers).  Re-associates
 * the recurrence, so not bit-identical to the golden.  The scan carries the
 * state as (z1, z1 - z2) for a1 <= 0 and (z1, z1 + z2) for a1 > 0, so that
 * poles next to z = 1 or z = -1 cancel nothing.  Tested, not proven: outputs
 * and carried state are within max(1e-5, 4 e32) of the float64 filter's peak,
 * e32 being what the ordered float32 form itself loses against float64 on the
 * same input, on sixteen sections in every form (tests/test_iir_scan_gpu.py:
 * high-passes, a shelf, Q 30 bells and notches from 20 Hz to 23 kHz at 48 and
 * 96 kHz, the mirror image of a 30 Hz high-pass; with the reference's filter
 * ~1e-7 of the golden).  Not covered: real poles next to BOTH z = 1 and z = -1
 * (a2 within 1e-4 of -1), where no one basis serves; a CPU restatement of the
 * scan measures up to 6 e32 there.  At bufsize 512 and 1024 the scan's form,
 * and with it the last bits of a track, depends on `tracks` (from 16 384 on
 * the buffer is scanned in 256-sample segments).  Any other bufsize, unaligned
 * buffers, and a section that is outside the stability triangle (|a2| < 1,
 * |a1| < 1 + a2) or holds a value that is not finite take gab_iir_sequential's
 * kernel and give its bits.
 * gab_iir_sequential: one lane per track in the golden's exact operation order,
 * bit-identical to it.                                                        */
int gab_iir(const float* d_in, float* d_out, const float* coeffs,
            float* d_state, int tracks, int bufsize, gab_stream_t stream);
int gab_iir_sequential(const float* d_in, float* d_out, const float* coeffs,
                       float* d_state, int tracks, int bufsize, gab_stream_t stream);

/* Conv1DTextureMemoryImplKernel (cuda/bench_conv1d.cu:7-27) with the CPU
 * golden's semantics (:188-208): y[t*B+i] = sum_j h[t*L+j] * x_flat[t*B+i-j]
 * over the FLAT input (history = previous track), j ascending.  d_ir is
 * T x L track-major (replaces the 2-D texture).                              */
int gab_conv1d(const float* d_in, float* d_out, const float* d_ir, int ir_len,
               int tracks, int bufsize, gab_stream_t stream);

/* The same for a channel SHARD (additive): d_in starts halo_tracks tracks BEFORE the first of the
 * `tracks` computed — the preceding tracks' rows, whose last ir_len-1 samples are the first track's history in
 * the golden's flat indexing (halo_tracks = min(first global track, ceil((ir_len-1)/bufsize))); d_ir and d_out
 * hold the computed tracks only.  halo_tracks = 0 is gab_conv1d.                                        */
int gab_conv1d_shard(const float* d_in, float* d_out, const float* d_ir, int ir_len,
                     int tracks, int bufsize, int halo_tracks, gab_stream_t stream);

/* RndMemKernel (cuda/bench_rndmem.cu:7-20): out[T*i+t] = pool[playhead[t]+i].
 * pool_elems is used to range-check nothing on device; it is the caller's
 * promise that playhead[t]+bufsize <= pool_elems.  Bit-exact copy.           */
int gab_rndmem(const float* d_pool, const int* d_playheads, float* d_out,
               int tracks, int bufsize, gab_stream_t stream);

/* ModalSynthesisKernel (cuda/bench_modal.cu:15-36), placeholder semantics:
 * out[i*B+s] = params[8i+0] * Re(exp(0.5+0.5i)) for i < out_tracks.           */
int gab_modal(const float* d_params, float* d_out, int n_modes, int bufsize,
              int out_tracks, gab_stream_t stream);

/* The real bank — the reference's Metal kernel BenchmarkModalFilterBank
 * (metal-swift/MetalSwiftBench/Metal/kernels_benchmark_staging.metal:121-162; golden
 * Benchmarks/ModalFilterBankBenchmark.swift:73-101) on the same 8-float parameter
 * records: out[(m % out_tracks)*B + i] = sum over modes of amp * Re(state * e^{i 2 pi f (i+1)}),
 * fp32 phasor recurrence, fixed summation order (no atomics).  out_tracks in 1..64;
 * d_params 16-byte aligned; d_workspace holds gab_modal_bank_workspace_bytes().  */
size_t gab_modal_bank_workspace_bytes(int n_modes, int out_tracks, int bufsize);
int gab_modal_bank(const float* d_params, float* d_out, int n_modes, int bufsize, int out_tracks,
                   float* d_workspace, gab_stream_t stream);
/* The launch gab_modal_bank makes for a shape: *J modes per lane (1, 2, 4; 8 with 32 tracks only), *grid workgroups,
 * *fixed_tracks = 1 for the instantiation with the track count at compile time (out_tracks == 32).  The same host
 * function decides for gab_modal_bank; no device call (tests/test_launch_forms_gpu.py).                         */
int gab_debug_modal_launch(int n_modes, int out_tracks, int* J, int* grid, int* fixed_tracks);

/* WaveguideState (cuda/bench_dwg.cuh:19-28), 32 bytes.                       */
typedef struct {
    int   length, inputTapPos, outputTapPos, writePos;
    float gain, reflection, damping, padding;
} gab_waveguide_state;

#define GAB_DWG_NAIVE 0   /* DWG1DNaiveKernel (cuda/bench_dwg.cu:10-59)       */
#define GAB_DWG_ACCEL 1   /* DWG1DAccelKernel (cuda/bench_dwg.cu:61-141)      */
/* Workspace the ordered (atomic-free) output reduction needs, in bytes: the tap contributions [n][bufsize], then
 * (since round 3) where every line reaches its tap, the per-sample hit counters and the hit lists.  gab_dwg takes no
 * size argument and writes ALL of these on every call: d_workspace MUST hold at least what this function returns
 * for the same (n_waveguides, bufsize) — a buffer sized n*bufsize floats by an older reading of this header is too
 * small and would be written past its end.                                                                */
size_t gab_dwg_workspace_bytes(int n_waveguides, int bufsize);
/* Updates the two delay-line banks (n_wg x max_len) in place and writes the
 * mono mix d_out[bufsize], summed over waveguides in index order.
 * GAB_DWG_ACCEL with 2048 or more mixed waveguides and bufsize <= 2048 keeps its per-sample hit counters in one of 16
 * slots of the library (not in d_workspace: they must be zero before the call's first append), picked round robin:
 * at most 16 such calls may be in flight at once per device (calls on one stream never are).                     */
int gab_dwg(const gab_waveguide_state* d_wg, float* d_fwd, float* d_bwd,
            const float* d_in, float* d_out, void* d_workspace, int n_waveguides,
            int bufsize, int max_len, int out_tracks, int variant,
            gab_stream_t stream);
/* The kernels gab_dwg launches for a shape: *cells advances the delay lines, *mix is how the ordered per-sample sum finds
 * its contributions.  The same host function decides for gab_dwg; no device call (tests/test_launch_forms_gpu.py).  */
#define GAB_DWG_CELLS_NAIVE         0   /* dwg_naive_kernel (GAB_DWG_NAIVE)                                        */
#define GAB_DWG_CELLS_ONE_LINE      1   /* dwg_cells_kernel: one line per workgroup, fewer than 1024 lines         */
#define GAB_DWG_CELLS_MULTI         2   /* dwg_cells_multi_kernel<8>: 1024 lines and more                          */
#define GAB_DWG_CELLS_LEAN          3   /* dwg_cells_lean_kernel<4>: 2048 mixed lines and more, bufsize <= 2048    */
#define GAB_DWG_CELLS_APPEND_STAGED 4   /* dwg_cells_append_kernel<8, true>: the same with 4 GiB of lines and more */
#define GAB_DWG_MIX_SCAN            0   /* dwg_mix_kernel scanning every waveguide per sample                      */
#define GAB_DWG_MIX_GATHER_SPARSE   1   /* dwg_gather_kernel, then dwg_mix_kernel on hit lists in the workspace    */
#define GAB_DWG_MIX_APPENDED_SPARSE 2   /* the cells kernel appended the lists itself (counters in a library slot) */
int gab_debug_dwg_route(int n_waveguides, int bufsize, int max_len, int out_tracks, int variant, int* cells, int* mix);

/* cufftExecR2C, N=1024, batch = tracks (cuda/bench_fft.cu:63,105):
 * d_in tracks x 1024 real, d_out tracks x 513 interleaved complex.
 * Channel pairs.  Tracks 2q and 2q+1 share one complex transform (z = x_a + i x_b; an odd last track beside
 * zeros), so a track's absolute error in any bin is bounded by its PAIR's spectral peak, not its own: measured
 * 2.7e-7 .. 3.5e-7 of (peak_a + peak_b), a plain float32 restatement 1.0e-7 .. 1.25e-7 (profiles/r18_conv_levels.txt;
 * tests/test_fft_levels_gpu.py holds the kernel within four times the restatement).  A silent track beside a loud
 * partner is not silent: it holds the partner's rounding error, -131 dB of the partner's peak.  A silent pair gives
 * zeros.  A pair depends on nothing outside itself, bit for bit; a NaN or an infinity in one track makes its
 * partner's spectrum non-finite too and touches no other pair.                                              */
int gab_fft_r2c_1024(const float* d_in, float* d_out, int tracks,
                     gab_stream_t stream);

/* ===================================================================== */
/* P. plans                                                              */
/* ===================================================================== */

/* ---- FFT convolution (Conv1DAccelBenchmark, cuda/bench_conv1d_accel.cu) -- */
typedef struct gab_conv_plan gab_conv_plan;

#define GAB_CONV_STATELESS 0  /* reference semantics: zero history each call  */
#define GAB_CONV_STREAMING 1  /* overlap-save with carried history            */
/* How a streaming plan cuts the taps.  Default SPLIT where the shape allows (512-sample buffers,
 * 1025..4096 taps, channel count divisible by 4), else CLASSIC; gab_conv_set_scheme changes it on a
 * fresh plan (before the first buffer or right after a reset).  A plan keeps its cut until then:
 * gab_conv_process (device or pinned host buffers) and gab_conv_process_batch all launch that cut.
 *   CLASSIC  taps [0,512) + [512,4096), both transforms in one workgroup per channel pair;
 *   SPLIT    taps [0,512) + [512,1024) + [1024,4096): the far partition runs for a pair every
 *            other buffer, one buffer ahead.  Same convolution, different rounding: results agree
 *            to ~1e-7 of the peak, not bit for bit.
 * Other power-of-two buffer sizes (32..2048) and responses up to 16384 taps run the fused
 * uniform-partition kernel (one cut, no choice); anything else the direct-form last resort.
 * gab_conv_set_ir on a plan that is mid-stream takes effect with the next buffer; on the SPLIT cut
 * the far shares already parked for the next two buffers were made with the previous taps.       */
#define GAB_CONV_SCHEME_CLASSIC 0
#define GAB_CONV_SCHEME_SPLIT 1
/* FDL: long impulse responses — uniformly partitioned overlap-save with a frequency-domain delay line
 * (partition = the buffer, B; transform 2B; K = ceil(ir_len / B) partitions, one complex multiply-add per
 * bin and partition per buffer).  Chosen at creation only, by gab_conv_create_scheme; gab_conv_create's
 * routing is unchanged.  Shapes: bufsize a power of two from 128 to 2048, tracks >= 1 (an odd last channel
 * is paired with a zero partner), 1 <= ir_len <= 2^21.  Supported: set_ir (every partition at once, also
 * mid-stream: from the next buffer on the output is bit-identical to a plan that had the new taps from the
 * start), reset, destroy, process (STATELESS / STREAMING / STREAMING_HOST_IO), process_batch (bit-identical
 * to per-buffer calls), get_scheme, state_bytes (spectra: the taps' spectra; history: the delay line and the
 * previous block; the plan's scratch — partial sums, a stateless call's spectrum — is not counted).  The round-trip, newest-block and engine entries, and set_scheme to another cut, refuse
 * with GAB_ERR_INVALID_ARG and leave the plan usable.                                                 */
#define GAB_CONV_SCHEME_FDL 2
/* Channel pairs.  Every FFT route — CLASSIC, SPLIT (their batch, host-I/O, round-trip and engine launches too), the
 * taps <= 512 cut, the uniform-partition kernel and FDL — packs channels 2q and 2q+1 into one complex transform,
 * z = x_a + i x_b (an odd last channel beside zeros); the direct form packs nothing.  What follows from that, as
 * measured per channel at unequal levels (profiles/r18_conv_levels.txt, tools/conv_levels.py) and held by
 * tests/test_conv_levels_gpu.py:
 *   - a channel's absolute error is bounded by its PAIR's level, not its own: a few 1e-7 of
 *     (peak_a + peak_b), the two channels' output peaks (measured 3.0e-7 .. 4.2e-7 on the 512-sample cuts and FDL,
 *     5.6e-7 .. 6.1e-7 on the uniform kernel; a plain float32 restatement of the same cuts loses 2.0e-7 .. 2.6e-7,
 *     and the tests hold every route within four times its restatement).  A channel 2^-20 below its partner
 *     therefore carries an error near 0.1 of its own peak; a pair whose channels are both quiet is as accurate,
 *     relative to itself, as a loud one.  The direct form: 1.3e-6 of the channel's own peak at 700 taps.
 *   - a silent channel beside a loud partner is NOT silent: it holds the partner's rounding error, -129 .. -140 dB
 *     of the partner's peak (-138 .. -142 dB in the restatement).  On the direct form it is zeros.
 *   - a pair whose two channels are silent gives zeros (of either sign), whatever the other pairs carry.
 *   - a pair's output depends on nothing outside the pair, bit for bit: not on the other pair of a SPLIT duo (which
 *     shares its workgroup and LDS), not on the level or content of any other channel.
 *   - a NaN or an infinity in one input sample makes BOTH channels of its pair non-finite, in every buffer whose
 *     transforms hold the sample, and touches no other pair.  The pair is the clean stream's bits again after
 *     exactly 2 buffers (the struck one included) with taps <= 512, 9 on CLASSIC, 10 or 9 on SPLIT (its far window is
 *     a block longer than its taps and is transformed a buffer ahead, for a pair every other buffer: which of the two
 *     depends on whether the strike meets the pair's turn), (4096 + B + (J-2)(4096-B)) / B on the uniform kernel
 *     with J > 1 partitions (4096 / B with one; 17, 17 and 129 buffers at 256 x 3000, 1024 x 16384 and 32 x 700),
 *     K + 1 on FDL; the direct form keeps it at most ceil((ir_len-1) / bufsize) + 1 buffers, in the struck channel
 *     alone.  While it lasts, gab_conv_process_batch and per-buffer launches agree in which values are NaN, not in
 *     the NaNs' sign bits (SPLIT).                                                                              */
int gab_conv_set_scheme(gab_conv_plan* plan, int scheme);
int gab_conv_get_scheme(const gab_conv_plan* plan, int* scheme);
#define GAB_CONV_STREAMING_HOST_IO 2  /* the same, d_in / d_out in pinned host memory: identical kernel
                                       * under its own name, so that link-speed launches do not
                                       * mix into per-kernel profiles of the HBM-resident ones    */

/* allocateAccelBuffers + setupFFTPlans (:88-150).  Allocates the spectra bank
 * and the history ring on the current device.                                */
int gab_conv_create(gab_conv_plan** plan, int tracks, int bufsize, int ir_len);
/* gab_conv_create with the cut named: CLASSIC / SPLIT = gab_conv_create then gab_conv_set_scheme (same
 * errors); FDL = a plan of that scheme.  Arguments are checked before any device call.                  */
int gab_conv_create_scheme(gab_conv_plan** plan, int tracks, int bufsize, int ir_len, int scheme);
int gab_conv_destroy(gab_conv_plan* plan);
/* precomputeImpulseResponseFFTs (:175-228): d_ir is tracks x ir_len floats on
 * the device.  Synchronous with respect to `stream`.  Mid-stream, on every
 * route: new taps from the next buffer on; bit-identical to a plan that had
 * them from the start, except the split cut's first buffer, which is equal to
 * rounding (its far share of the next two blocks is recomputed here from the
 * history).  Ordered after every launch queued on any stream since the last
 * reset: those run with the taps they were queued under.                     */
int gab_conv_set_ir(gab_conv_plan* plan, const float* d_ir, gab_stream_t stream);
/* Forget all history (the state a freshly created plan has).  Ordered after
 * launches queued on other streams; a later launch on another stream waits
 * for it.                                                                    */
int gab_conv_reset(gab_conv_plan* plan, gab_stream_t stream);
/* One buffer: d_in track-major T x B, d_out sample-major [T*s+t]
 * (performBenchmarkIteration :258-304 without the host copies).  d_in / d_out
 * must be device-ACCESSIBLE: device memory, or pinned host memory
 * (hipHostMalloc), in which case the kernel moves the buffer over PCIe itself
 * (zero-copy round trip: 94 us against 117 us with copy commands at C3).      */
int gab_conv_process(gab_conv_plan* plan, const float* d_in, float* d_out,
                     int mode, gab_stream_t stream);
/* n_buffers consecutive buffers in ONE launch (streaming mode): d_in = [n][T*B]
 * track-major buffers back to back, d_out = [n][B*T].  Same results, bit for bit, as n calls of
 * gab_conv_process; for callers whose input is resident ahead of time (offline rendering, and
 * bench.py's throughput figure): no kernel boundary between buffers.  On the split cut a 768-thread
 * workgroup owns a duo of channel pairs for the whole launch, near role on four waves, far role on
 * two groups of four (conv_split_batch12_kernel).  A call of more than 256 buffers goes out as launches of at most 256 on
 * `stream` (a launch boundary keeps the workgroups in step: over many hundred buffers they drift apart and the output
 * lines leave the L2s in pieces — 5.63 against 5.10 us per buffer at 2048; profiles/r05_batch_buffers_per_launch.txt).
 * Additive: the reference processes one buffer per iteration.                                                      */
int gab_conv_process_batch(gab_conv_plan* plan, const float* d_in, float* d_out,
                           int n_buffers, gab_stream_t stream);
/* One buffer from pinned host memory to pinned host memory, returning when h_out holds the result — the
 * reference's whole iteration (transferToDevice, the pipeline, transferToHost: cuda/bench_base.cu:30-42 +
 * bench_conv1d_accel.cu:258-304) with both link directions busy at once.  Streaming mode, same state and same
 * bits as gab_conv_process on device buffers.  On a CLASSIC-cut plan (512-sample buffers, 513..4096 taps,
 * channel count divisible by 4) the upload is one engine copy into a staging buffer that the kernel — launched
 * at once, its history-only partition first — consumes as it lands, and the outputs go back in channel groups
 * while later groups are still arriving (conv_round_trip_kernel).  Other plans: the kernel moves both buffers
 * over the link itself (as GAB_CONV_STREAMING_HOST_IO; h_in must then be pinned as well) and the call waits
 * for the stream.  h_out must be pinned (hipHostMalloc) — the kernel writes it.  h_in: pinned for the overlap; pageable
 * memory is accepted and uploaded completely before the launch (the kernel consumes an upload as it lands only when every
 * word is written exactly once and in one piece, which engine copies from pinned memory do when no engine packet ends
 * inside a word: the upload goes out in pieces of 4 MiB - 256 bytes; and a staging word counts as landed when its top
 * byte is no longer the sentinel's 0xff, so input words that are negative NaNs, -inf or below -1.7e38 wait for the
 * upload's completion instead: slower, same bits).  h_in is read from the moment of the
 * call on the plan's own upload stream: it must be complete by then (the upload is NOT ordered behind work queued on
 * `stream`).  Blocking; one call at a time per plan.  The call returns when the LAUNCH HAS ENDED on `stream`
 * (the launch's own stop event has completed): from then on h_out is the host's and the staging buffer the next call's — the completion
 * rule of cuda/bench_base.cu:30-42,177-179 (copy back after a device synchronisation), not a word the kernel writes.
 * GAB_ERR_RUNTIME if the input never arrived: the output of that call is then invalid AND so is the
 * plan's carried history (the kernel took placeholders for samples) — gab_conv_reset before the stream goes on;
 * the staging buffer has been re-armed, the next call works.  A launch that could not be made leaves the plan as it
 * was (history, epoch, staging buffer).                                                                      */
int gab_conv_round_trip(gab_conv_plan* plan, const float* h_in, float* h_out, gab_stream_t stream);
/* The overlapped round trip's kernel takes input words while the upload is still running: that rests on engine writes landing
 * whole and once (an observation; a violation was silent wrong audio once: profiles/r05_incident_torn_word.txt).  Since round 6
 * a second, small launch behind every call — on the same stream, ordered behind the UPLOAD'S COMPLETION EVENT — compares the
 * words the kernel consumed (the plan's newest history block) with what the completed upload left in the staging buffer and
 * only then re-arms the buffer.  It costs the call nothing: the call returns on the main launch's end, as before.
 *   set_check(plan, 1)  (default) the verdict is read by a FOLLOWING gab_conv_round_trip on the plan — the next one when the
 *                       check launch is through by then (one call per audio slot), the one after it for back-to-back calls
 *                       (the plan has two staging buffers, taken in turn, so that no call waits for the previous call's check) —
 *                       which then returns GAB_ERR_RUNTIME: an EARLIER buffer's output was wrong, gab_conv_reset before the
 *                       stream goes on; or by gab_conv_round_trip_check (after the last buffer of a stream);
 *   set_check(plan, 2)  the call itself waits for the verdict (15-20 us more per call: the upload's completion event goes
 *                       through the command processor) and fails AT the call;
 *   set_check(plan, 0)  the verdict is ignored (the check launch still re-arms the buffer).
 * (The check cannot run INSIDE the kernel for free: the earliest "the upload is complete" that reaches a running kernel
 * arrives 14-20 us after the last byte — measured both ways, profiles/r06_roundtrip_check.txt.)                              */
int gab_conv_round_trip_check(gab_conv_plan* plan);
int gab_conv_round_trip_set_check(gab_conv_plan* plan, int mode);
/* Every later gab_conv_round_trip of this plan ends with a gab_keep_warm_kick (see keep-warm above); on = 0 stops kicking. */
int gab_conv_round_trip_keep_warm(gab_conv_plan* plan, int on);
/* gab_keep_warm_placement of the plan's own keep-warm launch (started = 0 if the plan has none). */
int gab_conv_round_trip_keep_warm_placement(gab_conv_plan* plan, unsigned* hw_id, unsigned* xcc_id, int capacity, int* started);
/* The block the plan consumed LAST, as its kernels keep it (the newest slot of the history ring of a 512-sample
 * plan), written to d_out in the input's layout [tracks][512].  An inspection call (additive): after
 * gab_conv_round_trip it must equal that call's h_in word for word — the check of the upload hand-off that tests
 * and tools/roundtrip_stress.py make.                                                                         */
int gab_conv_newest_block(gab_conv_plan* plan, float* d_out, gab_stream_t stream);
/* ---- a resident engine fed through a doorbell (additive; split-cut plans) -----------------------------------------
 * For a caller whose buffers ARRIVE one at a time but who can keep a couple in flight: ONE launch (the batch launch's
 * kernel) stays on the device and convolves buffer k as soon as the host — or anything that can write the slot — has
 * published it, so no kernel boundary separates buffers (conv_split_kernel: 8.9 us per buffer; the engine: the batch
 * rate).  Same state, same bits as gab_conv_process.
 *   rings     allocates (once per ring size) input / output rings of ring_buffers slots ([slot][T*B] track-major in,
 *             [slot][B*T] sample-major out; ordinary device memory that the launch reads with system-scope loads and
 *             writes with write-through stores: COPY ENGINES may write and read them while the launch runs — kernels
 *             cannot: at 1024 channels the engine holds every compute unit until it stops);
 *   start     the same rings, and launches BEHIND what `stream` holds at the call, on a stream of the plan's own at the
 *             highest priority (the runtime maps streams onto a few hardware queues per priority; work that shared a queue with
 *             the resident launch would stand behind it until stop — at normal priority a copy on another stream did);
 *   publish   after buffer k has been written to slot k % ring_buffers: the doorbell count goes up by n_more;
 *   submit    publish with a rung: flush != 0 says "finish what is published, do not wait for more" — the real-time form,
 *             ONE buffer in flight: a period then runs buffer k although k + 1 is not there (it requests nothing for it),
 *             a drain period delivers it and its count is reported at once; the engine idles until the doorbell moves and
 *             takes the next buffer cold (cuda/bench_conv1d_accel.cu:258-304: one buffer per iteration).  With two or more
 *             buffers pending the engine pipelines as before, whatever the rung says;
 *   completed buffers whose output is complete in its slot.  Pipelined (no flush): the engine asks for a buffer one period
 *             before it uses it, delivers one period after, counts a period later and passes the doorbell on inside the
 *             device, so buffer k is reported once k + 5 is published (or the flush / stop rung): keep at least six in
 *             flight, and a ring of at least seven slots.  A producer reuses slot k % ring only when completed > k - ring;
 *   wait      spins until completed >= count (GAB_ERR_RUNTIME after timeout_seconds, or if the engine gave up);
 *   feed_one_in_flight   the real-time loop for resident rings: n_buffers times { submit(1, flush); wait for that buffer },
 *             the host-clock time of each into latency_us[i] (may be null);
 *   feed      a host loop for resident rings: rings the doorbell n_buffers times, one buffer each, never more than
 *             `ahead` (6 <= ahead < ring_buffers) in front of `completed`;
 *   stop      rings the stop bit, waits for the launch to end (every published buffer is finished), carries the
 *             history on for the next gab_conv_process / batch / engine;
 *   round_trip   the reference's iteration through the engine (cuda/bench_base.cu:30-42 around bench_conv1d_accel.cu:258-304),
 *             ONE buffer in flight: engine copy of h_in (pinned host, [T*B]) into the next ring slot, submit(1, flush), wait for
 *             that buffer, engine copy of its slot into h_out (pinned host, [B*T]).  Same bits as gab_conv_process.  The two link
 *             legs do not overlap with the transform — gab_conv_round_trip's do, and it is the faster round trip; this entry makes
 *             the per-buffer engine a complete replacement of that iteration.  Nothing else may be in flight;
 *   set_idle_limit   how long a stalled engine waits for the doorbell to move before it ends by itself (default 4 s; 0.5 .. 3600;
 *             taken at the next start).  A real-time caller that may pause for longer than that between buffers raises it.
 * The device is the engine's while it runs (256 workgroups at 1024 channels): other kernels queue behind it — and with
 * FEWER channels a kernel on another stream may still wait until stop: the runtime maps streams onto a few hardware
 * queues, and a kernel (a device-to-device copy is one) that lands on the engine's queue stands behind the resident
 * launch.  Only copy ENGINES (pinned host <-> device copies) are sure to move the rings while the launch runs.  Every
 * workgroup of the engine must be resident at once: start refuses a plan with more channels than 4 x the workgroups the
 * device holds (1024 channels on MI355X; more channels: one engine per device over channel shards).  If the
 * doorbell does not move for the idle limit (4 s unless set) the launch ends by itself and stop / feed / wait return
 * GAB_ERR_RUNTIME; stop then carries the plan's history on from what the engine CONSUMED (its message says how many of the
 * published buffers that is): a pipelined burst without the flush rung leaves its last buffer unconsumed — publish it again
 * after the next start.  start returns GAB_ERR_INVALID_ARG while a keep-warm launch other than the plan's own is resident on
 * the device (see keep-warm above).  A wait that runs out says in gab_last_error whether the launch ever became resident
 * (never started / only some workgroups / all of them), so a hardware-queue collision or a crowded device names itself.       */
int gab_conv_engine_rings(gab_conv_plan* plan, int ring_buffers, float** d_in_ring, float** d_out_ring);
int gab_conv_engine_start(gab_conv_plan* plan, int ring_buffers, float** d_in_ring, float** d_out_ring, gab_stream_t stream);
int gab_conv_engine_publish(gab_conv_plan* plan, int n_more);
int gab_conv_engine_submit(gab_conv_plan* plan, int n_more, int flush);
int gab_conv_engine_wait(gab_conv_plan* plan, int count, double timeout_seconds);
/* 1 while the resident launch is still on the device (it ends by itself if the doorbell stops moving; stop still has to be called) */
int gab_conv_engine_running(gab_conv_plan* plan, int* running);
int gab_conv_engine_completed(gab_conv_plan* plan, int* completed);
int gab_conv_engine_feed(gab_conv_plan* plan, int n_buffers, int ahead);
int gab_conv_engine_feed_one_in_flight(gab_conv_plan* plan, int n_buffers, float* latency_us);
int gab_conv_engine_stop(gab_conv_plan* plan);
int gab_conv_engine_round_trip(gab_conv_plan* plan, const float* h_in, float* h_out);
int gab_conv_engine_set_idle_limit(gab_conv_plan* plan, double seconds);
/* Bytes of device state the plan holds: spectra, history.                    */
int gab_conv_state_bytes(const gab_conv_plan* plan, size_t* spectra_bytes,
                         size_t* history_bytes);

/* ---- FDTD3D (FDTD3DBenchmark, cuda/bench_fdtd3d.cu) ---------------------- */
typedef struct gab_fdtd_plan gab_fdtd_plan;

/* FDTD3DParams (cuda/bench_fdtd3d.cuh:68-86), the fields the kernels read.   */
typedef struct {
    int   nx, ny, nz;
    int   source_x, source_y, source_z;
    int   receiver_x, receiver_y, receiver_z;
    int   steps_per_sample;
    float dt_over_rho_dx, rho_c2_dt_over_dx, absorption_coeff;
} gab_fdtd_params;

/* Reference constants (bench_fdtd3d.cuh:12-41) for an nx*ny*nz grid; source
 * and receiver scale with the room so 52^3 gives (25,25,5)/(40,15,25).       */
int gab_fdtd_default_params(int nx, int ny, int nz, gab_fdtd_params* out);
int gab_fdtd_create(gab_fdtd_plan** plan, const gab_fdtd_params* params);
int gab_fdtd_destroy(gab_fdtd_plan* plan);
int gab_fdtd_reset(gab_fdtd_plan* plan, gab_stream_t stream);     /* zero grids */
/* runFDTD3DTimeStep (:384-438) for samples [first_sample, first_sample+n):
 * inject -> steps_per_sample x {velocity, pressure} -> extract.
 * d_in/d_out are track-major T x B.                                          */
int gab_fdtd_process(gab_fdtd_plan* plan, const float* d_in, float* d_out,
                     int tracks, int bufsize, int first_sample, int n_samples,
                     gab_stream_t stream);
/* Which form gab_fdtd_process takes.  A room whose four fields fit the chip's LDS (nx <= 128;
 * up to 8192 cells per compute unit: 128^3 on 256 CUs) runs a whole buffer in ONE launch with the fields
 * resident in LDS and registers, one block of rows per workgroup, the blocks' boundary pressures handed to the
 * neighbours through memory every step (same bits as the step kernels, 4x their speed at 128^3).  It needs
 * every workgroup on the device at once (resident launches of one process are chained per device, whatever
 * their streams; other processes' kernels are not known; plan creation checks that the device can hold the whole grid at
 * once): a workgroup that waits about a second for a neighbour gives up, that call's output is NaN, gab_fdtd_status (or
 * the next call on the plan) returns GAB_ERR_RUNTIME and the plan uses the step kernels from then on.  Larger rooms, z-slabs,
 * per-track positions and calls inside a stream capture use the step kernels.
 * *resident = 1 when the next call (outside a capture) takes the resident form, *workgroups = its grid. */
int gab_fdtd_resident(const gab_fdtd_plan* plan, int* resident, int* workgroups);
/* A host that shares the device with other work can decline the resident form: STEP = one launch per step (per
 * sample for rooms up to 56^3), no workgroup ever waits for another; AUTO (default) = resident where it fits.  Same
 * bits either way.  Takes effect with the next gab_fdtd_process.                                          */
#define GAB_FDTD_FORM_AUTO 0
#define GAB_FDTD_FORM_STEP 1
int gab_fdtd_set_form(gab_fdtd_plan* plan, int form);
/* The kernel a gab_fdtd_process call of n_samples (with `capturing` != 0: made inside a stream capture) would launch,
 * and *graph = 1 if its launches would go through the plan's own graph cache (24 launches and more, outside a capture).
 * The same host function decides for gab_fdtd_process; no device call.  tests/test_launch_forms_gpu.py holds a case
 * per form to the oracle and fails when a form has none.                                                      */
#define GAB_FDTD_KERNEL_RESIDENT    0   /* fdtd_resident_kernel: the buffer in one launch                         */
#define GAB_FDTD_KERNEL_SAMPLE_TILE 1   /* fdtd_sample_tile_kernel: one launch per sample, rooms up to 56^3 at 3 steps */
#define GAB_FDTD_KERNEL_LDS_32X8    2   /* fdtd_step_lds_kernel<32, 8>:  64 < nx <= 128, nx % 4 == 0               */
#define GAB_FDTD_KERNEL_LDS_32X16   3   /*                     <32, 16>: the same, ceil(ny / 16) * nz >= 1024      */
#define GAB_FDTD_KERNEL_LDS_64X4    4   /*                     <64, 4>:  128 < nx <= 256, nx % 4 == 0              */
#define GAB_FDTD_KERNEL_LDS_64X8    5   /*                     <64, 8>:  the same, ceil(ny / 8) * nz >= 1024       */
#define GAB_FDTD_KERNEL_STEP_VEC4   6   /* fdtd_step_vec4_kernel: every other nx % 4 == 0                         */
#define GAB_FDTD_KERNEL_STEP_SCALAR 7   /* fdtd_step_kernel: nx % 4 != 0                                           */
int gab_debug_fdtd_form(const gab_fdtd_plan* plan, int tracks, int n_samples, int capturing, int* form, int* graph);
/* Errors at the call that failed (the reference throws from the failing iteration: synchronizeAndCheck,
 * cuda/bench_base.cu:177-179).  Synchronises `stream` and returns GAB_ERR_RUNTIME if the resident launch of the
 * last gab_fdtd_process on it gave up waiting for a neighbour workgroup.  That call's output is NaN in every
 * sample (never plausible audio); the plan then takes the step kernels and wants a gab_fdtd_reset.  Without this
 * call the same error is returned by the NEXT gab_fdtd_process, gab_fdtd_reset or gab_fdtd_destroy.        */
int gab_fdtd_status(gab_fdtd_plan* plan, gab_stream_t stream);
/* Track-dependent source and receiver cells — announced and never done by the Metal port
 * ("can be made track-dependent later", kernels_fdtd3d.metal:184,217).  src_xyz / rcv_xyz: HOST
 * arrays, tracks x (x, y, z).  From then on gab_fdtd_process (with that many tracks) adds
 * 0.1*in[t,s] into track t's source cell — tracks in order, so a cell shared by several tracks
 * receives their samples in track order — and writes out[t,s] = 0.1*p[receiver cell of t].
 * tracks = 0 returns to the shared cells of the params.                                          */
int gab_fdtd_set_track_positions(gab_fdtd_plan* plan, const int* src_xyz, const int* rcv_xyz, int tracks);
/* ---- z-slab domain decomposition (Metal comments kernels_fdtd3d.metal:184,217) ----
 * A plan that owns planes [z_begin, z_end) of the global grid, with one ghost pressure plane below
 * and above and one ghost vz face plane above.  One leapfrog step needs, from the slab below, its
 * top pressure plane, and from the slab above, its bottom pressure plane and bottom vz faces:
 *   per step:  gab_fdtd_step on every slab  ->  exchange the planes gab_fdtd_halo names
 *   per sample: gab_fdtd_inject (owner of the source acts, others return at once), steps_per_sample
 *   steps, the last one with strip_sample = the sample index (owner of the receiver stores
 *   0.1 * p[receiver] into its strip).
 * gab_fdtd_process needs the whole grid in one plan.                                              */
int gab_fdtd_create_slab(gab_fdtd_plan** plan, const gab_fdtd_params* params, int z_begin, int z_end);
int gab_fdtd_owns(const gab_fdtd_plan* plan, int* owns_source, int* owns_receiver);
/* inj[s] = sum over tracks of 0.1 * in[t, s], in track order, for the whole buffer */
int gab_fdtd_source_sums(gab_fdtd_plan* plan, const float* d_in, int tracks, int bufsize, gab_stream_t stream);
int gab_fdtd_inject(gab_fdtd_plan* plan, int sample, gab_stream_t stream);
int gab_fdtd_step(gab_fdtd_plan* plan, int strip_sample /* -1: none */, gab_stream_t stream);
#define GAB_FDTD_SEND_DOWN_P  0   /* my plane z_begin      -> lower slab's GAB_FDTD_RECV_UP_P   */
#define GAB_FDTD_SEND_DOWN_VZ 1   /* my faces z_begin      -> lower slab's GAB_FDTD_RECV_UP_VZ  */
#define GAB_FDTD_SEND_UP_P    2   /* my plane z_end-1      -> upper slab's GAB_FDTD_RECV_DOWN_P */
#define GAB_FDTD_RECV_DOWN_P  3
#define GAB_FDTD_RECV_UP_P    4
#define GAB_FDTD_RECV_UP_VZ   5
/* device pointer and length (nx*ny floats) of a halo plane of the CURRENT fields */
int gab_fdtd_halo(gab_fdtd_plan* plan, int which, float** d_ptr, size_t* n_floats);
/* out[t*bufsize + s] = strip[s] for every track: the receiver's owner writes the buffer's output */
int gab_fdtd_emit(gab_fdtd_plan* plan, float* d_out, int tracks, int bufsize, gab_stream_t stream);
/* the per-sample receiver values this slab recorded (meaningful on the receiver's owner) */
int gab_fdtd_strip(gab_fdtd_plan* plan, float** d_strip, int* capacity);
/* Copy the plan's own pressure planes (nx*ny*(z_end-z_begin) floats, x fastest) to d_dst. */
int gab_fdtd_copy_pressure(gab_fdtd_plan* plan, float* d_dst, gab_stream_t stream);

/* ---- Captured calls: what a stream capture of the plans below bakes in -----------------------------------------
 * The process calls of the eq, mix, delay, meter, resample, dynamics and reverb plans allocate nothing and wait for
 * nothing, so they can be recorded into a graph (hipStreamBeginCapture), one behind the other on one stream, as the
 * blocks of a channel strip.  A capture records the launches without running them: no state moves.  All state that a
 * buffer changes is on the device and is read and written by every replay.  What the HOST decides at the call is fixed
 * by the capture, and a replay repeats it whatever the host has been told since:
 *   pending / kernel form   dynamics, delay, reverb, mix: whether a ramp is pending picks the kernel form.  Captured
 *                       with none pending, every replay runs the steady form: it reads `target` alone, so values set
 *                       with ramp = 0 are in force from the next replay and values set with ramp = 1 too, at once and
 *                       without their ramp (`current` is never brought up to them).  Captured with a ramp pending,
 *                       every replay runs the ramp form, g = fmaf(target - current, r[s], current) read from the
 *                       device's tables at the replay, and the current := target copy behind it is in the graph.  So
 *                       the first replay is the ramp buffer; behind it target - current is +0 and fmaf(+0, r, c) is c
 *                       for every c but -0.0 (which comes out as +0.0; "Values at the edges of float32", below): later
 *                       replays give the steady form's bits as
 *                       long as no table holds a -0.0; and a set with ramp = 1 between two replays is ramped in by the
 *                       next replay, as between two plain calls.  The call that was captured also cleared the host's
 *                       flag, as if the ramp had run.
 *                       The saturator's process, process_batch and apply pick their form by the same flag and behave
 *                       the same way; capture them with no ramp pending (tests/test_saturator_gpu.py).
 *                       The nlms plan's process and process_batch too (tests/test_nlms_gpu.py): the taps and the history
 *                       are on the device and move with every replay.
 *                       The fdaf plan has no ramp and no host state at all: W, X, prev and count are the device's and
 *                       move with every replay, whatever is pending or set (tests/test_fdaf_gpu.py).
 *                       The mconv plan's process and process_batch pick their launches by the same flag (a ramp buffer
 *                       takes a second product launch, the blend and the copy): capture them with no ramp pending, and
 *                       the ring, prev and count move with every replay (tests/test_mconv_gpu.py).
 *   mix's ramp_first   the same flag: in a captured process_batch of n buffers the first buffer of every replay is the
 *                       one that takes the ramp form.
 *   meter's decay       a launch argument: set_decay after the capture does not reach the replays.
 *   alignment           eq picks the scan or the sequential kernel, mix, dynamics and meter the width of their loads,
 *                       from the 16-byte alignment of the pointers given: the pointers are the graph's in any case.
 *   resample's position a launch argument, (k mod period) at the capture: every replay resamples from that position.
 *                       The captured call also advanced the host's k by its buffers, as a call that ran; with
 *                       period == 1 both are without effect and the replays are the stream's next buffers.
 *   spectrum's phase    launch arguments, (p mod H) and the frame count at the capture; the history behind the frames
 *                       is the device's and moves with every replay.  Where H divides B the phase is 0 and the count
 *                       B / H on every call, and the replays are the stream's next buffers (tests/test_spectrum_gpu.py).
 *   fdtd's ping-pong    gab_fdtd_process can be captured too (it then takes the step kernels, never the resident one).  The
 *                       pointers of the two field sets are launch arguments: a replay starts in the set that was
 *                       current at the capture.  So a captured call must swap the sets an EVEN number of times
 *                       (n_samples x steps_per_sample even; n_samples even for rooms up to 56^3 at three steps per
 *                       sample, which take one launch per sample): then every replay ends where the next one starts and
 *                       the replays are successive calls on the fields.  A captured call with an odd count is refused
 *                       with GAB_ERR_INVALID_ARG, and so is one that would have to grow the plan's strips (the first
 *                       call with a bufsize larger than any before: make it outside the capture); a refusal touches
 *                       neither the plan nor the capture.  Plain calls between two replays must leave the same set
 *                       current (an even number of swaps in all).  Held by tests/test_launch_forms_gpu.py.
 * set_* calls and reset synchronise or belong to the host and stay outside a capture.  Held by
 * tests/test_strip_gpu.py for the whole strip in one graph and for every plan alone. */

/* ---- Values at the edges of float32: what the ordered forms of the plans below do there ---------------------------
 * The mix, delay, meter, resample, dynamics and reverb plans, and the equaliser's and gab_iir's sequential forms, state
 * their bits as a sequence of float32 operations rounded once each.  That sentence holds over the whole of float32:
 *   subnormals     are kept.  No operation flushes an operand or a result to zero, fmaxf / fminf / floorf included: a
 *                  tail that dies away walks its carried state down through the subnormals to zero exactly as IEEE 754
 *                  arithmetic does, and a product that underflows is rounded once, to a subnormal or to a zero of the
 *                  product's sign.
 *   overflow       is IEEE 754's: a result beyond FLT_MAX after its one rounding is an infinity of its sign (FLT_MAX +
 *                  2^102 is FLT_MAX, FLT_MAX + 2^103 is +inf; fmaf(FLT_MAX, 2, -FLT_MAX) is FLT_MAX, the product is
 *                  never rounded alone); inf - inf and 0 * inf are NaN.  Finite samples can therefore put an infinity
 *                  or a NaN into whatever a plan carries; each plan's section says how long such a value stays.  The
 *                  meter's nonfinite field speaks of the samples, not of what its own arithmetic overflowed to.
 *   NaN            which NaN comes out (sign, payload) is unspecified; that it is a NaN is not.
 *   zeros          have the sign that the stated sequence of operations gives: x * y has the product of the signs, an
 *                  exact zero sum is +0 unless both addends are -0.  So fmaf(+0, r, c) is c for every c but -0.0: a
 *                  table value of -0.0 is a -0.0 on a buffer without a ramp and a +0.0 on a ramp buffer on which its
 *                  row did not move.  A mix bus sums from +0.0 and never gives -0.0.
 * Held by tests/test_edges_host.py (the restatements against exact rational arithmetic, and that the cases reach
 * these values) and tests/test_edges_gpu.py (the kernels against the restatements bit for bit, every carried state
 * included).  The scan forms of the equaliser and of gab_iir are held to float64 by a bound, not to this. */

/* ---- biquad cascades: a parametric equaliser per track (additive; no counterpart in the reference, whose
 * IIRFilterKernel runs ONE biquad shared by every track) --------------------------------------------------
 * `tracks` channels, `sections` second-order sections in series on each (1..16), every (track, section) with its
 * own coefficients {b0,b1,b2,a1,a2} (a0 = 1; gab_iir's order), the DF-II state (z1, z2 as gab_iir documents it)
 * carried from buffer to buffer: state layout [tracks][sections][2].
 *   process             one buffer.  d_in / d_out track-major [t*B + s]; d_out == d_in (in place) is allowed — a wave
 *                       has read all of its samples before it writes any.  bufsize a power of two from 64 to 2048
 *                       with 16-byte aligned buffers takes the scan kernel (gab_iir's wave scan, once per section on
 *                       samples that stay in registers: one read and one write of the audio whatever `sections` is;
 *                       re-associates the recurrence: equal to the ordered form to rounding, not bit for bit); every
 *                       other bufsize >= 1, and unaligned pointers, the sequential kernel, as gab_iir falls back.
 *                       Which scan a plan runs (gab_eq_form) is fixed at creation from (bufsize, sections) alone,
 *                       never from `tracks`: a track's bits do not depend on how many other tracks the plan holds,
 *                       so a channel shard equals the unsharded job bit for bit.
 *   process_batch       n_buffers buffers back to back, [n][T*B], in ONE launch, the state running through: same
 *                       bits as n calls of process (a batch is more segments of the same scan).  A plan without a
 *                       scan form (or unaligned pointers) launches the sequential kernel once per buffer.
 *   process_sequential  one lane per track, every section in the ordered form of gab_iir_sequential (one rounding
 *                       per operation): with one section and the same coefficients on every track, its bits.
 *                       process and process_sequential share the plan's state; switching between them mid-stream
 *                       is allowed and equal to rounding.
 *   set_coeffs          d_coeffs: device, [tracks][sections][5].  The scan's constants are made on the device in
 *                       float64 and rounded once.  Synchronous with respect to `stream`.  A section outside the
 *                       stability triangle (|a2| < 1, |a1| < 1 + a2) or with a value that is not finite:
 *                       GAB_ERR_INVALID_ARG naming the first such (track, section); the plan then keeps the
 *                       coefficients it had.  Mid-stream the new coefficients take effect with the next buffer and the
 *                       carried state is kept as it is: the output is the ordered form run with the coefficients
 *                       switched at that buffer boundary.
 *   set_coeffs_tracks   the same for tracks [first_track, first_track + n_tracks), d_coeffs [n_tracks][sections][5]:
 *                       one channel's knobs moved; no other track's bits change.
 *   reset               zero state.    state: the plan's own state array, for inspection.
 *   form                the scan's samples per lane and segments per buffer; 0, 0: the sequential kernel only.
 * A new plan is the identity filter (b0 = 1, everything else 0) with zero state.  tracks >= 1, bufsize >= 1,
 * 1 <= sections <= 16; arguments are checked before any device call.  One thread at a time per plan.           */
typedef struct gab_eq_plan gab_eq_plan;
int gab_eq_create(gab_eq_plan** plan, int tracks, int bufsize, int sections);
int gab_eq_destroy(gab_eq_plan* plan);
int gab_eq_set_coeffs(gab_eq_plan* plan, const float* d_coeffs, gab_stream_t stream);
int gab_eq_set_coeffs_tracks(gab_eq_plan* plan, const float* d_coeffs, int first_track, int n_tracks,
                             gab_stream_t stream);
int gab_eq_reset(gab_eq_plan* plan, gab_stream_t stream);
int gab_eq_process(gab_eq_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_eq_process_batch(gab_eq_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_eq_process_sequential(gab_eq_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_eq_state(gab_eq_plan* plan, float** d_state, size_t* n_floats);
int gab_eq_form(const gab_eq_plan* plan, int* samples_per_lane, int* segments);

/* ---- mix bus: tracks summed into buses with ramped gains, in a fixed order (additive; no counterpart in the
 * reference, whose kernels are per track) ---------------------------------------------------------------------
 * out[m][s] = sum over t of g[t][m] x[t][s]: `tracks` channels into `buses` buses (1..64), a linear gain per
 * (track, bus).
 *   gains          device, [tracks][buses] float32.  The plan carries two matrices: `current` (what the last processed
 *                  sample was mixed with) and `target`; a new plan has both zero: silence.
 *     set_gains(ramp = 1)  target := the new matrix, current stays.  The next processed buffer is mixed with
 *                  g(t, m, s) = fmaf(target - current, r[s], current), r[s] = (s + 1) / bufsize (a table made on the
 *                  host in float64, rounded once, uploaded at creation: no device division enters the bits); after
 *                  that buffer current := target exactly.  Two sets before a buffer: the ramp still starts from
 *                  current, the audible gains.
 *     set_gains(ramp = 0)  current := target := the new matrix, at once.
 *     set_gains_tracks     the same for rows [first_track, first_track + n_tracks), d_gains [n_tracks][buses]; the other
 *                  rows keep their current and target.  Whether a ramp is pending is one fact of the whole plan, which a
 *                  set with ramp = 0 does not change: on rows whose ramp is pending it puts current and target at the new
 *                  values at once, and the next buffer still ramps every other row from its current to its target.  (So
 *                  for every plan with a ramped table: delay, dynamics, reverb, gate.)
 *                  A value that is not finite: GAB_ERR_INVALID_ARG naming the first such (track, bus); the plan keeps
 *                  what it had.  Both are synchronous with respect to `stream` and take effect with the next buffer.
 *     reset        current := target (a pending ramp is dropped).      gains: the plan's own two arrays, for inspection.
 *   process        one buffer.  d_out is bus-major [m*B + s] (track-major with the buses as tracks: a bus can go straight
 *                  into a gab_eq_plan of `buses` tracks).  d_in in either layout, named by `layout`; the two layouts
 *                  give the same bits for the same samples.  d_in and d_out must not overlap.  Any bufsize, any
 *                  tracks, any alignment: 16-byte aligned pointers with bufsize a multiple of 4 take the fast
 *                  kernels, everything else a general kernel with the same bits.
 *   process_batch  n_buffers buffers back to back ([n][T*B] in, [n][M*B] out) in one launch; a pending ramp runs through
 *                  the first of them; same bits as n calls of process.  One launch takes as many buffers as the plan's
 *                  workspace holds partial sums for (sized at creation: 32 MiB's worth, at least 1 and at most 64
 *                  buffers; plans of up to 256 tracks need none and take 64); a longer batch is that many per launch,
 *                  one launch after the other.  process and process_batch allocate nothing and wait for nothing.
 * The bits of one output, with g = target[t][m] on a buffer without a pending ramp and the ramp formula on a buffer
 * with one (then for every track, also those whose row did not move):
 *   1. leaf:  leaf_tracks consecutive tracks, acc = 0.0f; for t ascending: acc = fmaf(g, x[t][s], acc);
 *   2. group: group_leaves consecutive leaves added in ascending order with plain float adds, from the first leaf's value;
 *   3. the groups added in ascending order the same way.  A last leaf or group may be short.
 * No float atomics: the order is a function of the indices alone.  leaf_tracks and group_leaves are fixed at creation
 * from (bufsize, buses) alone — never from tracks, the layout, the device or the batch length — and gab_mix_form
 * reports them: a plan's bits are the same on every box, and one restatement of the three steps above, given those two
 * integers, is the kernel's bits for every shape.
 * tracks >= 1, bufsize >= 1, 1 <= buses <= 64, and ceil(tracks / 256) * ceil(bufsize / 64), the workgroups one buffer
 * takes, below 2^31; arguments are checked before any device call.  One thread at a time per plan.                  */
typedef struct gab_mix_plan gab_mix_plan;
#define GAB_MIX_TRACK_MAJOR  0   /* d_in [t*B + s]: what gab_eq_process, gab_gain, gab_iir write */
#define GAB_MIX_SAMPLE_MAJOR 1   /* d_in [T*s + t]: what gab_conv_process writes                 */
int gab_mix_create(gab_mix_plan** plan, int tracks, int bufsize, int buses);
int gab_mix_destroy(gab_mix_plan* plan);
int gab_mix_set_gains(gab_mix_plan* plan, const float* d_gains, int ramp, gab_stream_t stream);
int gab_mix_set_gains_tracks(gab_mix_plan* plan, const float* d_gains, int first_track, int n_tracks, int ramp,
                             gab_stream_t stream);
int gab_mix_reset(gab_mix_plan* plan, gab_stream_t stream);
int gab_mix_process(gab_mix_plan* plan, const float* d_in, float* d_out, int layout, gab_stream_t stream);
int gab_mix_process_batch(gab_mix_plan* plan, const float* d_in, float* d_out, int n_buffers, int layout,
                          gab_stream_t stream);
int gab_mix_gains(gab_mix_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_mix_form(const gab_mix_plan* plan, int* leaf_tracks, int* group_leaves);

/* ---- delay: a delay line per track, read at a fractional position, with feedback and ramped parameters (additive;
 * the reference's waveguide has fixed integer lengths and its own reflection rule) ------------------------------
 * Latency compensation and pre-delay (feedback 0), echo and comb (feedback), chorus and flanger (a delay that moves).
 *   parameters     device, [tracks][4] float32 = {delay, feedback, wet, dry}, delay in samples.  The plan carries two
 *                  tables, `current` and `target`; a new plan has {min_delay, 0, 0, 1} in both on every track
 *                  (pass-through) and a zero line.
 *     set_params(ramp = 1)  target := the new table, current stays.  On the next processed buffer every parameter p of
 *                  every track is p[s] = fmaf(target - current, r[s], current), r[s] = (s + 1) / bufsize (a table made on
 *                  the host in float64, rounded once, uploaded at creation; target - current rounded once); after that
 *                  buffer current := target by a copy.  Two sets before a buffer: the ramp still starts from current.
 *     set_params(ramp = 0)  current := target := the new table, at once.
 *     set_params_tracks     the same for rows [first_track, first_track + n_tracks), d_params [n_tracks][4]; the other
 *                  rows keep their current and target.
 *                  The values are checked on the device first: every value finite, min_delay <= delay <= max_delay,
 *                  |feedback| < 1.  A violation: GAB_ERR_INVALID_ARG naming the first (track, field) in index order
 *                  (field 0 delay, 1 feedback, 2 wet, 3 dry); the plan keeps what it had.  Both calls are synchronous
 *                  with respect to `stream` and take effect with the next buffer.
 *     reset        the lines and write positions zero, current := target, a pending ramp dropped: the stream that
 *                  follows is a new plan's with the same target.
 *     params       the plan's own two tables, for inspection.
 *     line         the ring's base ([tracks][capacity] float32), the capacity (a power of two >= max_delay + 3 +
 *                  bufsize) and the per-track write positions ([tracks] unsigned: the ring index of the next sample),
 *                  for inspection.
 *   process        one buffer, track-major [t*B + s] in and out, as gab_eq_process takes and writes.  d_out == d_in is
 *                  allowed (no other overlap).  Any bufsize, any alignment, any track count: the same bits.
 *   process_batch  n_buffers buffers back to back ([n][T*B]) in one launch; a pending ramp runs through the first of
 *                  them; same bits as n calls of process.  process and process_batch allocate nothing and wait for
 *                  nothing; the write position is device state.
 * The bits of one sample.  On a buffer without a pending ramp p = target, on one with a ramp the formula above, for all
 * four parameters.  Then the delay, and only the delay, is clamped: d = fminf(fmaxf(d, min_delay), max_delay).  The
 * clamp is a guard that is part of the bits: a tap below min_delay would read the sample being written, so the kernel
 * does not rest on an argument about roundings.  For the tables set_params admits it never acts downwards (min_delay -
 * current is a float32 and rounding is monotone, so the ramp's value is at least min_delay for every r in (0, 1]); a
 * ramp's value between its ends is simply kept inside [min_delay, max_delay].  For absolute sample n of a track, x the input, w the line (zero before
 * the first sample and after a reset):
 *     i  = (int)floorf(d);   fr = d - (float)i                      (exact)
 *     GAB_DELAY_LINEAR (min_delay 1):
 *       a = w[n-i];  b = w[n-i-1];   v = fmaf(fr, b - a, a)         (b - a rounded once)
 *     GAB_DELAY_LAGRANGE3 (min_delay 2), the third-order Lagrange weights of the points -1, 0, 1, 2 at fr, every
 *     difference, sum and product below rounded once, products taken left to right, fmaf only where written:
 *       am = w[n-i+1];  a = w[n-i];  b = w[n-i-1];  b2 = w[n-i-2]
 *       fm1 = fr - 1;   fm2 = fr - 2;   fp1 = fr + 1;   c6 = (float)(1.0 / 6.0)
 *       hm = ((fr  * fm1) * fm2) * (-c6)          h0 = ((fp1 * fm1) * fm2) * 0.5f
 *       h1 = ((fp1 * fr ) * fm2) * (-0.5f)        h2 = ((fp1 * fr ) * fm1) * c6
 *       v = hm * am;   v = fmaf(h1, b, v);   v = fmaf(h2, b2, v);   v = fmaf(h0, a, v)
 *     (fr == 0: hm, h1, h2 are zeros and h0 is exactly 1, so v == w[n-i].)
 *     w[n] = fmaf(feedback, v, x[n])                                what enters the line
 *     y[n] = fmaf(wet, v, dry * x[n])                               the output (dry * x[n] rounded once)
 * Samples that are not finite: a NaN or an infinity in a track's input enters that track's line and stays until reset,
 * whatever the feedback: with feedback 0 too, since w[n] = fmaf(0, v, x[n]) is a NaN when the tap v is a NaN or an
 * infinity, so the value comes round once per delay for good.  No other track is touched.
 * Nothing else has rounding freedom: every launch form gives the same bits, and a shard of tracks as its own plan gives
 * those tracks' bits.  Precision: delay is a float32, so a delay near 2^17 samples resolves 2^-7 of a sample.
 * Stability: |feedback| < 1 bounds a linear line (its two weights are non-negative and sum to 1, loop gain |feedback|).
 * The Lagrange weights sum to 1 but their magnitudes sum to up to 1.25 (at fr = 0.5), so a worst-case signal sees a loop
 * gain of 1.25 |feedback|: only |feedback| < 0.8 bounds a Lagrange line's level and rounding-error growth for every
 * input.  Above that a value is admitted, but |feedback| < 1 alone does not give such a bound.
 * tracks >= 1, bufsize >= 1, min_delay <= max_delay <= 2^20; arguments are checked before any device call.  One thread
 * at a time per plan.                                                                                               */
typedef struct gab_delay_plan gab_delay_plan;
#define GAB_DELAY_LINEAR    0   /* two-point interpolation, min_delay 1  */
#define GAB_DELAY_LAGRANGE3 1   /* four-point interpolation, min_delay 2 */
int gab_delay_create(gab_delay_plan** plan, int tracks, int bufsize, int max_delay, int interp);
int gab_delay_destroy(gab_delay_plan* plan);
int gab_delay_set_params(gab_delay_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_delay_set_params_tracks(gab_delay_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                                gab_stream_t stream);
int gab_delay_reset(gab_delay_plan* plan, gab_stream_t stream);
int gab_delay_process(gab_delay_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_delay_process_batch(gab_delay_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_delay_params(gab_delay_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_delay_line(gab_delay_plan* plan, float** d_ring, size_t* capacity, unsigned** d_pos);

/* ---- meter: per track and buffer one row of eight levels, with carried state (additive; the reference's gainstats is
 * one stateless mean and max that also writes a scaled copy of the block) -----------------------------------------
 * The input ([tracks][bufsize] float32, track-major, any alignment) is never written.  process writes d_rows
 * [tracks][8], process_batch [n][tracks][8] for n consecutive buffers in one call with the bits of n process calls.
 * Every field is linear; decibels are the caller's business.  Let w be the track's stream, zero before the first
 * sample and after a reset, x the buffer, B = bufsize, inv_B = (float)(1.0 / B), inv_W = (float)(1.0 / window).
 *   0 peak           max |x[s]| by fmaxf, from 0: a NaN is ignored.  Exact.
 *   1 true_peak      four-times oversampled peak, one polyphase pass of 12 taps per phase.  Taps of phase k = 1, 2, 3:
 *                    f = k / 4, d = 5 + f - j, h_k[j] = sinc(d) (0.5 + 0.5 cos(pi d / 6.5)), j = 0..11, in float64;
 *                    each phase divided by its sum (added in ascending j), rounded once to float32 on the host: 36
 *                    constants, no device division or transcendental function.  For absolute sample n
 *                      y_k[n] = fmaf(h_k[11], w[n-11], ... fmaf(h_k[1], w[n-1], h_k[0] * w[n]))     (ascending j)
 *                    and the field is the fmaxf, from 0 and over the buffer's n, of |w[n-5]|, |y_1[n]|, |y_2[n]|,
 *                    |y_3[n]|.  The reading lags by five samples.  Accuracy: a sine at 0.25 fs reads within 0.2 dB,
 *                    one at 0.4 fs up to 0.44 dB low, which is the limit of 12 taps.
 *   2 ms             sum(x^2) * inv_B.  The sum is a tree fixed by bufsize alone: the buffer is cut into segments of 64
 *                    samples, a short last segment is filled with zeros; in a segment every square is rounded once
 *                    (p_l = x_l * x_l, l = 0..63), then p_l = p_l + p_(l^32), then ^16, ^8, ^4, ^2, ^1 (all l at once)
 *                    and the segment's sum is p_0; the segments' sums are added in ascending order from 0.
 *   3 kms            the same tree over v^2, v being x through the two weighting sections in series.  A section is
 *                    direct form II transposed on its carried pair (s1, s2):
 *                      y = fmaf(b0, x, s1);  s1 = fmaf(b1, x, fmaf(-a1, y, s2));  s2 = fmaf(b2, x, (-a2) * y)
 *                    (the last product rounded once).  The plan runs exactly this ordered recurrence at every bufsize
 *                    (gab_eq's wave scan of a biquad re-associates too much for these two sections: DESIGN.md 4d).
 *                    The weighting is the same for every track; the default is the K weighting of ITU-R BS.1770 at
 *                    48 kHz (+0.691 dB at 997 Hz).
 *   4 peak_hold      hold = fmaxf(peak, hold * decay), the product rounded once; carried.  decay 1 (the default) holds
 *                    until reset.
 *   5 true_peak_max  the running fmaxf of field 1 since the last reset.
 *   6 kms_window     the mean of kms over the last `window` buffers: the values live in a ring per track, zero after
 *                    a reset; every buffer the ring is added from the oldest to the newest value in that order, from
 *                    0, and multiplied by inv_W.  No running sum that drifts.
 *   7 nonfinite      1.0 if any sample of the buffer was an infinity or a NaN (from the bits), else 0.0.  Such a sample
 *                    poisons the carried filter state (fields 3 and 6) until reset; the plan does not repair it.
 *   set_weighting    d_sections: device, [2][5] = {b0, b1, b2, a1, a2} (a0 = 1).  Checked on the device first: every
 *                    value finite, |a2| < 1, |a1| < 1 + a2.  A violation: GAB_ERR_INVALID_ARG naming the first value
 *                    in index order (a2 for the first rule, a1 for the second); the plan keeps its weighting.  In
 *                    force from the next buffer; the filter state is kept.  Synchronous with respect to `stream`.
 *   set_decay        0 <= decay <= 1, per buffer, in force from the next process call.
 *   reset            every carried value zero; the weighting and the decay stay.
 *   state            the plan's own memory, for inspection: d_hist [tracks][16] = the last 11 samples oldest first,
 *                    peak_hold, true_peak_max, three zeros; d_filter [tracks][2][2] = (s1, s2) per section; d_ring
 *                    [tracks][window]; d_pos [tracks], the ring index of the next value.
 * Every field has the bits of this text on every call form, and a shard of tracks as its own plan gives those tracks'
 * bits.  process and process_batch are one launch each, allocate nothing and wait for nothing; the launch reads the
 * block once (16-byte loads where d_in is 16-byte aligned and bufsize a multiple of 4) and writes the rows and the
 * carried state only.  It works in chunks of 64 samples on 64 tracks: a bufsize far below 64 pays for a whole chunk,
 * and fewer than 64 tracks x 256 use a part of the device.  tracks >= 1, bufsize >= 1, 1 <= window <= 64;
 * arguments are checked before any device call.  One thread at a time per plan.                                   */
typedef struct gab_meter_plan gab_meter_plan;
#define GAB_METER_FIELDS 8
int gab_meter_create(gab_meter_plan** plan, int tracks, int bufsize, int window);
int gab_meter_destroy(gab_meter_plan* plan);
int gab_meter_set_weighting(gab_meter_plan* plan, const float* d_sections, gab_stream_t stream);
int gab_meter_set_decay(gab_meter_plan* plan, float decay, gab_stream_t stream);
int gab_meter_reset(gab_meter_plan* plan, gab_stream_t stream);
int gab_meter_process(gab_meter_plan* plan, const float* d_in, float* d_rows, gab_stream_t stream);
int gab_meter_process_batch(gab_meter_plan* plan, const float* d_in, float* d_rows, int n_buffers, gab_stream_t stream);
int gab_meter_state(gab_meter_plan* plan, float** d_hist, float** d_filter, float** d_ring, unsigned** d_pos);

/* ---- resample: every track's stream from one sample rate to another by a rational factor, with carried state
 * (additive; the reference changes no stream's rate) --------------------------------------------------------------
 * create divides up and down by their gcd; call the reduced pair L and M (shape reports them), K = taps, B = bufsize.
 * A polyphase FIR: L rows of K taps, made on the host in float64; the device does no division and calls no
 * transcendental function, and no summation order is left open.  Let w be a track's input stream, zero before the first
 * sample after a reset.
 *   position       Output sample m, counted from the reset, lies at input time m M / L:
 *                    i = floor(m M / L),  p = (m M) mod L                       (exact integers)
 *                  Buffer k since the reset carries inputs [k B, (k+1) B) and produces exactly the outputs m in
 *                  [lo(k), lo(k+1)), lo(k) = ceil(k B L / M): all outputs whose newest tap w[i] lies in that buffer.
 *                  n_out(k) = lo(k+1) - lo(k) is floor(B L / M) or ceil(B L / M) and may be 0;
 *                  out_capacity = ceil(B L / M).  The pattern repeats with period = M / gcd(B L, M) buffers; the plan
 *                  carries k mod period on the host in 64-bit arithmetic, so nothing overflows however long the stream
 *                  runs.  n_out and counts are host integers computed without touching the device.
 *   value          y[m] = fmaf(h_p[K-1], w[i-K+1], ... fmaf(h_p[1], w[i-1], h_p[0] * w[i]))
 *                  The product first, then ascending j, one rounding per step (the meter's true-peak chain).  Nothing
 *                  is re-associated; a NaN or an infinity travels as fmaf carries it.
 *   taps           For phase p and tap j:  d = j - K/2 + p/L,  c = 0.94 min(1, L/M),  u = d / (K/2),
 *                    h_p[j] = sinc(c d) (0.35875 + 0.48829 cos(pi u) + 0.14128 cos(2 pi u) + 0.01168 cos(3 pi u))
 *                  in float64 with libm's sin and cos, sinc(x) = sin(pi x) / (pi x), sinc(0) = 1; each phase row
 *                  divided by its sum (added in ascending j), rounded once to float32.  The latency is K/2 input
 *                  samples.  A row's sum is 1 but the sum of its magnitudes reaches about 2.1: an output can exceed the
 *                  input's peak.
 *   layout         d_in [tracks][B] float32, track-major, any 4-byte alignment, never written.  d_out
 *                  [tracks][out_capacity]; elements [n_out, out_capacity) of every row are written as 0.0f, so a whole
 *                  row is defined.  process_batch takes [n][tracks][B], writes [n][tracks][out_capacity] and counts[n]:
 *                  one launch with the bits of n process calls.  d_out may not overlap d_in.
 *   state          d_hist [tracks][K-1]: the last K-1 input samples, oldest first; zero after reset, which also puts k
 *                  back to 0.  Right when B < K-1 too: the history then spans several buffers and is shifted, not
 *                  replaced.  d_taps [L][K]: the table in force.  The third value is k mod period.
 *   set_taps       d_taps: device, [L][K].  Checked on the device first: the first value that is not finite is named as
 *                  (phase, tap) with GAB_ERR_INVALID_ARG and the plan keeps its table.  Accepted taps are in force from
 *                  the next buffer; history and position are kept.  Synchronous with respect to `stream`.
 * A shard of tracks as its own plan gives those tracks' bits.  process and process_batch are one launch each, allocate
 * nothing and wait for nothing.  The position is a launch argument: a captured process replays one position and is only
 * meaningful when period == 1; the captured call also advances the host's k, as a call that ran ("Captured calls",
 * above).  Arguments are checked before any device call: tracks >= 1, 1 <= bufsize <= 2^20, up
 * and down in 1..1024, taps even and in 4..256 (GAB_ERR_INVALID_ARG); L K <= 16384 floats, the table that fits 64 KiB
 * of LDS (else GAB_ERR_UNSUPPORTED).  The launch works on 64 tracks x 64 input samples at a time: fewer than 64 tracks x
 * 256 use a part of the device.  One thread at a time per plan.                                                     */
typedef struct gab_resample_plan gab_resample_plan;
int gab_resample_create(gab_resample_plan** plan, int tracks, int bufsize, int up, int down, int taps);
int gab_resample_destroy(gab_resample_plan* plan);
int gab_resample_shape(gab_resample_plan* plan, int* up, int* down, int* taps, int* out_capacity, int* period);
int gab_resample_set_taps(gab_resample_plan* plan, const float* d_taps, gab_stream_t stream);
int gab_resample_reset(gab_resample_plan* plan, gab_stream_t stream);
int gab_resample_process(gab_resample_plan* plan, const float* d_in, float* d_out, int* n_out, gab_stream_t stream);
int gab_resample_process_batch(gab_resample_plan* plan, const float* d_in, float* d_out, int n_buffers, int* counts,
                               gab_stream_t stream);
int gab_resample_state(gab_resample_plan* plan, float** d_hist, float** d_taps,
                       long long* buffers_since_reset_mod_period);

/* ---- dynamics: a compressor / limiter per track, with a carried smoothed gain, ramped parameters, linked detectors
 * and a side chain (additive; the reference has no dynamics) -----------------------------------------------------
 * The block of a channel strip between the equaliser and the fader.  Level quantities are in log2 units: one unit is
 * 6.0206 dB.  The contract calls no library transcendental: log2 and exp2 are the two polynomials below, fmaf by
 * fmaf, so the device can be restated bit for bit.
 *   parameters     device, [tracks][8] float32 (GAB_DYN_FIELDS):
 *                    0 thr     threshold, log2 of the linear level           finite, |thr| <= 128
 *                    1 slope   1 / ratio - 1                                 -1 <= slope <= 0 (0: off, -1: limiter)
 *                    2 knee    half width of the soft knee                   0 <= knee <= 64
 *                    3 kq      1 / (4 knee), 0 for a hard knee               finite, >= 0
 *                    4 att     one-pole coefficient while the reduction grows    0 <= att <= 1 - 2^-20
 *                    5 rel     the same while it shrinks                     0 <= rel <= 1 - 2^-20
 *                    6 makeup  linear gain after the reduction               finite
 *                    7 range   floor of the reduction                        finite, <= 0
 *                  The plan carries two tables, `current` and `target`; a new plan has {0, 0, 0, 0, 0, 0, 1, -256} in
 *                  both on every track and a smoothed gain of 0: pass-through bit for bit, for every finite or
 *                  infinite sample.
 *     set_params(ramp = 1)  target := the new table, current stays.  On the next processed buffer every one of the
 *                  eight fields of every track is p[s] = fmaf(target - current, r[s], current), r[s] = (s + 1) /
 *                  bufsize (the delay plan's table: float64 on the host, rounded once; target - current rounded
 *                  once); after that buffer current := target by a copy.  Two sets before a buffer: the ramp still
 *                  starts from current.
 *     set_params(ramp = 0)  current := target := the new table, at once.
 *     set_params_tracks     the same for rows [first_track, first_track + n_tracks), d_params [n_tracks][8]; the other
 *                  rows keep their current and target.
 *                  The values are checked on the device first, against the column `admitted` above.  A violation:
 *                  GAB_ERR_INVALID_ARG naming the first (track, field) in index order; the plan keeps what it had.
 *                  Both calls are synchronous with respect to `stream` and take effect with the next buffer.
 *                  Why att and rel stop at 1 - 2^-20: a ramped value is the rounding of current + fl(target -
 *                  current) r with 0 < r <= 1.  fl(target - current) is off by at most 2^-25, the fmaf's rounding of a
 *                  value below 1 by at most 2^-25 more, so a ramped coefficient can land above the larger of its two
 *                  ends, but by no more than 2^-24: it stays below 1 - 2^-20 + 2^-24 < 1, and the smoothing below
 *                  stays a convex combination.  (slope, knee, kq and range cannot leave their sign: for ends of one
 *                  sign fl(target - current) lies between -current and target by the monotonicity of rounding.)
 *     reset        the smoothed gain zero, current := target, a pending ramp dropped.
 *     params       the plan's own two tables, for inspection.
 *     state        the smoothed gain, [tracks] float32, for inspection.
 *     poly         host pointers to the pinned coefficients: c0..c6 and d0..d6 below.
 *   create         tracks >= 1, bufsize >= 1, link a power of two in 1..64 with tracks % link == 0: tracks [g link,
 *                  (g + 1) link) share one detector (stereo or surround linking); every track keeps its own parameters
 *                  and its own smoothed gain.  Arguments are checked before any device call.
 *   process        one buffer.  d_in and d_out track-major [t*B + s]; d_out == d_in is allowed (no other overlap).
 *                  d_key is null or a block of the same shape that does not overlap d_out (refused): the side chain,
 *                  which the detector reads instead of d_in (ducking; de-essing behind a gab_eq plan).  d_gr is null or
 *                  [tracks]: per track the smallest smoothed gain of the buffer, the gain-reduction meter.  Any
 *                  bufsize, any alignment, any track count: the same bits.
 *   process_batch  n_buffers buffers back to back in one launch: d_in, d_key, d_out [n][T*B], d_gr [n][T]; a pending
 *                  ramp runs through the first of them; same bits as n calls of process.  process and process_batch
 *                  allocate nothing and wait for nothing; the smoothed gain is device state.
 * The bits of one sample.  On a buffer without a pending ramp p = target, on one with a ramp the formula above.  Every
 * + - * below is rounded once, fmaf only where written; fmaxf and fminf ignore a NaN operand and order -0 below +0.
 * For sample n of track j in link group G, x the input, k the key block if one is given, else x, and s the track's
 * carried smoothed gain (<= 0):
 *     detector   a  = fmaxf over j' in G of |k[j'][n]|, from 0         (a NaN is ignored, as by the meter's peak)
 *                v  = fmaxf(a, 2^-96);  u = the bits of v
 *                e  = (int)(u >> 23) - 127;  m = the float of bits (u & 0x7fffff) | 0x3f800000;  t = m - 1   (exact)
 *                r  = c6;  r = fmaf(r, t, c5);  ...  r = fmaf(r, t, c0);   L = (float)e + t * r
 *                (-96 <= L <= 128 + 2^-18; an infinity reads e = 128, t = 0: L = 128)
 *     computer   over = L - thr;   ok = over + knee
 *                c  = over <= -knee ? 0 : over >= knee ? over : (ok * ok) * kq
 *                g  = fmaxf(slope * c, range)
 *     smoothing  al = (g < s) ? att : rel;   s = fmaf(al, s - g, g)
 *     gain       sc = fminf(fmaxf(s, -126), 0);  nf = floorf(sc);  f = sc - nf                               (exact)
 *                q  = d6;  q = fmaf(q, f, d5);  ...  q = fmaf(q, f, d0)
 *                y  = x * ((q * the float of bits ((int)nf + 127) << 23) * makeup)
 *     gr         fminf of s over the buffer's samples, from +infinity
 * The polynomials: log2(1 + t) = t r(t) and exp2(f) = q(f) on [0, 1), degree 6 each, interpolated at Chebyshev nodes in
 * float64 by tools/dyn_poly.py and rounded once per coefficient.  Worst error of the float32 chains: log2 1.3e-6
 * absolute (2^-19.6) over all 2^23 mantissas, held to 2^-18 (2.3e-5 dB); exp2 6.5e-8 relative (2^-23.9), held to 2^-22.
 *     c0..c6 = 0x1.715454p+0  -0x1.7139ccp-1  0x1.e8f4cep-2  -0x1.5a7f8ep-2  0x1.b627dcp-3  -0x1.839766p-4  0x1.47f3eap-6
 *     d0..d6 = 1  0x1.62e43p-1  0x1.ebfc3ep-3  0x1.c69f98p-5  0x1.3c487cp-7  0x1.4cb7bp-10  0x1.b49554p-13
 * L is finite for every input, so g and s stay finite whatever the samples are: a NaN or an infinity in x reaches y
 * (x times a finite gain) and nothing else; a NaN in the key is ignored and an infinity reads as L = 128.  (The meter's
 * filter state, by contrast, is poisoned by one such sample.)  Nothing else has rounding freedom: every launch form gives
 * the same bits, and a shard of tracks that is a multiple of link, run as its own plan, gives those tracks' bits.
 * Look-ahead is not part of the plan: a gab_delay plan in front of d_in, with the undelayed signal as d_key, gives it,
 * but that only moves the attack's overshoot; for a ceiling that holds on every sample there is the gab_lim plan.
 * The launch works on 64 tracks x 64 samples per wave: fewer than 64 tracks x 1024 use a part of the device.  One thread
 * at a time per plan.                                                                                               */
typedef struct gab_dyn_plan gab_dyn_plan;
#define GAB_DYN_FIELDS 8
int gab_dyn_create(gab_dyn_plan** plan, int tracks, int bufsize, int link);
int gab_dyn_destroy(gab_dyn_plan* plan);
int gab_dyn_set_params(gab_dyn_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_dyn_set_params_tracks(gab_dyn_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream);
int gab_dyn_reset(gab_dyn_plan* plan, gab_stream_t stream);
int gab_dyn_process(gab_dyn_plan* plan, const float* d_in, const float* d_key, float* d_out, float* d_gr,
                    gab_stream_t stream);
int gab_dyn_process_batch(gab_dyn_plan* plan, const float* d_in, const float* d_key, float* d_out, float* d_gr,
                          int n_buffers, gab_stream_t stream);
int gab_dyn_params(gab_dyn_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_dyn_state(gab_dyn_plan* plan, float** d_smooth, size_t* n_floats);
int gab_dyn_poly(const float** log2_coeffs, int* n_log2, const float** exp2_coeffs, int* n_exp2);

/* ---- reverb: a feedback delay network per track, with carried lines, a damping low-pass in the loop and ramped
 * gains (additive; the reference has no reverb) ----------------------------------------------------------------
 * An algorithmic reverb beside the sampled room of gab_conv (scheme FDL) and the single line of gab_delay: N = `lines`
 * delay lines per track (4, 8 or 16), fed back through the unnormalised Walsh-Hadamard matrix H (orthogonal up to
 * sqrt(N)), a one-pole low-pass per line in the loop, O = `outs` outputs per track (1 or 2).
 *   delays         device, [tracks][N] int32, in samples: GAB_REVERB_MIN_DELAY <= m[i] <= max_delay.  Not ramped: a new
 *                  set acts from the next processed buffer, and the lines keep their contents (a line's history is
 *                  simply read further back or less far).  A new plan has max_delay on every line.
 *   parameters     device, [tracks][P] float32, P = gab_reverb_row_floats(N, O) = N (3 + O) + 1, one row per track:
 *                    g[N]      the line's loop gain                          finite, |g| <= gab_reverb_gmax(N)
 *                    damp[N]   the loop low-pass's coefficient               0 <= damp <= 1 - 2^-20
 *                    b[N]      input gain into the line                      finite
 *                    c[O][N]   output o's gain from line i, at (3 + o) N + i finite
 *                    dry       the input's gain into every output            finite
 *                  The plan carries two tables, `current` and `target`; a new plan has dry = 1 and zeros elsewhere in
 *                  both on every track, zero lines and a zero low-pass state: pass-through for every finite sample,
 *                  bit for bit (zeros are added to dry * x; only a -0 input comes out as +0).
 *     set_params(ramp = 1)  target := the new table, current stays.  On the next processed buffer every field of every
 *                  track is p[s] = fmaf(target - current, r[s], current), r[s] = (s + 1) / bufsize (the delay plan's
 *                  table: float64 on the host, rounded once; target - current rounded once); after that buffer
 *                  current := target by a copy.  Two sets before a buffer: the ramp still starts from current.
 *     set_params(ramp = 0)  current := target := the new table, at once.
 *     set_params_tracks     the same for rows [first_track, first_track + n_tracks), d_params [n_tracks][P]; the other
 *                  rows keep their current and target.
 *     set_delays, set_delays_tracks   the delays of every track, or of rows [first_track, first_track + n_tracks),
 *                  d_delays [n_tracks][N].
 *                  The values are checked on the device first, against the column `admitted` above.  A violation:
 *                  GAB_ERR_INVALID_ARG naming the first (track, field) or (track, line) in index order; the plan keeps
 *                  what it had, a pending ramp included.  All four calls are synchronous with respect to `stream` and
 *                  take effect with the next buffer.
 *                  Why these limits.  ||H|| = sqrt(N) and the low-pass is a convex combination (its gain never exceeds
 *                  1), so the loop's gain is at most sqrt(N) max|g|.  gmax(N) is the float32 nearest
 *                  (1 - 2^-20) / sqrt(N), formed in float64:
 *                      GAB_REVERB_GMAX_4  = 0x1.ffffep-2f    GAB_REVERB_GMAX_8 = 0x1.6a09dp-2f
 *                      GAB_REVERB_GMAX_16 = 0x1.ffffep-3f
 *                  and sqrt(N) gmax(N) < 1 - 2^-21 for all three.  A ramped value is the rounding of current +
 *                  fl(target - current) r with 0 < r <= 1: it can land beyond the larger of its two ends by no more than
 *                  2^-24 (dynamics plan, same argument), which carries neither sqrt(N) |g| nor damp to 1.
 *     reset        lines, write positions and low-pass states zero, current := target, a pending ramp dropped; the
 *                  delays stay.
 *     params       the plan's own two tables, for inspection.
 *     state        for inspection: the lines ([tracks][N][capacity] float32, capacity a power of two >= max_delay +
 *                  64), the capacity, the write positions ([tracks] unsigned: the ring index of the next sample, the
 *                  same for every line of a track, a word per track that the kernel updates with ordinary vector
 *                  stores), the low-pass states q ([tracks][N] float32) and the delays ([tracks][N] int32).
 *   process        one buffer.  d_in track-major [t*B + s]; d_out [(t*O + o)*B + s]: a track's outputs are neighbouring
 *                  rows, so a gab_mix plan of tracks*O tracks takes the block as it lies.  d_out == d_in is allowed when
 *                  outs == 1 and refused when outs == 2 (no other overlap either way).  Any bufsize, any alignment, any
 *                  track count: the same bits.
 *   process_batch  n_buffers buffers back to back (d_in [n][T*B], d_out [n][T*O*B]) in one launch; a pending ramp runs
 *                  through the first of them; same bits as n calls of process.  process and process_batch allocate
 *                  nothing and wait for nothing; lines, positions and q are device state.
 * The bits of one sample.  On a buffer without a pending ramp p = target, on one with a ramp the formula above, for
 * every field.  Every + - * below is rounded once, fmaf only where written, nothing is re-associated, no library
 * transcendental is called.  For absolute sample n of a track, x the input, line_i the track's i-th line (zero before
 * the first sample and after a reset), q[i] its carried low-pass state:
 *     1  s[i] = line_i[n - m[i]]
 *     2  v[i] = g[i] * s[i]
 *     3  q[i] = fmaf(damp[i], q[i] - v[i], v[i])            (q - v rounded once; DC gain 1, Nyquist (1 - d) / (1 + d))
 *     4  u = H q: log2 N butterfly stages h = 1, 2, 4, ..., N / 2 in that order.  Stage h replaces, for every k with
 *        (k & h) == 0, the pair (a, b) = (u[k], u[k + h]) by (a + b, a - b); u starts as q.
 *     5  line_i[n] = fmaf(b[i], x[n], u[i])
 *     6  for each output o: acc = dry * x[n]; acc = fmaf(c[o][i], q[i], acc) for i = 0 .. N-1 in that order;
 *        y[o][n] = acc                                         (the q of step 3, not u)
 * Samples that are not finite: a NaN or an infinity in a track's input enters that track's lines through step 5,
 * comes round through steps 1 to 4 for ever and stays until reset; no other track is touched.  (The dynamics plan, by
 * contrast, carries nothing that such a sample can reach.)
 * Nothing else has rounding freedom: every launch form gives the same bits, and a shard of tracks as its own plan gives
 * those tracks' bits.  The launch gives one wave 64 / N tracks: fewer than 64 / N x 1024 tracks use a part of the
 * device.  tracks >= 1, bufsize >= 1, GAB_REVERB_MIN_DELAY <= max_delay <= 2^20; arguments are checked before any
 * device call.  One thread at a time per plan.                                                                      */
typedef struct gab_reverb_plan gab_reverb_plan;
#define GAB_REVERB_MIN_DELAY 32
#define GAB_REVERB_GMAX_4  0x1.ffffep-2f
#define GAB_REVERB_GMAX_8  0x1.6a09dp-2f
#define GAB_REVERB_GMAX_16 0x1.ffffep-3f
int gab_reverb_create(gab_reverb_plan** plan, int tracks, int bufsize, int lines, int outs, int max_delay);
int gab_reverb_destroy(gab_reverb_plan* plan);
int gab_reverb_set_params(gab_reverb_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_reverb_set_params_tracks(gab_reverb_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                                 gab_stream_t stream);
int gab_reverb_set_delays(gab_reverb_plan* plan, const int* d_delays, gab_stream_t stream);
int gab_reverb_set_delays_tracks(gab_reverb_plan* plan, const int* d_delays, int first_track, int n_tracks,
                                 gab_stream_t stream);
int gab_reverb_reset(gab_reverb_plan* plan, gab_stream_t stream);
int gab_reverb_process(gab_reverb_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_reverb_process_batch(gab_reverb_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_reverb_params(gab_reverb_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_reverb_state(gab_reverb_plan* plan, float** d_lines, size_t* capacity, unsigned** d_pos, float** d_q,
                     int** d_delays);
/* N (3 + O) + 1, or 0 for a (lines, outs) the plan does not take; gmax(N), or 0.  Host arithmetic. */
int gab_reverb_row_floats(int lines, int outs);
float gab_reverb_gmax(int lines);

/* ---- gate: a noise gate / ducker per track, a two-state machine with hysteresis and a hold counter, a linear gain
 * that glides between two levels, ramped parameters, linked detectors and a side chain (additive; the reference has no
 * gate) ------------------------------------------------------------------------------------------------------------
 * The block of a channel strip in front of the compressor.  Everything is linear: levels are compared as they are, the
 * gain is a one-pole glide, and no transcendental of any kind enters, so the device can be restated bit for bit.
 *   parameters     device, [tracks][7] float32 (GAB_GATE_FIELDS):
 *                    0 open      linear level above which the gate opens         finite, 0 <= open <= 2^64
 *                    1 close     linear level below which the hold runs down     0 <= close <= open of the same row
 *                    2 att       one-pole coefficient while open                 0 <= att <= 1 - 2^-20
 *                    3 rel       one-pole coefficient while closed               0 <= rel <= 1 - 2^-20
 *                    4 g_open    linear gain the track glides to while open      0 <= g_open <= 256
 *                    5 g_closed  linear gain while closed                        0 <= g_closed <= 256
 *                    6 hold      samples the gate stays open below close         an integer value, 0 <= hold <= 2^24
 *                  A noise gate is g_open = 1, g_closed = the range (0: shut); a ducker is g_open = the depth,
 *                  g_closed = 1, with the voice as the key: there is no mode switch.  The plan carries two tables,
 *                  `current` and `target`; a new plan has {0, 0, 0, 0, 1, 1, 0} in both on every track, a gain of 1
 *                  and a count of -1: pass-through bit for bit, for every sample, finite or not.
 *     set_params(ramp = 1)  target := the new table, current stays.  On the next processed buffer fields 0 to 5 of every
 *                  track are p[s] = fmaf(target - current, r[s], current), r[s] = (s + 1) / bufsize (the delay plan's
 *                  table: float64 on the host, rounded once; target - current rounded once); after that buffer
 *                  current := target by a copy.  Field 6 is not ramped: that buffer takes target's hold from its first
 *                  sample, as every buffer does.  Two sets before a buffer: the ramp still starts from current.
 *     set_params(ramp = 0)  current := target := the new table, at once.
 *     set_params_tracks     the same for rows [first_track, first_track + n_tracks), d_params [n_tracks][7]; the other
 *                  rows keep their current and target.
 *                  The values are checked on the device first, against the column `admitted` above (close against
 *                  the open of its own row in d_params).  A violation: GAB_ERR_INVALID_ARG naming the first (track,
 *                  field) in index order; the plan keeps what it had, a pending ramp included.  Both calls are
 *                  synchronous with respect to `stream` and take effect with the next buffer.
 *                  Why att and rel stop at 1 - 2^-20 (the dynamics plan's argument): a ramped value is the rounding of
 *                  current + fl(target - current) r with 0 < r <= 1.  fl(target - current) is off by at most 2^-25,
 *                  the fmaf's rounding of a value below 1 by at most 2^-25 more, so a ramped coefficient can land
 *                  above the larger of its two ends, but by no more than 2^-24: it stays below 1 - 2^-20 + 2^-24 < 1,
 *                  and the glide below stays a convex combination of the gain and its goal.  (open, close, g_open and
 *                  g_closed cannot become negative: for ends that are both >= 0, fl(target - current) lies between
 *                  -current and target by the monotonicity of rounding.)  In the same way a ramped close may land a
 *                  rounding above the ramped open of its sample.  That is harmless: the order of the two tests below
 *                  decides, a > open first.
 *     reset        the count -1 (closed) and the gain target's g_closed on every track, so that a gate starts shut
 *                  and does not leak one release tail; current := target, a pending ramp dropped.
 *     params       the plan's own two tables, for inspection.
 *     state        the gain ([tracks] float32) and the count ([tracks] int32), for inspection.
 *   create         tracks >= 1, bufsize >= 1, link a power of two in 1..64 with tracks % link == 0: tracks [g link,
 *                  (g + 1) link) share one detector and nothing else; every track keeps its own row, its own gain and
 *                  its own count.  Arguments are checked before any device call.
 *   process        one buffer.  d_in and d_out track-major [t*B + s]; d_out == d_in is allowed (no other overlap).
 *                  d_key is null or a block of the same shape that does not overlap d_out (refused): the side chain,
 *                  which the detector reads instead of d_in.  d_act is null or [tracks] int32: per track the number of
 *                  samples of the buffer on which the gate was open (the gate's LED).  Any bufsize, any alignment, any
 *                  track count: the same bits.
 *   process_batch  n_buffers buffers back to back in one launch: d_in, d_key, d_out [n][T*B], d_act [n][T]; a pending
 *                  ramp runs through the first of them; same bits as n calls of process.  process and process_batch
 *                  allocate nothing and wait for nothing; the gain and the count are device state.
 * The bits of one sample.  On a buffer without a pending ramp p = target, on one with a ramp the formula above for
 * fields 0 to 5; H = (int)hold of target on either.  Every - and * below is rounded once, fmaf only where written;
 * fmaxf ignores a NaN operand.  For sample n of track j in link group G, x the input, k the key block if one is given,
 * else x, and the track's carried g (float32) and c (int32):
 *     detector   a  = fmaxf over j' in G of |k[j'][n]|, from 0         (a NaN is ignored, as by the meter's peak)
 *     state      c  = a > open ? H : a >= close ? (c >= 0 ? H : -1) : max(c - 1, -1)
 *                o  = c >= 0
 *     glide      tg = o ? g_open : g_closed;   al = o ? att : rel;   g = fmaf(al, g - tg, tg)
 *     output     y  = x * g
 *     act        the number of samples of the buffer with o
 * So the gate opens on the first sample above open, stays open for exactly `hold` samples below close (the count runs
 * H - 1, ..., 0, -1), and a level between close and open keeps whatever state there is and re-arms the hold of an open
 * gate.  g is a convex combination of its old value and g_open or g_closed: it stays within [0, 256] once it is there
 * and decays through the subnormals to 0 under g_closed = 0 (the device keeps subnormals).  g and c are finite whatever
 * the samples are: a NaN or an infinity in x reaches y (x times a finite gain) and nothing else; a NaN in the key is
 * ignored and an infinity in the key opens the gate.  Nothing has rounding freedom: every launch form gives the same
 * bits, and a shard of tracks that is a multiple of link, run as its own plan, gives those tracks' bits.
 * Out of scope: downward expansion with a ratio (the dynamics plan's log2 domain), look-ahead (a gab_delay plan in
 * front of d_in, with the undelayed signal as d_key, gives it; a look-ahead ceiling is the gab_lim plan), a filtered
 * key (a gab_eq plan on the key gives it).
 * The launch works on 16 tracks x 64 samples per wave, four waves to a workgroup: fewer than 16 x 1024 tracks use a
 * part of the device.  One thread at a time per plan.                                                               */
typedef struct gab_gate_plan gab_gate_plan;
#define GAB_GATE_FIELDS 7
int gab_gate_create(gab_gate_plan** plan, int tracks, int bufsize, int link);
int gab_gate_destroy(gab_gate_plan* plan);
int gab_gate_set_params(gab_gate_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_gate_set_params_tracks(gab_gate_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                               gab_stream_t stream);
int gab_gate_reset(gab_gate_plan* plan, gab_stream_t stream);
int gab_gate_process(gab_gate_plan* plan, const float* d_in, const float* d_key, float* d_out, int* d_act,
                     gab_stream_t stream);
int gab_gate_process_batch(gab_gate_plan* plan, const float* d_in, const float* d_key, float* d_out, int* d_act,
                           int n_buffers, gab_stream_t stream);
int gab_gate_params(gab_gate_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_gate_state(gab_gate_plan* plan, float** d_gain, int** d_count, size_t* n_tracks);

/* ---- crossover: a Linkwitz-Riley (fourth-order) split of every track into K = 2..4 bands whose sum is the input
 * through an all-pass, made of trapezoidal state-variable sections with fixed arithmetic (additive; the reference has
 * no crossover) -----------------------------------------------------------------------------------------------------
 * The block in front of a multiband compressor, a de-esser or a bass manager: the band block it writes is a K T-track
 * block as gab_dyn_process, gab_gate_process and gab_mix_process take it.  S = K - 1 splits per track.
 *   rows           device, [tracks][S][3] float32 (GAB_XOVER_FIELDS): {a1, a2, a3} per (track, split), the splits of a
 *                  track in ascending frequency.  Made on the host in float64 and rounded once:
 *                      g = tan(pi f / fs),  k = (double)K32,  K32 = (float)sqrt(2.0) = GAB_XOVER_K32
 *                      a1 = 1 / (1 + g (g + k)),  a2 = g a1,  a3 = g a2
 *     set_splits   the whole table; set_splits_tracks: rows [first_track, first_track + n_tracks), d_rows
 *                  [n_tracks][S][3], the other rows kept.  The values are checked on the device first.  Refused are
 *                      a value that is not finite;
 *                      field 0 unless 0 < a1 <= 1;    field 1 unless 0 <= a2 < 1;    field 2 unless 0 <= a3 < 1;
 *                      field 2, read with the two before it, unless |(fmaf(K32, a2, a1) + a3) - 1| <= 2^-20
 *                      and unless |fmaf(a2, a2, -(a1 * a3))| <= 2^-18 * (a2 * a2)      (every operation rounded once).
 *                  A row that passes is the row of some g >= 0 to within those margins (host-made rows reach 2^-23 and
 *                  2^-21.9), and the section below is stable for every such g.  A violation: GAB_ERR_INVALID_ARG naming
 *                  the first (track, field) in index order, field = 3 split + {0, 1, 2}; the plan keeps what it had.
 *                  Both calls are synchronous with respect to `stream`.  Coefficients are not ramped: as with
 *                  gab_eq_set_coeffs a set takes effect with the next buffer and keeps the state.  The states are the
 *                  integrators' own (twice the charge of the two capacitors of the analogue section), not a filter's
 *                  delay line: they mean the same under any row, so a moved split does not rescale them and makes no
 *                  click beyond the change of the filter itself.
 *     reset        every state to +0; the rows are kept.
 *     splits       the plan's own table, for inspection.     state: the plan's state array, [tracks][sections][2].
 *     sections     3 S + S (S - 1) / 2 = 3, 7, 12 for K = 2, 3, 4; 0 for any other K.  Host arithmetic, no plan.
 *   create         tracks >= 1, bufsize >= 1, bands 2..4.  Arguments are checked before any device call.  A new plan
 *                  has no rows: process before the first accepted set is refused, with a text that says so.  (Rows that
 *                  a first set_splits_tracks leaves out are {1, 0, 0}, g = 0: band K - 1 is the input.)
 *   process        one buffer.  d_in track-major [t*B + s]; d_out band-major [K][T][B], band 0 the lowest.  d_out may
 *                  not overlap d_in (refused).  Any bufsize, any alignment, any track count: the same bits; 16-byte
 *                  aligned pointers with bufsize % 4 == 0 take a wider load.
 *   process_batch  n_buffers buffers in one launch: d_in [n][T*B], d_out [n][K][T*B], the state running through; the
 *                  same bits as n calls of process.  Neither call allocates or waits.
 * One section.  State (ic1, ic2), input v0, its split's row; every written operation is rounded once:
 *     v3 = v0 - ic2
 *     v1 = fmaf(a2, v3, a1 * ic1)
 *     v2 = fmaf(a3, v3, fmaf(a2, ic1, ic2))
 *     ic1 = fmaf(2, v1, -ic1)
 *     ic2 = fmaf(2, v2, -ic2)
 *     low = v2      band = v1      high = fmaf(-K32, v1, v0) - v2
 * The topology, per track and sample, from the bottom up.  r_0 = x.  For split j = 0..S-1, on split j's row:
 *     (l, ., h) = A_j(r_j)        low_j = B_j(l).low        r_{j+1} = C_j(h).high
 * then for m = j+1..S-1 in turn, on split m's row, the all-pass that the upper bands see and band j would not:
 *     low_j = fmaf(-K2, D_{j,m}(low_j).band, low_j),      K2 = 2 * K32 (exact in float32)
 * Band j is low_j, band K - 1 is r_S.  In exact arithmetic the bands sum to x through the product of the splits'
 * second-order all-passes.  The order of the sections in the state array: split after split, and within split j
 *     A_j, B_j, C_j, D_{j,j+1}, ..., D_{j,S-1}
 * that is  K = 2: A0 B0 C0;  K = 3: A0 B0 C0 D01 A1 B1 C1;  K = 4: A0 B0 C0 D01 D02 A1 B1 C1 D12 A2 B2 C2.
 * A NaN or an infinity in x enters that track's states and stays in that track's bands until reset; it reaches no
 * other track.  Subnormals are kept: a tail runs down through them, and comes to rest not at zero but within a few
 * units of 2^-149 (round-to-nearest: a section stops moving once a2 v3 and a3 v3 round to nothing against its states,
 * about 1 / (2 a3) units); reset gives +0.  Every section is a deterministic recurrence, so nothing has rounding
 * freedom: every launch form gives the same bits, and a shard of tracks run as its own plan gives those tracks' bits.  Out of scope: ramped splits, other slopes, linear-phase splits (a gab_conv plan per band).
 * One thread at a time per plan.                                                                                     */
typedef struct gab_xover_plan gab_xover_plan;
#define GAB_XOVER_FIELDS 3
#define GAB_XOVER_K32 0x1.6a09e6p+0f
int gab_xover_create(gab_xover_plan** plan, int tracks, int bufsize, int bands);
int gab_xover_destroy(gab_xover_plan* plan);
int gab_xover_set_splits(gab_xover_plan* plan, const float* d_rows, gab_stream_t stream);
int gab_xover_set_splits_tracks(gab_xover_plan* plan, const float* d_rows, int first_track, int n_tracks,
                                gab_stream_t stream);
int gab_xover_reset(gab_xover_plan* plan, gab_stream_t stream);
int gab_xover_process(gab_xover_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_xover_process_batch(gab_xover_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_xover_splits(gab_xover_plan* plan, float** d_rows, size_t* n_floats);
int gab_xover_state(gab_xover_plan* plan, float** d_state, size_t* n_floats);
int gab_xover_sections(int bands);

/* ---- limiter: a brickwall look-ahead limiter per track, with a window of W = 2^k samples, ramped parameters, linked
 * detectors and three carried histories (additive; the reference has no limiter) ------------------------------------
 * The block at the very end of a bus, behind gab_mix: the one dynamics processor that GUARANTEES |y| <= ceil on every
 * sample.  (gab_dyn with slope = -1 is a limiter only in name: its gain is smoothed by an attack and goes through a
 * polynomial.)  No transcendental, no polynomial: a division, a window minimum, a release recursion and a box mean.
 *   parameters     device, [tracks][3] float32 (GAB_LIM_FIELDS):
 *                    0 drive   linear gain in front of the limiter           0 <= drive <= 2^32   (so finite)
 *                    1 ceil    the ceiling, linear                           2^-32 <= ceil <= 2^32
 *                    2 rel     release coefficient per sample                0 <= rel <= 1
 *                  The plan carries two tables, `current` and `target`; a new plan has {1, 2^32, 0} in both on every
 *                  track and the histories below: a pure delay of D = W - 1 samples, bit for bit, for every sample
 *                  whose magnitude is at most 2^32 or that is not finite.
 *     set_params(ramp = 1)  target := the new table, current stays.  On the next processed buffer every one of the
 *                  three fields of every track is p[s] = fmaf(target - current, r[s], current), r[s] = (s + 1) /
 *                  bufsize (the delay plan's table: float64 on the host, rounded once; target - current rounded
 *                  once); after that buffer current := target by a copy.  Two sets before a buffer: the ramp still
 *                  starts from current.
 *     set_params(ramp = 0)  current := target := the new table, at once.
 *     set_params_tracks     the same for rows [first_track, first_track + n_tracks), d_params [n_tracks][3]; the other
 *                  rows keep their current and target.
 *                  The values are checked on the device first, against the column `admitted` above.  A violation:
 *                  GAB_ERR_INVALID_ARG naming the first (track, field) in index order; the plan keeps what it had.
 *                  Both calls are synchronous with respect to `stream` and take effect with the next buffer.
 *                  What a ramp can do to the ends: a ramped value is the rounding of current + fl(target - current) r
 *                  with 0 < r <= 1.  fl(target - current) lies between -current and target by the monotonicity of
 *                  rounding, so a ramped drive or ceil is never negative (a ceil may reach 0 on the last sample of a
 *                  ramp from 2^32 down to 2^-32: the need is then 0 and the guarantee below holds with y = 0).  A
 *                  ramped rel can land above the larger of its two ends, but by no more than 2^-24 (fl(target -
 *                  current) is off by at most 2^-25, the fmaf's rounding of a value near 1 by at most 2^-25 more): up
 *                  to 1 + 2^-24.  That is harmless: the release step's fminf holds e at or below m <= 1 whatever
 *                  fmaf(rel, 1 - e, e) is.
 *     reset        the histories as in a new plan, current := target, a pending ramp dropped.
 *     params       the plan's own two tables, for inspection.
 *     state        the three histories, each [tracks][W - 1] float32, oldest first, as they stand after every call:
 *                  d_x the last W - 1 values of xd, d_t of t, d_e of e (below); *per_track = W - 1.  A new or reset plan
 *                  has xd = 0, t = 1, e = 1.
 *     latency      D = W - 1 samples, the same for every track: a desk compensates it once.
 *   create         tracks >= 1, bufsize >= 1, lookahead_log2 = k in 2..8: W = 2^k = 4..256 samples (5.3 ms at 48 kHz);
 *                  link a power of two in 1..64 with tracks % link == 0: tracks [g link, (g + 1) link) share one
 *                  detector; every track keeps its own parameters and histories.  Arguments are checked before any
 *                  device call.
 *   process        one buffer.  d_in and d_out track-major [t*B + s]; d_out == d_in is allowed, any other overlap is
 *                  refused.  d_gr is null or [tracks]: per track the smallest gain g of the buffer.  Any bufsize >= 1
 *                  (those shorter than W - 1 included), any alignment, any track count: the same bits.
 *   process_batch  n_buffers buffers back to back: d_in, d_out [n][T*B], d_gr [n][T]; a pending ramp runs through the
 *                  first of them; same bits as n calls of process.  process and process_batch allocate nothing and
 *                  wait for nothing, so they can be captured; the histories are device state.  One launch per call or
 *                  batch for link <= 8; for link = 16, 32 and 64 two launches per buffer (the group's detector first).
 * The bits of one sample.  On a buffer without a pending ramp p = target, on one with a ramp the formula above.  Every
 * + - * / below is rounded once, fmaf only where written; fminf and fmaxf ignore a NaN operand; the division is IEEE
 * (round to nearest even, subnormals kept).  For sample n of track j in link group G, x the input, p the parameters in
 * force at n:
 *     drive      xd = p.drive * x[n]
 *     detector   d  = fmaxf over j' in G of (|xd[j']| if its bits are below 0x7f800000, else 0), from 0
 *     need       t  = 1                          if d <= p_j.ceil
 *                t  = p_j.ceil / d               otherwise;  if t * d > p_j.ceil:  t = the float one unit below t (bits - 1)
 *     window     m  = fminf(t[n], t[n-1], ..., t[n-(W-1)])
 *     release    e  = fminf(m, fmaf(p_j.rel, 1 - e[n-1], e[n-1]))
 *     box        S1[n] = e[n];  S2h[n] = Sh[n] + Sh[n-h]  for h = 1, 2, ..., W/2;   s = SW[n] * 2^-k
 *     gain       g  = fminf(s, t[n-(W-1)])
 *     out        y[n] = g * xd[n-(W-1)]
 *     gr         fminf of g over the buffer's samples, from +infinity
 * (fminf is exact in any order; the box is the doubling tree as written, W - 1 additions in k levels.)
 * The guarantee.  |y[n]| <= the ceil in force when sample n - (W-1) came in, exactly, for every input whose xd at
 * n - (W-1) is finite.  In three steps, with n' = n - (W-1), d', c' the detector and the ceiling at n':
 *   1. Every e[k], k in [n', n], is at most m[k] (the release step's fminf), and m[k] <= t[n'] because t[n'] is inside
 *      the window of every such k.  So all W terms of the box are <= t[n'], and in exact arithmetic so is their mean.
 *   2. The sum's roundings could lift s above t[n'] all the same; the final fminf(s, t[n']) takes the sum's rounding out
 *      of the argument altogether: g <= t[n'], and g >= 0 because every t and so every e is.
 *   3. t[n'] * d' <= c' in float32: if d' <= c', t = 1 and 1 * d' = d'; otherwise that is what the correction
 *      established.  |xd_j[n']| <= d' (the track is in its own group), and rounding is monotone, so
 *      |y| = fl(g |xd_j|) <= fl(t[n'] d') <= c'.
 *   Why one unit is enough: q = fl(c / d) <= (c / d)(1 + 2^-24), so q d <= c (1 + 2^-24) before rounding, and one unit
 *   takes at least 2^-24 of a normal q away: (q - ulp) d <= c, which rounds to at most c.  A subnormal q loses a larger
 *   share; a q of +0 is never corrected, because 0 * d > c is false.
 * Linearity below the ceiling.  A stretch in which no link group's d exceeds its ceilings has t = 1; once the histories
 * hold t = e = 1 (a new plan, or W - 1 such samples with rel = 1, or the recovery of any rel > 0 run to its end), m = e =
 * 1, the box sums W ones exactly, g = 1 and y is drive * x delayed by D, bit for bit, with gr = 1.
 * Samples that are not finite.  An xd that is a NaN or an infinity is not seen by the detector (it reads as 0 there, for
 * its own track and for its link group), so t, m, e, s and g are finite whatever the samples are.  It reaches y once, D
 * samples later, times that sample's finite gain (infinity times a gain of 0 is a NaN).  Every other output sample and
 * every state word but its own slot of the xd history is what it would be with a 0 in its place; it stays in its track,
 * also inside a link group.
 * No rounding freedom.  Every launch form gives the same bits; a shard of tracks that is a multiple of link, run as its
 * own plan, gives those tracks' bits; any bufsize >= 1 and any cut of a stream into buffers gives the same bits; any
 * alignment gives the same bits (16-byte aligned pointers with bufsize % 4 == 0 take a wider load).
 * Out of scope: oversampled (true-peak) detection, a side-chain key, a look-ahead per track.
 * The launch works on 8 tracks x 64 samples per wave, a wave to a workgroup.  One thread at a time per plan.         */
typedef struct gab_lim_plan gab_lim_plan;
#define GAB_LIM_FIELDS 3
int gab_lim_create(gab_lim_plan** plan, int tracks, int bufsize, int lookahead_log2, int link);
int gab_lim_destroy(gab_lim_plan* plan);
int gab_lim_set_params(gab_lim_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_lim_set_params_tracks(gab_lim_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream);
int gab_lim_reset(gab_lim_plan* plan, gab_stream_t stream);
int gab_lim_process(gab_lim_plan* plan, const float* d_in, float* d_out, float* d_gr, gab_stream_t stream);
int gab_lim_process_batch(gab_lim_plan* plan, const float* d_in, float* d_out, float* d_gr, int n_buffers,
                          gab_stream_t stream);
int gab_lim_params(gab_lim_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_lim_state(gab_lim_plan* plan, float** d_x, float** d_t, float** d_e, size_t* per_track);
int gab_lim_latency(gab_lim_plan* plan, int* samples);

/* ---- spectrum: a short-time Fourier analyser per track, with carried history (additive; the reference's FFT benchmark
 * is one stateless transform of 1024 samples, gab_fft_r2c_1024 above) ------------------------------------------------
 * The running spectrum a channel strip draws beside its equaliser and its meter, and the analysis half of any later
 * spectral processor.  N = 1024 is the transform, B = bufsize, H the hop (fixed at create, 32 <= H <= 1024, any
 * integer), T = tracks.
 *   stream, frames  s[a] is a track's stream, a the absolute sample index since create or reset, s[a] = 0 for a < 0.
 *                   Frame j >= 1 covers samples jH - N .. jH - 1:
 *                     f_j[n] = w[n] * s[jH - N + n]                       one float32 product, rounded once
 *                   A call that takes samples [p, p + n B) emits exactly the frames with p < jH <= p + n B, in ascending
 *                   j: floor((p + n B) / H) - floor(p / H) of them, possibly none.  The count is host integer arithmetic
 *                   on the carried p mod H and is returned in *n_frames without touching the device.  gab_spec_frames
 *                   gives the largest count any call of n_buffers buffers can return, ceil(n_buffers B / H): what
 *                   d_rows must hold.  Rows past *n_frames are not written; a call that emits no frame writes none.
 *                   The plan carries the last 1023 samples of every track on the device.
 *   window          w: 1024 floats, the same for every track.  A new plan holds the periodic Hann window
 *                   0.5 - 0.5 cos(2 pi n / N), made in float64 on the host and rounded once.  S is the float64 sum of
 *                   the float32 values, added in ascending n.  set_window takes d_window (device, [1024]); checked on
 *                   the device first: the first value that is not finite is named with GAB_ERR_INVALID_ARG; then on the
 *                   host: a table with S == 0 is refused.  A refused set leaves the plan as it was.  An accepted window
 *                   is in force from the next call; the history is kept.  Synchronous with respect to `stream`.
 *   modes           fixed at create.
 *                   GAB_SPEC_COMPLEX (bands = 0): d_rows [frames][T][513][2], the unnormalised spectrum of f_j in the
 *                     layout of gab_fft_r2c_1024 (bins 0..512, re then im).
 *                   GAB_SPEC_POWER, bands = 0: d_rows [frames][T][513],
 *                     P[k] = (re * re + im * im) * inv_k        every operation rounded once, no fused multiply-add
 *                     inv_k = (float)(4 / S^2) for 0 < k < 512, (float)(1 / S^2) for k = 0 and k = 512    (in float64)
 *                     with (re, im) the bits of the complex mode.  So a sine of amplitude A on a bin reads A^2 and a
 *                     constant c reads c^2.  Linear; decibels are the caller's business.  (A window whose S^2 leaves
 *                     float32's range gives an inv_k of 0 or infinity.)
 *                   GAB_SPEC_POWER, 1 <= bands <= 64: d_rows [frames][T][bands]; band b is the float32 sum of P[k] for
 *                     e_b <= k < e_(b+1), added in ascending k from 0.0f.  set_bands takes bands + 1 HOST integers,
 *                     checked on the host: 0 <= e_0 < e_1 < ... < e_bands <= 513; the first edge that breaks the rule
 *                     is named and the plan keeps its edges.  A new plan holds e_b = floor(513 b / bands).  set_bands is
 *                     a blocking copy: in force from the next call; it is the caller's to have no call of the plan in
 *                     flight on a non-blocking stream.
 *   channel pairs   Tracks 2q and 2q + 1 share one complex transform (an odd last track beside zeros), as in
 *                   gab_fft_r2c_1024: a track's absolute error in any bin follows its PAIR's spectral peak, not its own
 *                   (tests/test_spectrum_gpu.py holds every frame within four times the float32 restatement of
 *                   tests/spectrum_twin.py, over peak_a + peak_b).  A silent track beside a loud partner holds the
 *                   partner's rounding error.  A silent pair gives zeros.  A pair depends on nothing outside itself,
 *                   bit for bit; a NaN or an infinity in one track makes the frames of its pair that hold it non-finite
 *                   (at most ceil(N / H) of them) and touches no other pair and no later frame.
 *   determinism     A frame's bits depend on two things only: the 1024 windowed samples of its pair, and (powers) S.
 *                   Not on B, on how the stream was cut into calls or batches, on the alignment of d_in, on the hop or
 *                   on which other frames were in the launch.  The band form's bits are the ordered float32 sum of the
 *                   bin form's bits.  A pair-aligned shard of tracks as its own plan gives those tracks' bits.
 *   layout          d_in [n][T][B] float32, track-major per buffer, any 4-byte alignment, never written; d_rows may not
 *                   overlap it.  process is process_batch with n = 1.
 *   reset           zeroes the history and the position; the window and the edges stay.
 *   state           the plan's own memory, for inspection: d_hist [T][1023], the last 1023 samples oldest first;
 *                   d_window [1024]; the third value is p mod H.
 * A call is two launches on `stream`, the frames and then (a wave per track, every value in a register before any is
 * written) the history, so no frame races with the history it reads; it allocates nothing and waits for nothing, and all
 * changing state but p mod H is on the device.  The frame phase p mod H and the count are launch arguments: a captured
 * process replays one phase ("Captured calls", above) and is the stream's next buffer only where H divides B, where
 * the phase is 0 and the count B / H on every call.  Arguments are checked before any device call: tracks >= 1,
 * bufsize >= 1, 32 <= hop <= 1024, bands 0..64 and 0 with GAB_SPEC_COMPLEX, n_buffers B < 2^31 - 1024, and at most
 * 2^23 workgroups (frames x ceil(T / 8)) a call.  Out of scope: averaging, peak hold or decay across frames (a line of
 * torch on the rows), other transform sizes, a window per track, complex rows in bands.  (The inverse is the resynthesis
 * plan, gab_resyn_*, below.)  One thread at a time per plan.                                                         */
typedef struct gab_spec_plan gab_spec_plan;
#define GAB_SPEC_COMPLEX 0
#define GAB_SPEC_POWER 1
int gab_spec_create(gab_spec_plan** plan, int tracks, int bufsize, int hop, int mode, int bands);
int gab_spec_destroy(gab_spec_plan* plan);
int gab_spec_set_window(gab_spec_plan* plan, const float* d_window, gab_stream_t stream);
int gab_spec_set_bands(gab_spec_plan* plan, const int* h_edges);
int gab_spec_reset(gab_spec_plan* plan, gab_stream_t stream);
int gab_spec_process(gab_spec_plan* plan, const float* d_in, float* d_rows, int* n_frames, gab_stream_t stream);
int gab_spec_process_batch(gab_spec_plan* plan, const float* d_in, float* d_rows, int n_buffers, int* n_frames,
                           gab_stream_t stream);
int gab_spec_frames(gab_spec_plan* plan, int n_buffers, int* capacity);
int gab_spec_state(gab_spec_plan* plan, float** d_hist, float** d_window, int* position_mod_hop);

/* ---- resynthesis: the overlap-add inverse of the spectrum plan, with a carried accumulator (additive; no counterpart in
 * the reference) -----------------------------------------------------------------------------------------------------
 * The synthesis half: the complex rows of a spectrum plan, whatever was done to them in between (a gate, a per-bin
 * equaliser, a freeze, any torch operation on [frames][T][513][2]), become a stream again.  N = 1024 is the transform,
 * B = bufsize, H the hop (fixed at create, 32 <= H <= 1024, any integer), T = tracks.
 *   rows in         d_rows [frames][T][513][2] float32, exactly what GAB_SPEC_COMPLEX writes (bins 0..512, re then im),
 *                   on an 8-byte boundary, never written; it may not overlap d_out.  The imaginary parts of bins 0 and
 *                   512 are READ AS ZERO, whatever the row holds (in the packed pair below they would otherwise leak
 *                   from one track of a pair into the other).
 *   frames taken    A call that produces the output samples [p, p + n B) takes exactly the frames j with
 *                   p < jH <= p + n B, in ascending j: the frames a spectrum plan of the same B and H emits for the same
 *                   call of the same cut.  floor((p + n B) / H) - floor(p / H) of them, possibly none.  The count is
 *                   host integer arithmetic on the carried p mod H and is returned in *n_frames without touching the
 *                   device; d_rows must hold that many frames (and is not read in a call that takes none).
 *                   gab_resyn_frames gives the largest count any call of n_buffers buffers can take,
 *                   ceil(n_buffers B / H); gab_resyn_count gives the count the NEXT call of n_buffers buffers takes,
 *                   without moving the plan.
 *   a frame         u_j[n] = x_j[n] * 2^-10, x_j the unnormalised real inverse 1024-point transform of the Hermitian
 *                   extension of the track's row of frame j, in float32;
 *                   v_j[n] = g[n] * u_j[n]                                one float32 product, rounded once
 *                   with g the synthesis window.
 *   the sum         y[a], a >= -N, is the float32 sum of v_j[a - (jH - N)] over the frames j >= 1 with
 *                   jH - N <= a < jH, added in ascending j starting from +0.0f, one addition per frame, rounded once and
 *                   never fused with the product.
 *   output, latency d_out [n][T][B] float32, the layout of the analyser's input, any 4-byte alignment.  Output sample o
 *                   (absolute since create or reset) is y[o - N]: the latency is 1024 samples (gab_resyn_latency), the
 *                   same for every H and B, and to within one sample the smallest that holds for every cut (the frame
 *                   that ends one sample past a call's end still adds to the sample 1023 places before it).  The
 *                   shorter N - H that a plan whose hop divides its buffer could have is out of scope.  The first H
 *                   outputs after a reset are +0.0f; outputs H .. N - 1 are y at negative indices exactly as the sum
 *                   gives them (rounding-level values for an analyser's rows: its first frames reach back before the
 *                   stream), and nothing special-cases them.
 *   state           One accumulator d_acc [T][1024].  After a call that ends at position P, acc[i] is the partial sum of
 *                   y[P - N + i] over every frame with jH <= P; acc[0] is then complete.  Also carried: the window
 *                   [1024] and p mod H.  gab_resyn_state exposes all three, the plan's own memory, for inspection.
 *                   reset zeroes the accumulator and the position; the window stays.
 *   window          g: 1024 floats, the same for every track.  set_window takes d_window (device, [1024]), checked on
 *                   the device: the first value that is not finite is named with GAB_ERR_INVALID_ARG, and a refused set
 *                   leaves the plan as it was.  There is no rule on a sum.  An accepted window acts on the frames of the
 *                   next call; what is in the accumulator stays.  Synchronous with respect to `stream`.
 *                   A new plan holds the least-squares dual of the spectrum plan's periodic Hann window w at its hop,
 *                     g[n] = w[n] / sum_m w[n + m H]^2      m over every index inside 0..1023, ascending; 0 where the
 *                                                           sum is 0
 *                   in float64 on the float32 values of w, rounded once: sum_j w[a - jH + N] g[a - jH + N] = 1 for every
 *                   a, so analyser -> resynthesis returns the stream delayed by 1024 samples.  The dual is
 *                   ILL-CONDITIONED as H approaches 1024, where the frames overlap only in the window's skirts: the
 *                   largest |g| is 0.67 / 1.2 / 2.6 / 430 / 1e5 at H = 256 / 512 / 700 / 1000 / 1023, and at H = 1024
 *                   Hann's zero at n = 0 cannot be undone: sample 0 of every frame is lost.
 *   channel pairs   Tracks 2q and 2q + 1 share one complex inverse (an odd last track beside zeros):
 *                   Z[k] = Xa[k] + i Xb[k] for k <= 512, Z[N - k] = conj(Xa[k]) + i conj(Xb[k]) for 0 < k < 512; the real
 *                   part of the inverse is track a, the imaginary part track b.  A track's absolute error follows its
 *                   PAIR's peak (tests/test_resynthesis_gpu.py holds every frame within four times the float32
 *                   restatement of tests/resynthesis_twin.py, over peak_a + peak_b in time).  A silent pair gives zeros.
 *                   A pair depends on nothing outside itself, bit for bit.  A NaN or an infinity in one row makes that
 *                   frame's 1024 output samples of its pair non-finite and touches nothing else: an emitted sample's
 *                   accumulator slot is STORED as zero, not scaled, so nothing lingers.
 *   determinism     u_j's bits depend on the pair's two rows of frame j alone (bins 0 and 512 as ruled above).  The
 *                   output's bits depend on the u_j, on g and on the order above; not on B, on how the stream was cut
 *                   into calls or batches, on the alignment of d_out or on which frames share a launch.  A pair-aligned
 *                   shard of tracks as its own plan gives those tracks' bits.
 * A call is one launch on `stream` (a wave per pair walks the call's frames in ascending j: that walk is the order of the
 * sum; no atomics, no scratch); it allocates nothing and waits for nothing, and all changing state but p mod H is on the
 * device.  The frame phase p mod H and the count are launch arguments: a captured process replays one phase ("Captured
 * calls", above) and is the stream's next buffer only where H divides B.  Arguments are checked before any device call:
 * tracks >= 1, bufsize >= 1, 32 <= hop <= 1024, tracks <= 2^26 (2^23 workgroups of eight tracks), n_buffers B <
 * 2^31 - 1024, null pointers, d_rows on an 8-byte boundary and apart from d_out.  Out of scope: other transform sizes,
 * a window per track, the N - H latency, any spectral processor itself (a gate per bin between the two plans, and both
 * fused around it, is the denoise plan, gab_dn_*, below).  One thread at a time per plan.                           */
typedef struct gab_resyn_plan gab_resyn_plan;
int gab_resyn_create(gab_resyn_plan** plan, int tracks, int bufsize, int hop);
int gab_resyn_destroy(gab_resyn_plan* plan);
int gab_resyn_set_window(gab_resyn_plan* plan, const float* d_window, gab_stream_t stream);
int gab_resyn_reset(gab_resyn_plan* plan, gab_stream_t stream);
int gab_resyn_process(gab_resyn_plan* plan, const float* d_rows, float* d_out, int* n_frames, gab_stream_t stream);
int gab_resyn_process_batch(gab_resyn_plan* plan, const float* d_rows, float* d_out, int n_buffers, int* n_frames,
                            gab_stream_t stream);
int gab_resyn_frames(gab_resyn_plan* plan, int n_buffers, int* capacity);
int gab_resyn_count(gab_resyn_plan* plan, int n_buffers, int* frames);
int gab_resyn_state(gab_resyn_plan* plan, float** d_acc, float** d_window, int* position_mod_hop);
int gab_resyn_latency(gab_resyn_plan* plan, int* samples);

/* ---- denoise: a spectral noise gate per track and bin, fused between analysis and resynthesis (additive; no
 * counterpart in the reference) ---------------------------------------------------------------------------------------
 * Broadband noise reduction in the style of "take a noise profile, then reduce": every bin of every frame is compared
 * with its own threshold, and a smoothed gain per (track, bin) follows the verdict.  Two forms share one state and one
 * arithmetic: the FUSED form (process, process_batch) takes the stream and returns the stream in one launch, the rows
 * never leaving the wave; the ROWS form (process_rows) takes the complex rows of a spectrum plan and returns rows for a
 * resynthesis plan.  N = 1024 is the transform, B = bufsize, H the hop (fixed at create, 32 <= H <= 1024, any integer),
 * T = tracks.
 *   the contract    On one device, the fused form equals
 *                     gab_spec_* (GAB_SPEC_COMPLEX, same B and H) -> gab_dn_process_rows -> gab_resyn_* (same B and H)
 *                   with the same tables and windows BIT FOR BIT: the outputs, d_hist against the analyser's history,
 *                   d_acc against the resynthesiser's accumulator, d_mask and p mod H, after every call of any cut.
 *   analysis        exactly the spectrum plan's: frame j is the 1024 samples that end at stream position jH, the last
 *                   1023 samples per track are carried in d_hist [T][1023], the windowed sample is one float32 product
 *                   w[n] * x, tracks 2q and 2q + 1 share one complex transform and are unpacked as gab_fft_r2c_1024
 *                   does it.  A new plan holds the spectrum plan's periodic Hann window, bit for bit, and its
 *                   inv_k = (float)(4 / S^2) for 0 < k < 512, (float)(1 / S^2) for k = 0 and 512.
 *   the gate        per frame j in ascending order, track t, bin k = 0..512, on the bin (re, im); every operation is
 *                   rounded once and nothing is fused but the one fmaf:
 *                     P   = ((re * re) + (im * im)) * inv_k        bit for bit GAB_SPEC_POWER's value of that bin
 *                     tg  = (P > thr[t][k]) ? 1.0f : floor[t]      strict; a NaN P compares false
 *                     c   = (tg > m[t][k]) ? att[t] : rel[t]
 *                     m[t][k] = fmaf(c, m[t][k] - tg, tg)          the gate plan's glide
 *                     re' = m[t][k] * re;  im' = m[t][k] * im
 *                   m is carried in d_mask [T][513] and is 1.0f after create and reset.  With 0 <= c < 1 every rounded
 *                   step stays between the old m and tg, so with floor <= 1 m stays within [the smallest floor seen, 1];
 *                   and tg is one of two finite values, so m never holds a NaN or an infinity, whatever the input.
 *                   With floor 0 and rel 0.5 a shut bin's m halves exactly, through the subnormals, to +0.
 *   synthesis       exactly the resynthesis plan's: the pair is packed, the imaginary parts of bins 0 and 512 are read as
 *                   zero, the inverse is scaled by 2^-10, multiplied once by the synthesis window g[n], and added with one
 *                   rounded addition per frame in ascending j into d_acc [T][1024]; emitted slots are stored as zero.
 *                   Output sample o is the gated stream's sample o - 1024 (gab_dn_latency).  A new plan holds the
 *                   least-squares dual of Hann at H, the values gab_resyn_create makes.
 *   tables          thr [T][513]: every value >= 0, or +inf (that bin is always shut); a NaN and a negative value are
 *                   refused.  A new plan holds zeros.  params [T][GAB_DN_FIELDS] = {floor, att, rel} per track with
 *                   0 <= floor <= 1, 0 <= att < 1, 0 <= rel < 1; a new plan holds {1, 0, 0}.  So a new plan is
 *                   transparent: its output is the bits of spectrum plan -> resynthesis plan.  att and rel are per FRAME:
 *                   exp(-H / (fs t)) for a time constant t.  Both sets take a device table for tracks [first_track,
 *                   first_track + n_tracks), checked on the device first: the first value that breaks its rule is named
 *                   (track, bin or field) with GAB_ERR_INVALID_ARG and the plan keeps its table.  An accepted set acts
 *                   from the next frame processed, unramped (the gain law itself is the glide); the state is kept.
 *                   gab_dn_tables exposes both tables, the plan's own memory.  Synchronous with respect to `stream`.
 *   windows         set_windows takes both, each device [1024]: every value finite, and the analysis sum S not zero (it
 *                   scales P).  Both are checked before either is written; a refused set keeps both.
 *   rows form       d_rows_in, d_rows_out [n_frames][T][513][2], any n_frames >= 0, on 8-byte boundaries; d_rows_out is
 *                   d_rows_in itself or apart from it (a partial overlap is refused).  It advances the mask ONLY: the
 *                   history, the accumulator and the position belong to the analyser and the resynthesiser beside it.
 *                   One launch, a thread per (track, bin) that walks the frames in order.
 *   fused form      d_in, d_out [n][T][B] float32, any 4-byte alignment.  d_in may NOT overlap d_out: the output is
 *                   delayed, and a later frame still reads input that the delayed output would already have overwritten.
 *   reset           d_hist and d_acc become zero, d_mask 1.0f, the position 0; the tables and the windows stay.
 *   state           gab_dn_state: d_hist [T][1023], d_acc [T][1024], d_mask [T][513], p mod H; the plan's own memory.
 *   channel pairs   as in both plans: a pair depends on nothing outside itself, bit for bit; a silent pair gives zeros.
 *                   A NaN or an infinity in the input stays in its pair and in the 1024-sample spans of the frames that
 *                   hold it, and leaves the mask finite.
 *   determinism     Output bits depend on the pair's samples, the tables and the order of frames.  Not on B, on the cut
 *                   into calls or batches, on the alignment of d_in and d_out, or on which frames share a launch.  A
 *                   pair-aligned shard of tracks as its own plan gives those tracks' bits.
 * A fused call is one launch on `stream` (a wave per pair walks the call's frames in ascending j and owns the pair's
 * state: no atomics, no scratch, no second launch); it allocates nothing and waits for nothing, and all changing state but
 * p mod H is on the device.  The frame phase p mod H and the count are launch arguments: a captured process replays one
 * phase ("Captured calls", above) and is the stream's next buffer only where H divides B.  Arguments are checked before
 * any device call: tracks >= 1, bufsize >= 1, 32 <= hop <= 1024, tracks <= 2^26, n_buffers B < 2^31 - 1024, null
 * pointers, the track range of a set, the overlaps and alignments above.  Out of scope: smoothing across bins, a hold
 * counter, subtractive or Wiener gain laws, one threshold table for all tracks, other transform sizes, the N - H
 * latency, ramped table sets.  One thread at a time per plan.                                                       */
typedef struct gab_dn_plan gab_dn_plan;
#define GAB_DN_FIELDS 3
int gab_dn_create(gab_dn_plan** plan, int tracks, int bufsize, int hop);
int gab_dn_destroy(gab_dn_plan* plan);
int gab_dn_set_thresholds(gab_dn_plan* plan, const float* d_thr, int first_track, int n_tracks, gab_stream_t stream);
int gab_dn_set_params(gab_dn_plan* plan, const float* d_params, int first_track, int n_tracks, gab_stream_t stream);
int gab_dn_set_windows(gab_dn_plan* plan, const float* d_analysis, const float* d_synthesis, gab_stream_t stream);
int gab_dn_reset(gab_dn_plan* plan, gab_stream_t stream);
int gab_dn_process(gab_dn_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_dn_process_batch(gab_dn_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_dn_process_rows(gab_dn_plan* plan, const float* d_rows_in, float* d_rows_out, int n_frames,
                        gab_stream_t stream);
int gab_dn_state(gab_dn_plan* plan, float** d_hist, float** d_acc, float** d_mask, int* position_mod_hop);
int gab_dn_tables(gab_dn_plan* plan, float** d_thr, float** d_params);
int gab_dn_latency(gab_dn_plan* plan, int* samples);

/* ---- saturator: a waveshaper per track between an interpolator by R and a decimator by R, fused (additive; no
 * counterpart in the reference) ---------------------------------------------------------------------------------------
 * Drive into a curve colours a signal and, at the stream's own rate, folds the new harmonics back below Nyquist.  The
 * plan shapes at R times the rate: up by R, the curve, down by R, in one launch.  T = tracks, B = bufsize, R =
 * oversample in {1, 2, 4, 8}, Ku = up_taps, Kd = down_taps; `curve` is one curve for the plan.
 *   the contract    On one device, the fused form (process, process_batch) equals
 *                     gab_resample_* (T, B, up R, down 1, taps Ku) -> gab_sat_apply -> gab_resample_* (T, R B, up 1,
 *                     down R, taps Kd)
 *                   BIT FOR BIT: the outputs, d_hist_in against the first resampler's history and d_hist_os against the
 *                   second's, after every call of any cut.  At R = 1 process is apply.
 *   rows            [T][GAB_SAT_FIELDS] float32 = {drive, bias, level} per track; a new plan holds {1, 0, 1}.  One rule:
 *                   every field finite.  set_params (all tracks) and set_params_tracks ([first_track, first_track +
 *                   n_tracks)) take a device table, checked on the device first: the first refused value is named as
 *                   (track, field) with GAB_ERR_INVALID_ARG and the plan keeps its parameters.  ramp = 0: in force at
 *                   once.  ramp = 1: over the next buffer processed, base sample s of that buffer takes, per field,
 *                     fmaf(target - current, r[s], current),  r[s] = (float)((s + 1) / B)    (float64, rounded once)
 *                   and all R oversampled samples of base sample s take that row; behind that buffer current := target.
 *                   In a batch only the first buffer ramps.  Synchronous with respect to `stream`.
 *   stage 1, up     (R >= 2) w is the track's input stream, zero before the first sample after a reset:
 *                     u[R i + p] = fmaf(h_p[Ku-1], w[i-Ku+1], ... fmaf(h_p[1], w[i-1], h_p[0] * w[i]))     p = 0..R-1
 *                   the resample plan's chain with its table for L = R, M = 1 ("taps" above; the one design function).
 *   stage 2, curve  per oversampled sample, every operation rounded once:
 *                     a = fmaf(drive, u, bias);   v = level * (S(a) - S(bias))
 *                   so silence stays silence under a bias.  S is written with comparisons, and a NaN passes through:
 *                     GAB_SAT_HARD      S(x) = x > 1 ? 1 : (x < -1 ? -1 : x)
 *                     GAB_SAT_CUBIC     c = HARD(x);  c2 = c * c;  S = c * fmaf(-0.5f, c2, 1.5f)   (+-1 at the rails,
 *                                       slope 0 there)
 *                     GAB_SAT_RATIONAL  S(x) = x / (1.0f + fabsf(x))                (the IEEE division, rounded once)
 *                   No library transcendental anywhere.  At R = 1, u is the input itself.
 *   stage 3, down   (R >= 2) base output m is the resample plan's chain with its one-row table g for L = 1, M = R:
 *                     y[m] = fmaf(g[Kd-1], v[m R - Kd + 1], ... fmaf(g[1], v[m R - 1], g[0] * v[m R]))
 *   latency         Ku / 2 + Kd / (2 R) base samples, the same for every track; 0 at R = 1 (gab_sat_info).
 *   state           d_hist_in [T][Ku-1]: the last Ku-1 inputs; d_hist_os [T][Kd-1]: the last Kd-1 shaped oversampled
 *                   samples; both oldest first, zero after create and reset, and right when B < Ku-1 or R B < Kd-1: they
 *                   are shifted, not replaced.  gab_sat_state exposes both and the two tap tables d_up [R][Ku] and
 *                   d_down [Kd], the plan's own memory (all four null at R = 1).  reset also makes current := target
 *                   and drops a pending ramp; the taps stay.
 *   set_taps        d_up [R][Ku], d_down [Kd], device.  Both are checked on the device before either is written: the first
 *                   value that is not finite is named as (table, phase, tap) with GAB_ERR_INVALID_ARG and the plan keeps
 *                   both tables.  The histories are kept; accepted taps are in force from the next buffer.  Refused at
 *                   R = 1, which has no taps.  Synchronous with respect to `stream`.
 *   fused form      d_in, d_out [n][T][B] float32, any 4-byte alignment (16-byte loads and stores where both pointers
 *                   and B allow).  d_out may not overlap d_in (refused): the output is delayed.  One launch on `stream`: a
 *                   workgroup owns 16 tracks for the whole call, every buffer of a batch included, walks them in chunks
 *                   of 64 base samples through LDS and is the only reader and writer of their histories: no second
 *                   launch.  process_batch gives the bits of n process calls.
 *   curve form      gab_sat_apply: stage 2 alone on d_in, d_out [n_buffers][T][R B] oversampled blocks, base sample s of
 *                   a row being its samples [R s, R s + R).  d_out may be d_in itself (any other overlap is refused).
 *                   It consumes a pending ramp exactly as process_batch would and touches no history.
 *   determinism     Output bits depend on the track's samples, its rows and the taps.  Not on B, on the cut into calls
 *                   or batches, or on alignment.  A shard of tracks as its own plan gives those tracks' bits.  A NaN or
 *                   an infinity stays in its track, and is gone from the output once the input that made it has left
 *                   both windows: Ku - 1 + ceil((Kd - 1) / R) base samples behind it.
 * Every call allocates nothing and waits for nothing but the sets, and all changing state but the pending flag is on the
 * device: capture with no ramp pending ("Captured calls", above).  Arguments are checked before any device call, each
 * refusal with its own text: tracks >= 1, 1 <= bufsize <= 2^20, oversample in {1, 2, 4, 8}, curve in 0..2; at R >= 2
 * up_taps even and in 4..64, down_taps in 4..256 and a multiple of 2 R (so that the latency is a whole number of
 * samples); at R = 1 both 0; null pointers, n_buffers >= 1, the track range of a set, the overlaps above.  Fewer than 16
 * tracks x 256 use a part of the device.  Out of scope: a dry / wet mix (the dry path needs its own delay line: the
 * delay and mix plans do it), a curve per track, tanh or any transcendental curve, minimum-phase filters, in-place
 * process.  One thread at a time per plan.                                                                          */
typedef struct gab_sat_plan gab_sat_plan;
#define GAB_SAT_FIELDS 3
#define GAB_SAT_HARD 0
#define GAB_SAT_CUBIC 1
#define GAB_SAT_RATIONAL 2
int gab_sat_create(gab_sat_plan** plan, int tracks, int bufsize, int oversample, int curve, int up_taps,
                   int down_taps);
int gab_sat_destroy(gab_sat_plan* plan);
int gab_sat_info(gab_sat_plan* plan, int* oversample, int* curve, int* up_taps, int* down_taps, int* latency);
int gab_sat_set_params(gab_sat_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_sat_set_params_tracks(gab_sat_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                              gab_stream_t stream);
int gab_sat_set_taps(gab_sat_plan* plan, const float* d_up, const float* d_down, gab_stream_t stream);
int gab_sat_reset(gab_sat_plan* plan, gab_stream_t stream);
int gab_sat_process(gab_sat_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_sat_process_batch(gab_sat_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_sat_apply(gab_sat_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_sat_params(gab_sat_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_sat_state(gab_sat_plan* plan, float** d_hist_in, float** d_hist_os, float** d_up, float** d_down);

/* ---- nlms: an adaptive filter per track, normalised LMS (additive; no counterpart in the reference) ---------------
 * An echo canceller, a feedback suppressor, hum or bleed removal with a reference: per track the plan reads a
 * REFERENCE x (the far end, the loudspeaker feed) and an INPUT d (the microphone), writes the ESTIMATE y, x through the
 * track's taps, and the ERROR e = d - y, the input with the echo removed, and adapts the taps on every sample.  With
 * the step mu at 0 it is an FIR filter with its own taps per track.  T = tracks, B = bufsize, L = taps = 64 R with R in
 * {1, 2, 4, 8}.
 *   the arithmetic  Every operation is rounded once in float32.  Tap k = 64 q + l (q = 0..R-1, l = 0..63); the window
 *                   is X[k] = x[n - k], zero before the stream's start and after a reset.  Per sample n, ascending:
 *                     y   = T( C_q( w[64 q + l], X[64 q + l] ) )
 *                             C_q, per l: acc = w[l] * X[l] (one rounded product), then
 *                                         acc = fmaf(w[64 q + l], X[64 q + l], acc) for q = 1 .. R-1;
 *                             T: the balanced binary tree over l = 0..63 in natural order, adjacent pairs first:
 *                                32 sums of (2i, 2i + 1), then 16 of those, down to 1, each one rounded addition;
 *                     P   = T( C_q( X, X ) )      the same chain and tree on the squares, recomputed on every sample:
 *                                                 no running sum, so it cannot drift, is never negative and forgets a
 *                                                 bad sample after L samples;
 *                     e   = d[n] - y
 *                     den = P + eps
 *                     s   = mu / den              (the IEEE division)
 *                     g   = s * e
 *                     if g is finite (its exponent bits are not all ones):  w[k] = fmaf(g, X[k], w[k]) for every k;
 *                     otherwise the taps are left as they are;
 *                     err[n] = e,  est[n] = y     both from the taps BEFORE this sample's update.
 *   bad inputs      An X[k] that is not finite makes y, hence e, hence g not finite: an infinity or a NaN in x reaches
 *                   err and est for exactly L samples and never a tap; one in d reaches one sample of err and never a
 *                   tap.  One track's samples never reach another track.  Overflow of a tap by FINITE arithmetic
 *                   (samples near FLT_MAX) is not guarded.
 *   rows            [T][GAB_NLMS_FIELDS] float32 = {mu, eps} per track.  A new plan holds zero taps and {0, 1}: est is all
 *                   +0 and err is d, bit for bit.  The rule: mu finite and 0 <= mu <= 2 (-0.0 is taken); eps finite and
 *                   2^-126 <= eps <= 2^64.  set_params (all tracks) and set_params_tracks ([first_track, first_track +
 *                   n_tracks)) take a device table, checked on the device first: the first refused value is named as
 *                   (track, field) with GAB_ERR_INVALID_ARG and the plan keeps its tables.  ramp = 0: in force at once.
 *                   ramp = 1: over the next buffer processed (in a batch, its first), sample s takes, per field,
 *                     fmaf(target - current, r[s], current),  r[s] = (float)((s + 1) / B)    (float64, rounded once)
 *                   and behind that buffer current := target.  Synchronous with respect to `stream`.
 *   state           d_taps [T][L]; d_history [T][L - 1], the last L - 1 reference samples, oldest first, shifted and
 *                   not replaced, so right when B < L - 1.  Both on the device, exposed by gab_nlms_state (the plan's
 *                   own memory).  set_taps / set_taps_tracks take device tables [n][L] of finite values (the first
 *                   that is not is named as (track, tap), and the plan keeps its taps), are not ramped, are in force
 *                   from the next sample processed and leave the history alone; synchronous with respect to `stream`.
 *                   reset: taps and history zero, current := target, a pending ramp dropped.
 *   blocks          d_in (d), d_ref (x), d_err, d_est: [n][T][B] float32, track-major, any 4-byte alignment, any B >= 1.
 *                   One of d_err and d_est may be null (both: refused).  d_err may be d_in itself and d_est may be d_ref
 *                   itself; every other overlap between an output and anything else is refused with its text.  One
 *                   launch on `stream` per call or batch: a wave per track, four a workgroup, no workgroup barrier and
 *                   no atomics; the wave holds its track's taps and window in registers for the whole call, so a batch
 *                   moves the state once.  process_batch gives the bits of n process calls.
 *   determinism     Output bits depend on the track's samples, its row and its taps.  Not on B, on the cut into calls or
 *                   batches, or on alignment.  A shard of tracks as its own plan gives those tracks' bits.
 * process and process_batch allocate nothing and wait for nothing, and all changing state but the pending flag is on
 * the device: capture with no ramp pending ("Captured calls", above).  Arguments are checked before any device call,
 * each refusal with its own text: tracks and bufsize >= 1, taps in {64, 128, 256, 512}, null pointers, n_buffers >= 1,
 * the track range of a set, the overlaps above.  Fewer than 1024 tracks use a part of the device.  Out of scope: a leak
 * term, double-talk detection, frequency-domain or block-exact forms, tap counts that are not 64 * 2^k, a call-level
 * "do not adapt" kernel form (mu = 0 runs the same kernel), linked tracks.  One thread at a time per plan.              */
typedef struct gab_nlms_plan gab_nlms_plan;
#define GAB_NLMS_FIELDS 2
int gab_nlms_create(gab_nlms_plan** plan, int tracks, int bufsize, int taps);
int gab_nlms_destroy(gab_nlms_plan* plan);
int gab_nlms_set_params(gab_nlms_plan* plan, const float* d_params, int ramp, gab_stream_t stream);
int gab_nlms_set_params_tracks(gab_nlms_plan* plan, const float* d_params, int first_track, int n_tracks, int ramp,
                               gab_stream_t stream);
int gab_nlms_set_taps(gab_nlms_plan* plan, const float* d_taps, gab_stream_t stream);
int gab_nlms_set_taps_tracks(gab_nlms_plan* plan, const float* d_taps, int first_track, int n_tracks,
                             gab_stream_t stream);
int gab_nlms_reset(gab_nlms_plan* plan, gab_stream_t stream);
int gab_nlms_process(gab_nlms_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                     gab_stream_t stream);
int gab_nlms_process_batch(gab_nlms_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                           int n_buffers, gab_stream_t stream);
int gab_nlms_params(gab_nlms_plan* plan, float** d_current, float** d_target, size_t* n_floats);
int gab_nlms_state(gab_nlms_plan* plan, float** d_taps, float** d_history, int* taps);

/* ---- fdaf: a block adaptive filter per track, partitioned frequency-domain NLMS (additive; no counterpart) ---------
 * The nlms plan's long form, the multidelay block filter (MDF): K = partitions of 512 taps each, L = 512 K taps up to
 * 16 384 (341 ms at 48 kHz), adapted per bin once per BLOCK of 512 samples with 1024-point overlap-save transforms.
 * d (d_in) is the microphone, x (d_ref) the far end; est is x through the taps, err = d - est.  With mu = 0 and set_taps
 * it is a partitioned FIR filter with its own long taps per track.  T = tracks, B = bufsize, a positive multiple of 512
 * (other sizes are refused): a buffer is B / 512 blocks, walked in order.  K in 1..32, any integer.
 *   pairs           Tracks 2q and 2q + 1 share every transform as a + i b, as the spectrum, resynthesis and denoise
 *                   plans' do.  An odd last track stands beside a partner of zero samples, zero taps and the row {0, 1},
 *                   of which nothing is stored.
 *   state           W [T][K][513][2], the partitions' half-spectra; X [T][K][513][2], the delay line as a ring: block
 *                   b's spectra sit in slot b mod K; prev [T][512], the reference block before; count [T] (uint32), the
 *                   blocks since the reset, skipped ones included (it wraps after 2^32 blocks).  On the device, exposed
 *                   by gab_fdaf_state as the plan's own memory.  A new plan and a reset hold zeros everywhere.
 *   the arithmetic  float32, every operation rounded once; fmaf is one rounding.  The two complex products:
 *                     acc (+)= a b        re = fmaf(a.re, b.re, fmaf(-a.im, b.im, acc.re))
 *                                         im = fmaf(a.re, b.im, fmaf( a.im, b.re, acc.im))
 *                     acc (+)= conj(a) b  re = fmaf(a.re, b.re, fmaf( a.im, b.im, acc.re))
 *                                         im = fmaf(a.re, b.im, fmaf(-a.im, b.re, acc.im))
 *                   Per block b = count and pair, in this order:
 *                     1. X[b mod K] = the half-spectra of the pair's window [prev | x_b]: the spectrum plan's analysis
 *                        with a window of ones (no product), the same wave-held forward transform and unpack.  The
 *                        slot holds, bit for bit, the row gab_spec_* (hop 512, complex) writes for that frame.
 *                     2. Y[k] = sum_p X[(b - p) mod K][k] W_p[k], p ascending from acc = +0, the first product above;
 *                        S[k] = sum_p fmaf(im, im, fmaf(re, re, S)) of the same spectra, p ascending from +0.  S is
 *                        formed anew every block: it cannot drift, is never negative and forgets a bad block after K.
 *                     3. The pair's Y packed as the resynthesis plan packs its rows, the inverse transform;
 *                        est[n] = fmaf(z[512 + n], 2^-10, +0) (a -0 becomes +0), e[n] = d[n] - est[n].
 *                     4. THE SKIP.  If any of the pair's 1024 values of e (both tracks) is not finite, steps 5 to 7 are
 *                        skipped for this block and pair: W stays as it is, count still advances.
 *                     5. E = the half-spectra of [0 | e] (512 zeros, then the block's errors), as in step 1.
 *                     6. s[k] = mu / (S[k] + eps) (one addition, the IEEE division; per track); G[k] = (s E.re, s E.im);
 *                        W_p[k] (+)= conj(X[(b - p) mod K][k]) G[k] for every p, the second product above.
 *                     7. THE GRADIENT CONSTRAINT, alternated (the scheme of Speex's MDF): for partition c = b mod K
 *                        only, the pair's W_c packed, inverse, times 2^-10, samples 512..1023 stored as +0, forward,
 *                        unpacked as in step 1, stored.  One inverse and one forward a block whatever K is.  There is
 *                        no unconstrained mode: without it the misalignment stalls between -10 and -30 dB.
 *                   Then prev := x_b, count += 1.  A track whose mu is 0 never writes its W (its taps stay bit for bit,
 *                   where steps 6 and 7 would move them by roundings), and a pair of two such tracks leaves steps 5 to 7
 *                   out: an FIR filter costs two transforms and one pass a block.
 *   bad inputs      An infinity or a NaN in x lies in two windows, its block's and the next one's, so in the delay
 *                   line for K + 1 blocks: it is in that pair's err and est for exactly K + 1 blocks and never in W.
 *                   One in d is in err for that sample only and costs the pair one block of adaptation.  Nothing
 *                   crosses a pair.  Overflow by FINITE arithmetic (samples near FLT_MAX) is not guarded.
 *   rows            [T][GAB_FDAF_FIELDS] float32 = {mu, eps} per track.  A new plan holds {0, 1}: est is all +0 and err
 *                   is d, bit for bit.  The rule: mu finite and 0 <= mu <= 1 (-0.0 is taken); eps finite and 2^-126 <=
 *                   eps <= 2^64.  S is in the units of the unnormalised transform: white noise of power P gives about
 *                   1024 K P.  With K = 1 the filter diverges at mu = 1 and is fine at 0.5; K >= 4 takes 1.
 *                   set_params (all tracks) and set_params_tracks take a device table, checked on the device first: the
 *                   first refused value is named as (track, field) with GAB_ERR_INVALID_ARG and the plan keeps its
 *                   table.  UNRAMPED: a block is the step's own granularity, and with one block a buffer a ramp over a
 *                   buffer is nothing; in force from the next block processed.  Synchronous with respect to `stream`.
 *   taps            set_taps / set_taps_tracks take device tables [n][512 K] of finite time-domain taps (the first that
 *                   is not is named as (track, tap), and the plan keeps its taps) and fill W_p with the half-spectrum of
 *                   [h[512 p .. 512 p + 512) | 512 zeros], each track alone in its transform: a small launch of the
 *                   plan's own.  They leave X, prev and count alone; synchronous with respect to `stream`.  The taps in
 *                   time are the first 512 samples of each partition's inverse transform.
 *   blocks          d_in, d_ref, d_err, d_est: [n][T][B] float32, track-major, any 4-byte alignment.  One of d_err and
 *                   d_est may be null (both: refused).  d_err may be d_in itself and d_est may be d_ref itself; every
 *                   other overlap between an output and anything else is refused with its text.  One launch on `stream`
 *                   per call or batch: a wave per pair, four a workgroup, no workgroup barrier and no atomics; the wave
 *                   walks its pair's blocks in ascending order.  process_batch gives the bits of n process calls.
 *   determinism     Output bits depend on the pair's samples, rows and state.  Not on B, on the cut into calls or
 *                   batches, on alignment, or on which plan (a shard that starts on an even track) holds the pair.
 * process and process_batch allocate nothing and wait for nothing, and all changing state is on the device: they can be
 * captured ("Captured calls", above).  Arguments are checked before any device call, each refusal with its own text:
 * tracks and bufsize >= 1, bufsize a multiple of 512, partitions in 1..32, null pointers, n_buffers >= 1, n_buffers *
 * bufsize below 2^31 - 1024, the track range of a set, the overlaps above.  Fewer than 2048 tracks use a part of the
 * device.  Out of scope: double-talk detection, a leak term, other block or transform sizes (buffers of 64 to 256
 * samples), a smoothed power estimate, linked tracks, the gpubench driver, tests/walks.py, the strip helpers.  One
 * thread at a time per plan.                                                                                          */
typedef struct gab_fdaf_plan gab_fdaf_plan;
#define GAB_FDAF_FIELDS 2
int gab_fdaf_create(gab_fdaf_plan** plan, int tracks, int bufsize, int partitions);
int gab_fdaf_destroy(gab_fdaf_plan* plan);
int gab_fdaf_set_params(gab_fdaf_plan* plan, const float* d_params, gab_stream_t stream);
int gab_fdaf_set_params_tracks(gab_fdaf_plan* plan, const float* d_params, int first_track, int n_tracks,
                               gab_stream_t stream);
int gab_fdaf_set_taps(gab_fdaf_plan* plan, const float* d_taps, gab_stream_t stream);
int gab_fdaf_set_taps_tracks(gab_fdaf_plan* plan, const float* d_taps, int first_track, int n_tracks,
                             gab_stream_t stream);
int gab_fdaf_reset(gab_fdaf_plan* plan, gab_stream_t stream);
int gab_fdaf_process(gab_fdaf_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                     gab_stream_t stream);
int gab_fdaf_process_batch(gab_fdaf_plan* plan, const float* d_in, const float* d_ref, float* d_err, float* d_est,
                           int n_buffers, gab_stream_t stream);
int gab_fdaf_params(gab_fdaf_plan* plan, float** d_params, size_t* n_floats);
int gab_fdaf_state(gab_fdaf_plan* plan, float** d_W, float** d_X, float** d_prev, unsigned** d_count, int* partitions);

/* ---- mconv: a matrix of partitioned FIR filters, inputs summed into outputs (additive; no counterpart) -------------
 * What the mix plan does with a gain per (track, bus), with a filter per (output, input): a binaural renderer (sources
 * through a head-related response per ear), a true-stereo reverb (2 x 2), an array decoder, a crosstalk canceller.  I =
 * inputs 1..4096 (the plan's tracks, and what a refusal of the common entries calls them), O = outputs 1..64, K =
 * partitions 1..32 of 512 taps, L = 512 K taps per (output, input), I O K <= 65 536.  B = bufsize, a positive multiple
 * of 512: a buffer is B / 512 blocks.  d_in [n][I][B] and d_out [n][O][B] (bus-major, as the mix plan writes), float32
 * at any 4-byte alignment; any overlap of d_out with d_in is refused.
 *   state           H_current and H_target [O][I][K][513][2], the taps' half-spectra; X [S][I][513][2], the ring of
 *                   input spectra, S = K + 15 slots, block b in slot b mod S; prev [I][512], the input block before;
 *                   count, one uint32, the blocks since the reset (the ring's position is count mod S: a stream is
 *                   reset before 2^32 blocks, 1.4 years at 48 kHz).  On the device, exposed by gab_mconv_state as the
 *                   plan's own memory.  A new plan holds zeros everywhere: its output is all +0.  A reset zeroes X, prev
 *                   and count, keeps the taps and makes current := target (a pending ramp is dropped).
 *   the arithmetic  float32, every operation rounded once; the product is the fdaf section's first, acc (+)= a b.  Per
 *                   block b = count:
 *                     1. Inputs 2q and 2q + 1 share a forward transform as a + i b: the window [prev | x_b], no window
 *                        product, the stages of the fdaf plan's step 1.  X[b mod S] holds, bit for bit, the row
 *                        gab_spec_* (hop 512, complex, a window of ones) writes for that frame.  An odd last input
 *                        stands beside zeros.
 *                     2. The inputs fall into groups of 32 by their index, [32 g, 32 g + 32): a cut that depends on I
 *                        alone.  For output o and bin k the group partial is
 *                          P_g = sum of X_i[(b - p) mod S][k] H[o][i][p][k], i ascending over the group and inside it
 *                                p ascending, one chain from acc = +0;
 *                        then Y_o = ((P_0 + P_1) + P_2) ..., g ascending, re and im by one rounded addition each.
 *                     3. Outputs 2r and 2r + 1 share an inverse: Y packed as the fdaf plan's step 3 packs, the inverse
 *                        transform, y[n] = fmaf(z[512 + n], 2^-10, +0).  An odd last output stands beside a zero spectrum.
 *                     4. prev := x_b, count += 1.
 *   taps            set_taps (the whole table [O][I][512 K]) and set_taps_range (outputs [first_output, first_output +
 *                   n_outputs) x inputs [first_input, first_input + n_inputs), a table [n_outputs][n_inputs][512 K]) take
 *                   device tables of finite time-domain taps, checked on the device first: the first that is not is
 *                   named as (output, input, tap) with GAB_ERR_INVALID_ARG and the plan keeps its taps.  Each (output,
 *                   input, partition) is transformed alone, [h[512 p .. 512 p + 512) | 512 zeros], as the fdaf plan's
 *                   taps are.  Synchronous with respect to `stream`; X, prev and count stay.
 *                   ramped = 0: into both tables.  The ring holds input spectra only, so the new taps act on every
 *                   partition from the next block, and from there on the output is bit for bit that of a plan that had
 *                   them from the start and was fed the same stream.
 *                   ramped = 1: into H_target only, and the next buffer processed (of a batch: its first) is the ramp
 *                   buffer: steps 2 and 3 run against both tables and sample s of the buffer is
 *                   fmaf(y_target[s] - y_current[s], r[s], y_current[s]), r[s] = (s + 1) / B in float64, rounded once;
 *                   then current := target by a copy on that call's stream.  The click-free move of a source.
 *   bad inputs      An infinity or a NaN in an input lies in two windows, so in the ring for K + 1 blocks: it is in the
 *                   outputs for at most K + 1 blocks, and because NaN 0 is NaN in every output whatever its taps.  It
 *                   never reaches H.  From block K + 2 on the output is bit for bit that of a stream which held a zero
 *                   in its place.  Overflow by FINITE arithmetic is not guarded.
 *   determinism     Output bits depend on the samples, the taps and the state.  Not on B, on the cut into calls or
 *                   batches, on alignment, or on which plan holds an output pair: a plan that holds outputs [2r, 2r + n)
 *                   of the table gives those outputs' bits.
 *   calls           A call is rounds of at most 16 blocks, three launches a round on `stream` (the forward transforms; the
 *                   group partials into the plan's own scratch, no atomics; the sums and the inverses) and a fourth on
 *                   the blocks of a ramp buffer.  The ring has the slots for a round.  process_batch gives the bits of
 *                   n process calls.
 * process and process_batch allocate nothing and wait for nothing, and all changing state is on the device: they can be
 * captured ("Captured calls", above).  Arguments are checked before any device call, each refusal with its own text:
 * inputs (as tracks) and bufsize >= 1, inputs <= 4096, outputs in 1..64, partitions in 1..32, the product of the three,
 * bufsize a multiple of 512, null pointers, n_buffers >= 1, n_buffers * bufsize below 2^31 - 1024, the input (track)
 * range and the output range of a set, the overlap.  Out of scope: sparse tables, other transform sizes, buffers below
 * 512, non-uniform partitions, taps interpolated from a set, a taps getter, the gpubench driver, tests/walks.py, the
 * strip helpers.  One thread at a time per plan.                                                                      */
typedef struct gab_mconv_plan gab_mconv_plan;
int gab_mconv_create(gab_mconv_plan** plan, int inputs, int bufsize, int outputs, int partitions);
int gab_mconv_destroy(gab_mconv_plan* plan);
int gab_mconv_set_taps(gab_mconv_plan* plan, const float* d_taps, int ramped, gab_stream_t stream);
int gab_mconv_set_taps_range(gab_mconv_plan* plan, const float* d_taps, int first_output, int n_outputs, int first_input,
                             int n_inputs, int ramped, gab_stream_t stream);
int gab_mconv_reset(gab_mconv_plan* plan, gab_stream_t stream);
int gab_mconv_process(gab_mconv_plan* plan, const float* d_in, float* d_out, gab_stream_t stream);
int gab_mconv_process_batch(gab_mconv_plan* plan, const float* d_in, float* d_out, int n_buffers, gab_stream_t stream);
int gab_mconv_state(gab_mconv_plan* plan, float** d_H_current, float** d_H_target, float** d_X, float** d_prev,
                    unsigned** d_count, int* slots);

/* ===================================================================== */
/* G. host-side data generators of the harness                           */
/* ===================================================================== */

/* generateRandomAudioData (cuda/bench_utils.cu:238-245): mt19937(seed), U(-1,1). */
int gab_generate_noise(float* h_buf, size_t n, unsigned seed);
/* Conv1DBenchmark::generateImpulseResponses (cuda/bench_conv1d.cu:159-181) and
 * Conv1DAccelBenchmark::generateImpulseResponses (cuda/bench_conv1d_accel.cu:
 * 152-173).  The formulas use the GLOBAL track index and count: a shard asks
 * for tracks [track_offset, track_offset+n_tracks) of a bank of total_tracks.  */
int gab_generate_conv1d_ir(float* h_ir, int ir_len, size_t track_offset,
                           size_t n_tracks, size_t total_tracks);
int gab_generate_conv_accel_ir(float* h_ir, int ir_len, size_t track_offset,
                               size_t n_tracks, size_t total_tracks);

/* The stream glibc's srand(seed) + rand() gives (random_r.c TYPE_3), from its `skip`-th value on, as the harness draws it
 * for FFT1D's input and RndMemRead's pool and playheads (private generators: no other rand() user or thread moves
 * them, and a channel shard enters them at its first track).  Host arithmetic; additive.                          */
int gab_glibc_rand(unsigned seed, unsigned long long skip, int* out, size_t n);

/* Channel shards of a multi-GPU job (additive; BASELINE configs[4]): the contiguous range
 * [*lo, *hi) of `rank` out of `world`, the remainder going to the low ranks.  Host arithmetic.  */
int gab_shard_range(int rank, int world, size_t total_tracks, size_t* lo, size_t* hi);
/* The same cut at multiples of `granule` tracks, and the granule a benchmark (registry name) needs: FFT1D packs two
 * tracks into one complex transform (2), Conv1D_accel four channels into one workgroup's (4) — their bits depend on
 * which tracks share a transform, so their shards keep those groups whole; every other benchmark 1.            */
int gab_shard_range_aligned(int rank, int world, size_t total_tracks, size_t granule, size_t* lo, size_t* hi);
size_t gab_shard_granule(const char* benchmark);

/* calculateStatistics (cuda/bench_utils.cu:358-414): mean, median, sample
 * std-dev, min, max, linearly interpolated p95/p99.                          */
typedef struct {
    float  mean, median, std_dev, min_val, max_val, p95, p99;
    size_t count;
} gab_statistics;
int gab_calculate_statistics(const float* latencies, size_t n, gab_statistics* out);
/* The CLI-backed process globals the legacy writers read (cuda/globals.cu:4-7). */
int gab_set_globals(int fs, int buffer_size, int n_tracks, int n_runs);
/* generateJSONResults (cuda/globals.cu:137-182) into buf (NUL-terminated);
 * returns the length the full text needs, excluding the NUL.                 */
size_t gab_format_json_results(const float* latencies, size_t n, const char* name,
                               char* buf, size_t capacity);
/* writeCSVResults (cuda/globals.cu:69-122): appends one row, header if new.  */
int gab_write_csv_results(const float* latencies, size_t n, const char* name,
                          const char* filename);

/* ===================================================================== */
/* H. harness (GPUABenchmark by registry name)                           */
/* ===================================================================== */

typedef struct gab_bench gab_bench;

typedef struct {
    int    fs, buffer_size, n_tracks, n_runs;       /* cuda/globals.cu:4-7     */
    int    ir_length;       /* <=0: the benchmark's DEFAULT_IR_LEN             */
    int    fdtd_grid;       /* <=0: 52 (bench_fdtd3d.cuh:36-38)                */
    int    conv_mode;       /* GAB_CONV_STATELESS | GAB_CONV_STREAMING | 2: streaming with every
                               iteration ONE gab_conv_round_trip call (--convMode roundtrip)   */
    int    quiet;           /* suppress the reference's progress printf        */
    int    modal_mode;      /* ModalFilterBank: 0 the CUDA port's placeholder
                               (bench_modal.cu:15-36), 1 the real bank (Metal port) */
    int    conv_batch;      /* Conv1D_accel: <=1 one buffer per iteration with its copies (the
                               reference); n: n HBM-resident buffers per iteration in ONE
                               gab_conv_process_batch launch (throughput mode)           */
    int    fdtd_form;       /* FDTD3D: GAB_FDTD_FORM_AUTO (0) | GAB_FDTD_FORM_STEP (1)              */
    int    datacopy_mode;   /* datacopy*: 0 upload and download at once (gab_datatransfer_round_trip)
                               | 1 H2D -> kernel -> D2H one after the other (the reference's schedule) */
    int    conv_scheme;     /* Conv1D_accel: 0 gab_conv_create's routing (default) | 2 the fdl scheme
                               (gab_conv_create_scheme; not with conv_mode 2, the round trip)          */
} gab_bench_config;

typedef struct {
    int    iterations;
    float  mean_ms, median_ms, std_dev_ms, min_ms, max_ms, p95_ms, p99_ms;
    float  gpu_median_ms;                    /* 0 when the benchmark records none */
    double throughput_gbps, samples_per_sec; /* cuda/bench_base.cu:110-115     */
    size_t bytes_processed;
} gab_bench_result;

typedef struct {
    int   status;            /* 0 SUCCESS, 1 FAILURE, -1 FATAL (bench_base.cuh:36-40) */
    float max_error, mean_error;
} gab_bench_validation;

void gab_bench_default_config(gab_bench_config* cfg);
int  gab_bench_count(void);
const char* gab_bench_name(int index);                 /* cuda/main.cu:84-100 */
int  gab_bench_create(gab_bench** b, const char* name, const gab_bench_config* cfg);
int  gab_bench_destroy(gab_bench* b);
/* Channel shard (additive; BASELINE configs[4]): the benchmark — created with n_tracks = the shard's
 * own track count — computes tracks [first_track, first_track + n_tracks) of a job of total_tracks: its inputs,
 * impulse responses, playheads and goldens are the global job's rows, so that the shards' results side by side
 * are the unsharded results bit for bit.  Before gab_bench_setup.  GAB_ERR_INVALID_ARG for benchmarks whose
 * tracks are not independent (DWG, modal, FDTD3D: replicas only).                                        */
int  gab_bench_set_shard(gab_bench* b, size_t first_track, size_t total_tracks);
/* What the last iteration left on the host: result arrays by index (0 .. count-1).  layout 0: track-major rows of
 * per_track floats (shards concatenate by rows), 1: sample-major [per_track][tracks] (shards concatenate by
 * columns).  The pointers stay valid until the next iteration / destroy.                                */
int  gab_bench_result_count(gab_bench* b);
int  gab_bench_result_array(gab_bench* b, int index, const char** name, const float** data, size_t* count,
                            int* layout, size_t* per_track);
int  gab_bench_setup(gab_bench* b);
int  gab_bench_run(gab_bench* b, int iterations, int warmup, gab_bench_result* out);
int  gab_bench_validate(gab_bench* b, gab_bench_validation* out);
/* text of the validation messages of the last gab_bench_validate, '\n'-joined */
const char* gab_bench_validation_text(gab_bench* b);
/* roofline numerator of one iteration (GPUABenchmark::algorithmicBytes)      */
int  gab_bench_algorithmic_bytes(gab_bench* b, size_t* bytes);
/* latencies of the last run (ms); returns how many were copied               */
int  gab_bench_latencies(gab_bench* b, float* out, int capacity);

/* ---- DAW-style pacing --------------------------------------------------------
 * The CUDA reference declares the knobs only (cuda/globals.cuh:27-30,
 * cuda/bench_utils.cuh:57-58,95 "--dawsim"); the scheduler is its Metal port's
 * DAWSimulator (metal-swift/MetalSwiftBench/Core/BenchmarkUtilities.swift:140-178,
 * used by Core/GPUABenchmark.swift:358-392): iteration k+1 starts no earlier
 * than t0 + (k+1)*buffer_seconds (+/- jitter).  mode: 0 spin, 1 sleep.          */
typedef struct gab_dawsim gab_dawsim;
int gab_dawsim_create(gab_dawsim** s, double buffer_seconds, int mode, double jitter_seconds);
int gab_dawsim_wait(gab_dawsim* s);
int gab_dawsim_stats(const gab_dawsim* s, unsigned long long* waits, unsigned long long* missed_slots);
int gab_dawsim_destroy(gab_dawsim* s);
/* pace every warm-up and timed iteration of gab_bench_run (enable = 0 turns it off) */
int gab_bench_set_dawsim(gab_bench* b, int enable, double buffer_seconds, int mode, double jitter_seconds);
/* leave a gab_keep_warm launch (8 workgroups; idle limit four pacing slots, at least 0.05 s) on the device for the length of every gab_bench_run and kick it after
 * every iteration: with pacing on, the device does not go idle while the loop waits for the next slot (enable = 0: off) */
int gab_bench_set_keep_warm(gab_bench* b, int enable);
/* pacing counters of the last gab_bench_run */
int gab_bench_dawsim_stats(gab_bench* b, unsigned long long* waits, unsigned long long* missed_slots);

#ifdef __cplusplus
}
#endif
#endif /* GAB_C_API_H */
