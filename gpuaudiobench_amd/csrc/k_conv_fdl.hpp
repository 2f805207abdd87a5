// k_conv_fdl.hpp — host side of the frequency-domain-delay-line convolution (k_conv_fdl.hip), for the
// conv plan of k_conv_accel.hip.  Internal: the C ABI is gab_conv_create_scheme(..., GAB_CONV_SCHEME_FDL).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace gab {
namespace fdl {

struct Plan;

// The shapes the scheme takes: bufsize a power of two in [128, 2048], tracks >= 1, 1 <= ir_len <= 2^21.
bool shape_ok(int tracks, int bufsize, int ir_len);
// Allocates every buffer (zeroed history); throws std::runtime_error on a runtime failure, leaking nothing.
Plan* create(int tracks, int bufsize, int ir_len);
void destroy(Plan* f);                                   // (null is fine; the caller has synchronised the device)
// d_ir: tracks x ir_len floats on the device.  One launch; the caller synchronises.
void set_ir(Plan* f, const float* d_ir, hipStream_t s);
void reset(Plan* f, hipStream_t s);
// One buffer: in [T][B], out [B][T] (sample-major).  Stateless: zero history, the delay line untouched.
void process(Plan* f, const float* in, float* out, bool streaming, hipStream_t s);
// n consecutive buffers (in [n][T][B], out [n][B][T]): the same bits as n process() calls.
void process_batch(Plan* f, const float* in, float* out, int n, hipStream_t s);
// spectra: the taps' spectra; history: the delay line and one previous block.  Not counted: the partial sums
// (kChunk planes, times the group count where the groups are spread over threads), a stateless call's spectrum and the
// second previous block — at 128 channels x 480 000 taps about 0.25 GB beside the 1 GB counted.
void state_bytes(const Plan* f, size_t* spectra, size_t* history);

}  // namespace fdl
}  // namespace gab
