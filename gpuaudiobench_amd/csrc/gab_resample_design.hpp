// gab_resample_design.hpp — the tap table of a polyphase resampler by L / M (include/gab_c_api.h, gab_resample_*,
// "taps"): the one copy that the resample plan and the saturator plan's two stages both call, so that the saturator's
// tables are the resampler's bit for bit.  Host arithmetic.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace gab {

// The header's taps: float64, each phase divided by its sum (added in ascending j), rounded once.
inline std::vector<float> resample_design(int L, int M, int K) {
    const double pi = 3.14159265358979323846;
    const double ratio = (double)L / (double)M;
    const double c = 0.94 * (ratio < 1.0 ? ratio : 1.0);
    const double half = (double)(K / 2);
    std::vector<float> taps((size_t)L * K);
    std::vector<double> h((size_t)K);
    for (int p = 0; p < L; ++p) {
        double sum = 0.0;
        for (int j = 0; j < K; ++j) {
            const double d = (double)(j - K / 2) + (double)p / (double)L;
            const double u = d / half;
            const double x = c * d;
            const double s = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
            const double wnd = 0.35875 + 0.48829 * std::cos(pi * u) + 0.14128 * std::cos(2.0 * pi * u) +
                               0.01168 * std::cos(3.0 * pi * u);
            h[(size_t)j] = s * wnd;
            sum += h[(size_t)j];
        }
        for (int j = 0; j < K; ++j) taps[(size_t)p * K + j] = (float)(h[(size_t)j] / sum);
    }
    return taps;
}

}  // namespace gab
