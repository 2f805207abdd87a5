// gab_stft.hpp — the two default windows of the short-time Fourier plans (spectrum, resynthesis, denoise), made on the
// host: one copy, so the three plans hold the same bits.
#pragma once

#include <cmath>
#include <vector>

namespace gab {

constexpr int kStftN = 1024;                              // the transform of the three plans

// The periodic Hann window 0.5 - 0.5 cos(2 pi n / N): float64, rounded once.
inline std::vector<float> stft_hann() {
    const double pi = 3.14159265358979323846;
    std::vector<float> w((size_t)kStftN);
    for (int n = 0; n < kStftN; ++n) w[(size_t)n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)n / (double)kStftN));
    return w;
}

// S: the float64 sum of the float32 values, added in ascending n.
inline double stft_window_sum(const std::vector<float>& w) {
    double S = 0.0;
    for (int n = 0; n < kStftN; ++n) S += (double)w[(size_t)n];
    return S;
}

// The least-squares dual of stft_hann() at hop H: g[n] = w[n] / sum_m w[n + m H]^2, m over every index inside 0..1023 in
// ascending order, 0 where the sum is 0: float64 on the float32 values of w, rounded once.
inline std::vector<float> stft_hann_dual(int H) {
    const std::vector<float> wf = stft_hann();
    std::vector<double> w((size_t)kStftN);
    for (int n = 0; n < kStftN; ++n) w[(size_t)n] = (double)wf[(size_t)n];
    std::vector<float> g((size_t)kStftN);
    for (int n = 0; n < kStftN; ++n) {
        double s = 0.0;
        for (int i = n % H; i < kStftN; i += H) s += w[(size_t)i] * w[(size_t)i];
        g[(size_t)n] = s == 0.0 ? 0.0f : (float)(w[(size_t)n] / s);
    }
    return g;
}

}  // namespace gab
