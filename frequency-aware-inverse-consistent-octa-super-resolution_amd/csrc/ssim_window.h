// The SSIM window of ssim.py:7-13 as its 1-D taps, for ssim.hip and msssim.hip: 11 taps, sigma 1.5, by value in the kernel arguments.
#pragma once
#include <cmath>

namespace faoctasr {

constexpr int SSIM_R = 5;            // window radius
struct SsimTaps { float g[2 * SSIM_R + 1]; };

static inline SsimTaps ssim_taps() {
    // ssim.py:7-9: gauss = Tensor([exp(-(x - 5)^2 / (2 * 1.5^2))]) (fp32) / gauss.sum()
    SsimTaps t;
    float sum = 0.f;
    for (int k = 0; k < 11; ++k) {
        t.g[k] = (float)exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        sum += t.g[k];
    }
    for (int k = 0; k < 11; ++k) t.g[k] /= sum;
    return t;
}

}  // namespace faoctasr
