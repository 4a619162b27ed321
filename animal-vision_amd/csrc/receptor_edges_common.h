// csrc/receptor_edges_common.h -- what the two edges entries share (receptor_edges.hip: the fused kernel; receptor_smooth.hip: the planes
// route with the edge-preserving smoothing in front of the edges), in one copy: the block geometry and the slots of the
// taps, the luminance channel as the kernels take it, the reflection, the blur's LDS, and the host's checks of (lum, channel, sigma,
// step) with the taps they yield.  No kernel code beyond fold101: the blur passes stay a copy per kernel (receptor_edges.hip says why).
#pragma once
#include <cmath>

#include "delta_e_common.h"
#include "receptor_common.h"

namespace {

constexpr int kBlockW = 64, kBlockH = 32, kPer = 8;  // a thread: column tid & 63, rows (tid >> 6) * 8 ...
constexpr int kMaxRad = (AVX_MAX_KSIZE - 1) / 2;     // 16
constexpr int kTapFront = 3;                         // zero taps in front of t_0
constexpr int kTapSlots = 40;                        // 3 + 33 taps, and the zeros the last group of four reads
constexpr int kPadRows = 4;                          // zero rows below the row-pass result, for the last group of the column pass
constexpr int kMaxStep = 8;
constexpr int kPlane = kBlockW * kBlockH;            // floats of a plane of log-catches
static_assert(kBlockW * kBlockH == kThreads * kPer && kBlockW == 64 && kThreads == 256, "block geometry");
static_assert(4 * ((2 * kMaxRad + 3) / 4) + 6 < kTapSlots && kTapFront + 4 * ((2 * kMaxRad + 4) / 4) - 1 < kTapSlots, "tap slots");
static_assert(kPadRows * kBlockW == kThreads, "one pad word a thread");
static_assert(2 * kMaxStep < kBlockH, "a block owns pixels at every step");

// the luminance channel as the kernel takes it: columns 0 and 2 of the normalised row, and 1 / e_L
struct LumArgs {
    float r0, r2, rcp;
};

// BORDER_REFLECT_101, folded as often as needed: n = 1 gives 0
__device__ __forceinline__ long long fold101(long long i, long long n) {
    if (n == 1) return 0;
    const long long p = 2 * (n - 1);
    long long m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - m;
}

// the blur's dynamic LDS in floats: the tile [rows][span], then the row-pass result [rows + kPadRows][64]
constexpr size_t blur_floats(int R) { return (size_t)(kBlockH + 2 * R) * ((kBlockW + 2 * R + 3) & ~3) + (size_t)(kBlockH + 2 * R + kPadRows) * kBlockW; }

// The host's checks of the channel, the luminance channel, sigma and step (`fn` is the entry's name, for the messages), and what they
// yield: the luminance channel's constants, the taps in their slots (tp zeroed by the caller: tp[kTapFront + k] = t_k) and the radius
inline int edges_check(avx_ctx* ctx, const char* fn, const avx_luminance_desc* lum, int channel, double sigma, int step, LumArgs& l,
                       float (&tp)[kTapSlots], int& R) {
    AVX_REQUIRE(ctx, channel == AVX_EDGES_CHROMATIC || channel == AVX_EDGES_ACHROMATIC || channel == AVX_EDGES_EITHER, "%s: bad channel %d", fn, channel);
    AVX_REQUIRE(ctx, lum || channel == AVX_EDGES_CHROMATIC, "%s: channel %d needs the luminance channel (lum is NULL)", fn, channel);
    if (lum) {
        AVX_REQUIRE(ctx, lum->struct_size == sizeof(avx_luminance_desc), "%s: lum struct_size mismatch (ABI %d)", fn, AVX_ABI_VERSION);
        const double* row = lum->row;
        AVX_REQUIRE(ctx, std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]) && row[0] >= 0.0 && row[1] >= 0.0 && row[2] >= 0.0,
                    "%s: the luminance row must be finite and not negative (got %g %g %g)", fn, row[0], row[1], row[2]);
        const double sum = row[0] + row[1] + row[2];
        AVX_REQUIRE(ctx, sum > 0.0 && std::isfinite(sum), "%s: the luminance row sums to %g, it must be above 0 and finite", fn, sum);
        AVX_REQUIRE(ctx, lum->weber >= 0.01 && lum->weber <= 1.0, "%s: the luminance Weber fraction must be from 0.01 to 1 (got %g)", fn, lum->weber);
        l = {(float)(row[0] / sum), (float)(row[2] / sum), (float)(1.0 / lum->weber)};
    }
    AVX_REQUIRE(ctx, sigma == 0.0 || (std::isfinite(sigma) && sigma >= 0.2 && sigma <= 4.0),
                "%s: sigma must be 0 (no blur) or a finite number from 0.2 to 4 (got %g)", fn, sigma);
    AVX_REQUIRE(ctx, step >= 1 && step <= kMaxStep, "%s: step must be 1..%d (got %d)", fn, kMaxStep, step);
    const int ksize = sigma == 0.0 ? 1 : (int)lrint(sigma * 8.0 + 1.0) | 1;  // cvRound: half to even
    AVX_REQUIRE(ctx, ksize >= 1 && ksize <= AVX_MAX_KSIZE, "%s: sigma %g needs %d taps, 3 .. %d are supported", fn, sigma, ksize, AVX_MAX_KSIZE);

    // ---- the taps: cv::getGaussianKernel(ksize, sigma) in double, summed left to right, rounded once; no blur is the one tap 1 ----
    if (ksize == 1) {
        tp[kTapFront] = 1.0f;
    } else {
        const double scale2x = -0.5 / (sigma * sigma), mid = (ksize - 1) * 0.5;
        double t[AVX_MAX_KSIZE], sum = 0.0;
        for (int i = 0; i < ksize; ++i) sum += t[i] = exp(scale2x * (i - mid) * (i - mid));
        const double scale = 1.0 / sum;
        for (int i = 0; i < ksize; ++i) tp[kTapFront + i] = (float)(t[i] * scale);
    }
    R = (ksize - 1) / 2;
    return AVX_OK;
}

}  // namespace
