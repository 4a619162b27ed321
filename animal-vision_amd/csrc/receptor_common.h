// csrc/receptor_common.h -- what the receptor-noise-limited distance kernels share (receptor.hip: dS per pixel; receptor_acuity.hip: dS
// behind the observer's acuity blur; receptor_edges.hip: dS between a pixel and its neighbours within one frame), in one copy so that
// they cannot drift apart: the pairs of classes, the observer's constants as the kernels take them, the catch of a class, the value of
// two pixels from their six linear values or from their K contrasts, and the host's checks of an avx_receptor_desc with the constants it
// yields.  The definition is include/avx.h's, above avx_receptor_delta_u8.
#pragma once
#include <cmath>

#include "avx_internal.h"

namespace {

constexpr int kMaxK = 4, kMaxPairs = 6;

// the pairs of classes in the order of the definition's numerator, zero-based: pair j of K classes is (pair_class(K, j, 0),
// pair_class(K, j, 1)), and K classes have pair_count(K) of them
__host__ __device__ constexpr int pair_count(int K) { return K * (K - 1) / 2; }
__host__ __device__ constexpr int pair_class(int K, int j, int which) {
    constexpr int p3[3][2] = {{2, 1}, {2, 0}, {1, 0}};
    constexpr int p4[6][2] = {{3, 2}, {3, 1}, {2, 1}, {3, 0}, {2, 0}, {1, 0}};
    return K == 2 ? which : K == 3 ? p3[j][which] : p4[j][which];
}

struct RnlArgs {
    float r0[kMaxK], r2[kMaxK];  // R': columns 0 and 2 of the normalised matrix, the anchored form needs no other
    float w[kMaxPairs];          // the weight of a pair: the product of e_k^2 over the classes k outside it
    float eps;
    float rcp;                   // K = 2: 1 / sqrt(e_1^2 + e_2^2); else 1 / the denominator
};

// the catch of a class in the anchored form, from the row's columns 0 and 2 and the pixel's g, r - g and b - g: a grey gives g exactly
__device__ __forceinline__ float rnl_catch(float r0, float r2, float g, float dr, float db) { return (g + r0 * dr) + r2 * db; }

template <int K>
struct Rnl {
    RnlArgs c;
    // dS of two pixels from their linear values
    __device__ __forceinline__ float value(float r1, float g1, float b1, float r2, float g2, float b2) const {
        const float dr1 = r1 - g1, db1 = b1 - g1, dr2 = r2 - g2, db2 = b2 - g2;
        float df[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float qa = rnl_catch(c.r0[i], c.r2[i], g1, dr1, db1);
            const float qb = rnl_catch(c.r0[i], c.r2[i], g2, dr2, db2);
            df[i] = logf((qa + c.eps) / (qb + c.eps));
        }
        return from_contrasts(df);
    }
    // dS from the K contrasts df_i of two pixels: the quadratic form, in one copy (receptor_edges.hip forms its df_i as differences of
    // log-catches and comes here too)
    __device__ __forceinline__ float from_contrasts(const float (&df)[K]) const {
        if (K == 2) return fabsf(df[0] - df[1]) * c.rcp;
        float num = 0.0f;
#pragma unroll
        for (int j = 0; j < pair_count(K); ++j) {
            const float d = df[pair_class(K, j, 0)] - df[pair_class(K, j, 1)];
            const float t = c.w[j] * (d * d);
            num = j == 0 ? t : num + t;
        }
        return sqrtf(num * c.rcp);
    }
    // dS of two pixels whose codes differ: the table lookup, then the value
    __device__ __forceinline__ float operator()(const float* lut, int ar, int ag, int ab, int br, int bg, int bb) const {
        return value(lut[ar], lut[ag], lut[ab], lut[br], lut[bg], lut[bb]);
    }
};

// The host's checks of an observer (`fn` is the entry's name, for the messages) and its constants: float64 on the host, rounded once
inline int rnl_constants(avx_ctx* ctx, const char* fn, const avx_receptor_desc* obs, RnlArgs& c, int& K) {
    AVX_REQUIRE(ctx, obs && obs->struct_size == sizeof(avx_receptor_desc), "%s: obs is NULL or struct_size mismatch (ABI %d)", fn, AVX_ABI_VERSION);
    K = obs->n_receptors;
    AVX_REQUIRE(ctx, K >= 2 && K <= kMaxK, "%s: n_receptors must be 2..4 (got %d)", fn, K);
    AVX_REQUIRE(ctx, obs->floor >= 1e-6 && obs->floor <= 0.1, "%s: the floor must be from 1e-6 to 0.1 (got %g)", fn, obs->floor);
    c = {};
    double e2[kMaxK];
    for (int i = 0; i < K; ++i) {
        const double* row = obs->matrix + 3 * i;
        AVX_REQUIRE(ctx, std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]) && row[0] >= 0.0 && row[1] >= 0.0 && row[2] >= 0.0,
                    "%s: matrix row %d must be finite and not negative (got %g %g %g)", fn, i, row[0], row[1], row[2]);
        const double sum = row[0] + row[1] + row[2];
        AVX_REQUIRE(ctx, sum > 0.0 && std::isfinite(sum), "%s: matrix row %d sums to %g, it must be above 0 and finite", fn, i, sum);
        AVX_REQUIRE(ctx, obs->weber[i] >= 0.01 && obs->weber[i] <= 1.0, "%s: Weber fraction %d must be from 0.01 to 1 (got %g)", fn, i, obs->weber[i]);
        c.r0[i] = (float)(row[0] / sum), c.r2[i] = (float)(row[2] / sum);
        e2[i] = obs->weber[i] * obs->weber[i];
    }
    // the weight of a pair is the product of e_k^2 over the classes outside it; the denominator sums the products that leave one class out
    for (int j = 0; j < pair_count(K); ++j) {
        double w = 1.0;
        for (int k = 0; k < K; ++k) w *= k == pair_class(K, j, 0) || k == pair_class(K, j, 1) ? 1.0 : e2[k];
        c.w[j] = (float)w;
    }
    double den = 0.0;
    for (int out = K - 1; out >= 0; --out) {
        double t = 1.0;
        for (int k = 0; k < K; ++k) t *= k == out ? 1.0 : e2[k];
        den += t;
    }
    c.eps = (float)obs->floor;
    c.rcp = (float)(K == 2 ? 1.0 / sqrt(den) : 1.0 / den);
    return AVX_OK;
}

}  // namespace
