// csrc/receptor.hip -- receptor-noise-limited colour distance maps on the device (Vorobyev & Osorio 1998; the definition
// is include/avx.h's): per pixel of two uint8 sRGB batches the distance dS, in just-noticeable differences, between the two colours as
// an observer with K = 2, 3 or 4 receptor classes tells them apart -- as a float32 plane, as a picture and as a record per frame,
// which are avx_delta_e_u8's in every respect but the value.
//
// k_receptor<K>: the chunk walk, the map and the record are delta_e_walk.h's one copy, shared with delta_e.hip; the value of a pixel is
// this file's: the K catches of both pixels (the decode table in LDS, the anchored matrix form: a grey has every catch equal to g), K
// divisions and K logf for the contrasts, and the quadratic form of their differences.  The observer's constants -- the normalised
// matrix, the weights of the pairs and the reciprocal of the denominator, formed on the host in double and rounded once -- are kernel
// arguments; the kernel is instantiated on K so that the loops over classes and pairs unroll.
#include "delta_e_common.h"
#include "delta_e_walk.h"

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

// dS of two pixels whose codes differ
template <int K>
struct Rnl {
    RnlArgs c;
    __device__ __forceinline__ float operator()(const float* lut, int ar, int ag, int ab, int br, int bg, int bb) const {
        const float r1 = lut[ar], g1 = lut[ag], b1 = lut[ab], r2 = lut[br], g2 = lut[bg], b2 = lut[bb];
        const float dr1 = r1 - g1, db1 = b1 - g1, dr2 = r2 - g2, db2 = b2 - g2;
        float df[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float qa = (g1 + c.r0[i] * dr1) + c.r2[i] * db1;
            const float qb = (g2 + c.r0[i] * dr2) + c.r2[i] * db2;
            df[i] = logf((qa + c.eps) / (qb + c.eps));
        }
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
};

template <int K, bool VEC>
__global__ __launch_bounds__(kThreads) void k_receptor(DeArgs p, RnlArgs c) {
    de_chunk_walk<VEC>(p, Rnl<K>{c});
}

template <int K>
void launch_receptor(bool vec, dim3 grid, hipStream_t s, const DeArgs& p, const RnlArgs& c) {
    if (vec) hipLaunchKernelGGL((k_receptor<K, true>), grid, dim3(kThreads), 0, s, p, c);
    else hipLaunchKernelGGL((k_receptor<K, false>), grid, dim3(kThreads), 0, s, p, c);
}

}  // namespace

extern "C" int avx_receptor_delta_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                     int mode, float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out,
                                     void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = de_walk_check(ctx, "avx_receptor_delta_u8", a_hwc, b_hwc, n_frames, H, W, mode, gain, threshold, layout, map_out, rec_dev, ds_out);
    if (rc) return rc;
    AVX_REQUIRE(ctx, obs && obs->struct_size == sizeof(avx_receptor_desc), "avx_receptor_delta_u8: obs is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    const int K = obs->n_receptors;
    AVX_REQUIRE(ctx, K >= 2 && K <= kMaxK, "avx_receptor_delta_u8: n_receptors must be 2..4 (got %d)", K);
    AVX_REQUIRE(ctx, obs->floor >= 1e-6 && obs->floor <= 0.1, "avx_receptor_delta_u8: the floor must be from 1e-6 to 0.1 (got %g)", obs->floor);

    // ---- the constants: float64 on the host, rounded once ----
    RnlArgs c = {};
    double e2[kMaxK];
    for (int i = 0; i < K; ++i) {
        const double* row = obs->matrix + 3 * i;
        AVX_REQUIRE(ctx, std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]) && row[0] >= 0.0 && row[1] >= 0.0 && row[2] >= 0.0,
                    "avx_receptor_delta_u8: matrix row %d must be finite and not negative (got %g %g %g)", i, row[0], row[1], row[2]);
        const double sum = row[0] + row[1] + row[2];
        AVX_REQUIRE(ctx, sum > 0.0 && std::isfinite(sum), "avx_receptor_delta_u8: matrix row %d sums to %g, it must be above 0 and finite", i, sum);
        AVX_REQUIRE(ctx, obs->weber[i] >= 0.01 && obs->weber[i] <= 1.0, "avx_receptor_delta_u8: Weber fraction %d must be from 0.01 to 1 (got %g)", i,
                    obs->weber[i]);
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

    return de_walk_launch(ctx, a_hwc, b_hwc, n_frames, H, W, mode, gain, threshold, layout, map_out, rec_dev, ds_out, stream,
                          [&](bool vec, dim3 grid, hipStream_t s, const DeArgs& p) {
                              if (K == 2) launch_receptor<2>(vec, grid, s, p, c);
                              else if (K == 3) launch_receptor<3>(vec, grid, s, p, c);
                              else launch_receptor<4>(vec, grid, s, p, c);
                          });
}
