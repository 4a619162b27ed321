// csrc/ssim_window.h -- the 11 x 11 Gaussian-window SSIM tile scheme (Wang et al. 2004: sigma 1.5, valid positions), shared by
// metrics.hip (k_metrics_tile: RGB bytes, float32), plane_metrics.hip (k_plane_tile: YUV planes, float32 at 8 bits, float64 at 10)
// and ms_ssim.hip (k_ms_levels: scales 1..4, float64) so that the three compile one copy.  That is what their promises rest on: a
// frame's record does not depend on the batch it was in, and scale 0 of MS-SSIM is bit-equal to the plain SSIM record, because
// every kernel forms its sums by the same operations in the same order (nothing is contracted: -ffp-contract=off).
//
// One workgroup of kThreads owns a kT x kT tile of window positions.  The kP x kP patch of both sides goes into LDS once, in the
// file's own layout.  The row pass writes the five moment planes a, b, a^2, b^2, ab of centred samples (kP x kT values of the moment
// type M each) into LDS: hp[plane][row][x].  The column pass keeps its 4 x 5 window sums in registers, and the file forms its own
// term of each position from them.  The positions are summed in float64 in a fixed order: a workgroup reduces its own to one double
// per sum, and the file's *_final kernel adds the tiles of a record entry with tile_partials_sum: no floating-point atomics.
// What differs between the files stays in them: how a patch gets into LDS and its samples from there into registers, the histogram
// of each layout, and the arithmetic of a position.  diff_map.hip (k_diff_ssim_tile: the SSIM of every position as a picture) runs
// the passes on metrics.hip's RGB byte patches and keeps the positions instead of summing them; what those two share beyond the
// passes -- the row item of a byte patch and the float32 arithmetic of a position -- is here too, in one copy.
#pragma once
#include <cmath>
#include <type_traits>

#include "avx_internal.h"

namespace {

constexpr int kT = 32;                 // tile: kT x kT window positions
constexpr int kK = 11;                 // window
constexpr int kP = kT + kK - 1;        // patch side: 42
constexpr int kThreads = 256;

// tiles along a side of n >= kK samples
inline unsigned ssim_tiles(int n) { return (unsigned)((n - (kK - 1) + kT - 1) / kT); }

template <typename M>
struct Taps { M w[kK]; };

// the window, normalised in float64; a float32 kernel rounds each tap once
inline void ssim_window_taps(double (&w)[kK]) {
    double g[kK], sum = 0.0;
    for (int k = 0; k < kK; ++k) sum += g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < kK; ++k) w[k] = g[k] / sum;
}

__device__ __forceinline__ float fma_m(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_m(double a, double b, double c) { return __builtin_fma(a, b, c); }

// Row pass of NOUT adjacent positions of patch row `row`, from column x on: a and b are the NOUT + 10 centred samples of both sides;
// their products are formed once, the five moment sums go to hp[plane][row][x ...] (x a multiple of NOUT: the float32 runs are one
// aligned store each).
template <typename M, int NOUT>
__device__ __forceinline__ void row_moments(const M (&a)[NOUT + kK - 1], const M (&b)[NOUT + kK - 1], const Taps<M>& tp, M* hp, int row, int x) {
    M m[5][NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        m[0][o] = tp.w[0] * a[o];
        m[1][o] = tp.w[0] * b[o];
        m[2][o] = tp.w[0] * (a[o] * a[o]);
        m[3][o] = tp.w[0] * (b[o] * b[o]);
        m[4][o] = tp.w[0] * (a[o] * b[o]);
#pragma unroll
        for (int k = 1; k < kK; ++k) {
            const M u = a[o + k], v = b[o + k];
            m[0][o] = fma_m(tp.w[k], u, m[0][o]);
            m[1][o] = fma_m(tp.w[k], v, m[1][o]);
            m[2][o] = fma_m(tp.w[k], u * u, m[2][o]);
            m[3][o] = fma_m(tp.w[k], v * v, m[3][o]);
            m[4][o] = fma_m(tp.w[k], u * v, m[4][o]);
        }
    }
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        M* dst = hp + (p * kP + row) * kT + x;
        if constexpr (std::is_same<M, float>::value && NOUT == 4) {
            *reinterpret_cast<float4*>(dst) = make_float4(m[p][0], m[p][1], m[p][2], m[p][3]);
        } else if constexpr (std::is_same<M, float>::value && NOUT == 2) {
            *reinterpret_cast<float2*>(dst) = make_float2(m[p][0], m[p][1]);
        } else {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) dst[o] = m[p][o];
        }
    }
}

// The row pass's schedule: the first kT patch rows as 256 items of 4 positions, the other 10 as 160 items of 2, so every wave stays
// busy.  item(n, row, x) is the file's own row item of decltype(n)::value positions.
template <typename F>
__device__ __forceinline__ void row_pass(F&& item) {
    const int tid = threadIdx.x;
    item(std::integral_constant<int, 4>{}, tid >> 3, (tid & 7) * 4);
    if (tid < (kP - kT) * (kT / 2)) item(std::integral_constant<int, 2>{}, kT + (tid >> 4), (tid & 15) * 2);
}

// Column pass: the window sums of the five planes at the thread's 4 positions, rows seg * 4 ... + 3 of column col
template <typename M>
__device__ __forceinline__ void column_pass(const M* hp, const Taps<M>& tp, int col, int seg, M (&acc)[5][4]) {
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        M v[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) v[k] = hp[(p * kP + seg * 4 + k) * kT + col];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            M s = tp.w[0] * v[o];
#pragma unroll
            for (int k = 1; k < kK; ++k) s = fma_m(tp.w[k], v[o + k], s);
            acc[p][o] = s;
        }
    }
}

// ---- uint8 RGB frames in float32: what metrics.hip (the record) and diff_map.hip (the map) share beyond the passes ----
constexpr int kRaw = kP * 3 + 6;       // bytes of a patch row in LDS (132: rows land one bank apart)

// Row item of NOUT adjacent positions of patch row `row`, from column x on, for channel C: the NOUT + 10 samples of both frames,
// centred by 128.  NOUT == 4 (x a multiple of 4) reads the bytes as the 11 aligned words that hold them, NOUT == 2 byte by byte.
template <int NOUT, int C>
__device__ __forceinline__ void rgb_row_item(const uint8_t* raw_a, const uint8_t* raw_b, float* hp, const Taps<float>& tp, int row, int x) {
    constexpr int NS = NOUT + kK - 1;
    float a[NS], b[NS];
    if (NOUT == 4) {
        const uint32_t* wa = reinterpret_cast<const uint32_t*>(raw_a + row * kRaw + x * 3);
        const uint32_t* wb = reinterpret_cast<const uint32_t*>(raw_b + row * kRaw + x * 3);
        uint32_t va[11], vb[11];
#pragma unroll
        for (int i = 0; i < 11; ++i) va[i] = wa[i], vb[i] = wb[i];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int byte = 3 * j + C;
            a[j] = (float)((va[byte >> 2] >> (8 * (byte & 3))) & 255u) - 128.0f;
            b[j] = (float)((vb[byte >> 2] >> (8 * (byte & 3))) & 255u) - 128.0f;
        }
    } else {
        const uint8_t* ra = raw_a + row * kRaw + x * 3 + C;
        const uint8_t* rb = raw_b + row * kRaw + x * 3 + C;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            a[j] = (float)ra[3 * j] - 128.0f;
            b[j] = (float)rb[3 * j] - 128.0f;
        }
    }
    row_moments<float, NOUT>(a, b, tp, hp, row, x);
}

// The SSIM of one position of uint8 RGB frames in float32 (metrics.hip: the record; diff_map.hip: the map), from its five window sums
// of samples centred by 128: ma, mb the means, eaa, ebb, eab the second moments.  E[x^2] - mu^2 loses nothing to float32: the rounding
// error of the product is recovered with an fma and taken off the difference, so variance and covariance carry a relative error of
// 2^-23, not one of the size of mu^2.  WITH_CS: *cs receives the contrast-structure term (2 s_ab + C2) / (s_a^2 + s_b^2 + C2).
template <bool WITH_CS>
__device__ __forceinline__ float ssim_position_f32(float ma, float mb, float eaa, float ebb, float eab, float* cs) {
    const float C1 = 6.5025f, C2 = 58.5225f;  // (0.01 * 255)^2, (0.03 * 255)^2
    const float paa = ma * ma, pbb = mb * mb, pab = ma * mb;
    const float va = (eaa - paa) - fmaf(ma, ma, -paa);
    const float vb = (ebb - pbb) - fmaf(mb, mb, -pbb);
    const float cab = (eab - pab) - fmaf(ma, mb, -pab);
    const float ua = ma + 128.0f, ub = mb + 128.0f;
    const float num = (2.0f * (ua * ub) + C1) * (2.0f * cab + C2);
    const float den = ((ua * ua + ub * ub) + C1) * ((va + vb) + C2);
    if constexpr (WITH_CS) *cs = (2.0f * cab + C2) / ((va + vb) + C2);
    return num / den;
}

// The workgroup's sums of N doubles per thread, in a fixed order: a __shfl_down tree per wave, then the four waves in order.  Every
// thread gets them; red holds N * (kThreads / 64) doubles.  Its barrier is also behind every LDS access of the passes before it.
template <int N>
__device__ __forceinline__ void workgroup_sum(double (&s)[N], double* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_down(s[i], o);
        if ((tid & 63) == 0) red[i * (kThreads / 64) + (tid >> 6)] = s[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double* r = red + i * (kThreads / 64);
        s[i] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

// The sum of n tile partials in a fixed order: thread t adds p[t], p[t + 256], ..., then a fixed tree over red[kThreads].  Called by
// every thread of the workgroup; the sum is thread 0's.
__device__ __forceinline__ double tile_partials_sum(const double* p, size_t n, double* red) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (size_t t = tid; t < n; t += kThreads) s += p[t];
    red[tid] = s;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// the workgroup's LDS histogram into a record's: one global atomic per non-empty bin (integers: order does not matter)
__device__ __forceinline__ void hist_flush(const unsigned* hist, int bins, unsigned* dst) {
    for (int i = threadIdx.x; i < bins; i += kThreads) {
        const unsigned v = hist[i];
        if (v) atomicAdd(dst + i, v);
    }
}

}  // namespace
