// csrc/delta_e_common.h -- what the colour difference kernels share (delta_e.hip: dE00 per pixel; scielab.hip: dE00 after the S-CIELAB
// filters; receptor.hip: the receptor-noise-limited distance per pixel, which takes the record and the map's colours), in one copy so
// that they cannot drift apart: the Lab transfer function, CIEDE2000, the choice between the palette and the dim grey of a map pixel,
// the key of the largest dE, a workgroup's share of a record and the kernel that finishes the records.
// The two roundings of the map's quantiser (__fmul_rn, __fadd_rn) are spelled out next to the pixel they apply to: in delta_e_walk.h
// (the chunk walk of delta_e.hip and receptor.hip) and in scielab.hip.
#pragma once
#include "lab_tables.h"
#include "map_common.h"
#include "ssim_window.h"

namespace {

constexpr float kPi = 3.14159265358979f, kTwoPi = 6.28318530717959f;

// the sRGB -> XYZ (D65) matrix and the sums of its rows (the white point)
constexpr double kM[3][3] = {{0.4124564, 0.3575761, 0.1804375}, {0.2126729, 0.7151522, 0.0721750}, {0.0193339, 0.1191920, 0.9503041}};
constexpr double kSX = 0.4124564 + 0.3575761 + 0.1804375, kSY = 0.2126729 + 0.7151522 + 0.0721750, kSZ = 0.0193339 + 0.1191920 + 0.9503041;
constexpr float kLabEps = (float)(216.0 / 24389.0);      // (6/29)^3
constexpr float kLabSlope = (float)(841.0 / 108.0);      // 1 / (3 (6/29)^2)
constexpr float kLabOffset = (float)(4.0 / 29.0);
constexpr float k25p7 = 6103515625.0f;                   // 25^7

// one rounding each, 1 ulp: v_sqrt_f32, v_rcp_f32
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fdiv(float x, float y) { return x * __builtin_amdgcn_rcpf(y); }

// the linear branch also takes a negative t (scielab.hip: the filters leave some on saturated noise)
__device__ __forceinline__ float lab_f(float t) { return t > kLabEps ? cbrtf(t) : t * kLabSlope + kLabOffset; }

// h' in [0, 2 pi], 0 where the chroma is 0
__device__ __forceinline__ float hue_of(float b, float ap, float cp) {
    float h = atan2f(b, ap);
    h = h < 0.0f ? h + kTwoPi : h;
    return cp == 0.0f ? 0.0f : h;
}

__device__ __forceinline__ float pow7(float c) {
    const float c2 = c * c, c4 = c2 * c2;
    return (c4 * c2) * c;
}

// Sharma, Wu, Dalal 2005, k_L = k_C = k_H = 1; hue in radians
__device__ __forceinline__ float ciede2000(float L1, float a1, float b1, float L2, float a2, float b2) {
    const float C1 = fsqrt(a1 * a1 + b1 * b1), C2 = fsqrt(a2 * a2 + b2 * b2);
    const float cb7 = pow7(0.5f * (C1 + C2));
    const float G1 = 1.0f + 0.5f * (1.0f - fsqrt(fdiv(cb7, cb7 + k25p7)));
    const float a1p = G1 * a1, a2p = G1 * a2;
    const float C1p = fsqrt(a1p * a1p + b1 * b1), C2p = fsqrt(a2p * a2p + b2 * b2);
    const float h1 = hue_of(b1, a1p, C1p), h2 = hue_of(b2, a2p, C2p);
    const float dL = L2 - L1, dC = C2p - C1p, CC = C1p * C2p;
    float dh = h2 - h1, hb = h1 + h2;
    if (CC == 0.0f) {
        dh = 0.0f;
    } else if (fabsf(dh) <= kPi) {
        hb = 0.5f * hb;
    } else {
        hb = hb < kTwoPi ? 0.5f * (hb + kTwoPi) : 0.5f * (hb - kTwoPi);
        dh = dh > 0.0f ? dh - kTwoPi : dh + kTwoPi;
    }
    const float dH = 2.0f * fsqrt(CC) * sinf(0.5f * dh);
    const float Lb = 0.5f * (L1 + L2), Cb = 0.5f * (C1p + C2p);
    // cos(hb - 30), cos(2 hb), cos(3 hb + 6), cos(4 hb - 63) (degrees) from sin and cos of hb
    float s1, c1;
    sincosf(hb, &s1, &c1);
    const float c2 = 2.0f * c1 * c1 - 1.0f, s2 = 2.0f * s1 * c1;
    const float c3 = c2 * c1 - s2 * s1, s3 = s2 * c1 + c2 * s1;
    const float c4 = 2.0f * c2 * c2 - 1.0f, s4 = 2.0f * s2 * c2;
    const float T = (((1.0f - 0.17f * (c1 * 0.866025403784439f + s1 * 0.5f)) + 0.24f * c2) + 0.32f * (c3 * 0.994521895368273f - s3 * 0.104528463267653f)) -
                    0.20f * (c4 * 0.453990499739547f + s4 * 0.891006524188368f);
    const float u = (hb - 4.79965544298441f) * 2.29183118052329f;  // (hb - 275 deg) / 25 deg
    const float two_dtheta = 1.04719755119660f * expf(-(u * u));   // 2 * 30 deg * exp(.)
    const float cp7 = pow7(Cb);
    const float RC = 2.0f * fsqrt(fdiv(cp7, cp7 + k25p7));
    const float lm2 = (Lb - 50.0f) * (Lb - 50.0f);
    const float SL = 1.0f + fdiv(0.015f * lm2, fsqrt(20.0f + lm2));
    const float SC = 1.0f + 0.045f * Cb, SH = 1.0f + 0.015f * Cb * T;
    const float RT = -sinf(two_dtheta) * RC;
    const float tL = fdiv(dL, SL), tC = fdiv(dC, SC), tH = fdiv(dH, SH);
    const float rad = ((tL * tL + tC * tC) + tH * tH) + RT * (tC * tH);
    return fsqrt(fmaxf(rad, 0.0f));
}

// The key of a pixel's dE in the 64-bit integer maximum of a frame: (float bits of dE << 32) | (0xFFFFFFFF - pixel index).  dE is never
// negative, so its bits order as its value, and among equals the earlier pixel wins.
__device__ __forceinline__ unsigned long long de_key(float de, uint32_t index) {
    return ((unsigned long long)__float_as_uint(de) << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}

// The map's colour of a pixel whose quantised value is v: the palette, or in the heat mode within the threshold the dim grey of A's pixel
__device__ __forceinline__ void de_colour(float v, float de, float T, int mode, int ar, int ag, int ab, uint32_t& r, uint32_t& g, uint32_t& b) {
    pal((int)fmaxf(v, 0.0f), r, g, b);
    if (mode == AVX_DELTA_E_HEAT && !(de > T)) r = g = b = dim_grey(ar, ag, ab);
}

// A workgroup's share of a frame's record, called by all kThreads threads: `sum` (the thread's pixels in float64), `key`, `beyond` and
// `zeros` (the thread's pixels of bin 0, which are not in hist) are the thread's own; hist is the workgroup's LDS histogram of the other
// bins.  The sum goes to *partial in ssim_window.h's fixed order, everything else into the record with integer atomics; the key lies in
// the bytes of (max_de, max_x) until k_delta_e_final takes it apart.  red, wred and bred hold kThreads / 64 entries each.
__device__ __forceinline__ void de_record_share(double sum, unsigned long long key, unsigned beyond, unsigned zeros, unsigned* hist, double* red,
                                                unsigned long long* wred, unsigned* bred, double* partial, avx_delta_e_rec* rec) {
    const int tid = threadIdx.x;
    zeros = wave_sum_u32(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&hist[0], zeros);
    double s[1] = {sum};
    workgroup_sum(s, red);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_down(key, o);
        key = k > key ? k : key;
        beyond += __shfl_down(beyond, o);
    }
    if ((tid & 63) == 0) wred[tid >> 6] = key, bred[tid >> 6] = beyond;
    __syncthreads();
    if (tid == 0) {
        *partial = s[0];
        unsigned long long k = wred[0];
        unsigned n = bred[0];
        for (int w = 1; w < kThreads / 64; ++w) k = wred[w] > k ? wred[w] : k, n += bred[w];
        if (k >> 32) atomicMax(reinterpret_cast<unsigned long long*>(&rec->max_de), k);  // dE == 0 everywhere leaves the zeroed record
        if (n) atomicAdd(&rec->beyond, n);
    }
    hist_flush(hist, 256, rec->hist);
}

// grid (frames): the frame's partials in index order -> sum; the key in the bytes of (max_de, max_x) -> (max_de, max_x, max_y)
__global__ __launch_bounds__(kThreads) void k_delta_e_final(const double* __restrict__ partials, size_t nchunks, int W, avx_delta_e_rec* __restrict__ rec) {
    __shared__ double red[kThreads];
    const int f = blockIdx.x;
    const double s = tile_partials_sum(partials + (size_t)f * nchunks, nchunks, red);
    if (threadIdx.x == 0) {
        const unsigned long long key = *reinterpret_cast<const unsigned long long*>(&rec[f].max_de);
        const uint32_t bits = (uint32_t)(key >> 32), index = 0xFFFFFFFFu - (uint32_t)key;
        rec[f].sum = s;
        rec[f].max_de = __uint_as_float(bits);
        rec[f].max_x = bits ? index % (uint32_t)W : 0u;
        rec[f].max_y = bits ? index / (uint32_t)W : 0u;
    }
}

static_assert(sizeof(avx_delta_e_rec) == 1048 && offsetof(avx_delta_e_rec, max_de) == 1032, "avx_delta_e_rec: the key needs 8 aligned bytes at max_de");

}  // namespace
