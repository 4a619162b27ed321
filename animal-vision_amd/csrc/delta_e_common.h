// csrc/delta_e_common.h -- what the five colour difference entries share (delta_e.hip: dE00 per pixel; scielab.hip: dE00 after the
// S-CIELAB filters; receptor.hip and receptor_acuity.hip: the receptor-noise-limited distance, per pixel and behind the acuity blur;
// itp.hip: dE_ITP), in one copy so that they cannot drift apart.  The values: the Lab transfer function and CIEDE2000.  Everything
// between a pixel's value and the outputs, which is the same whatever the value: the tail of the argument structs (DeOut), a thread's
// share of the record (DeTally) and the workgroup's (DeRecLds, de_record_share), the map's quantiser and colour (de_map_colour: its
// roundings are spelled out there and nowhere else), a pixel's panels (de_px_panels, the tile kernels), the side layout's rows of a
// chunk (de_side_rows_out, the chunk kernels) and the body of the kernel that finishes the records (de_final; the kernel itself is
// delta_e.hip's, the library's one copy).  The host side: the argument checks (de_check_options, de_check_pair) and the launch frame
// around an entry's own kernels (de_begin, de_finish).
#pragma once
#include <cmath>

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

// The fields that the argument struct of every entry's kernel ends with: where the outputs go and how the map is drawn
struct DeOut {
    uint8_t* out;      // NULL: no map
    float* de;         // NULL: no float plane
    double* partials;  // [frame][chunk or tile]
    avx_delta_e_rec* rec;
    int H, W, mode, side;
    float gain, threshold;
};

// The LDS of a workgroup's share of a record: the histogram of the bins above 0, and what de_record_share reduces through
struct DeRecLds {
    unsigned hist[256];
    double red[kThreads / 64];
    unsigned long long wred[kThreads / 64];
    unsigned bred[kThreads / 64];
};

// A thread's share of a record: the float64 sum of its pixels in the order it meets them, the key of its largest, its pixels beyond
// the threshold and its pixels of bin 0, which stay out of the LDS histogram
struct DeTally {
    double sum = 0.0;
    unsigned long long key = 0;
    unsigned beyond = 0, zeros = 0;

    // the pixel at `index` of its frame, of value de >= 0; hist: the workgroup's DeRecLds::hist
    __device__ __forceinline__ void add(float de, uint32_t index, float T, unsigned* hist) {
        const int bin = min(255, (int)(de + de));  // floor(2 dE)
        if (bin == 0) ++zeros;
        else atomicAdd(&hist[bin], 1u);
        sum += (double)de;
        beyond += de > T ? 1u : 0u;
        const unsigned long long k = de_key(de, index);
        key = k > key ? k : key;
    }
};

// The map's colour of a pixel of value de whose pixel in A is (ar, ag, ab).  The quantiser is float32 with one rounding per operation,
// multiply and add never fused: v = min(floor(G x + 0.5), 255) with x = dE - T in the heat mode and dE in the plain mode.  Then the
// palette, or in the heat mode within the threshold the dim grey of A's pixel.
__device__ __forceinline__ void de_map_colour(float de, float G, float T, int mode, int ar, int ag, int ab, uint32_t& r, uint32_t& g, uint32_t& b) {
    const float x = mode == AVX_DELTA_E_HEAT ? __fsub_rn(de, T) : de;
    const float v = fminf(floorf(__fadd_rn(__fmul_rn(G, x), 0.5f)), 255.0f);
    pal((int)fmaxf(v, 0.0f), r, g, b);
    if (mode == AVX_DELTA_E_HEAT && !(de > T)) r = g = b = dim_grey(ar, ag, ab);
}

// The panels of pixel (y, x) of a frame, for a kernel that walks tiles: with the side layout A's bytes, B's bytes and the map's colour
// into the three panels, otherwise the map's colour alone.  fa, fb: the frames as given; fo: the frame's panels.
__device__ __forceinline__ void de_px_panels(const DeOut& o, uint8_t* fo, const uint8_t* fa, const uint8_t* fb, size_t y, size_t x, float de) {
    const size_t at = y * o.W + x, row = (size_t)o.W * 3;  // bytes of a panel's row
    const uint8_t* pa = fa + at * 3;
    const int ar = pa[0], ag = pa[1], ab = pa[2];
    uint32_t r, g, b;
    de_map_colour(de, o.gain, o.threshold, o.mode, ar, ag, ab, r, g, b);
    if (o.side) {
        const uint8_t* pb = fb + at * 3;
        uint8_t* dst = fo + y * (3 * row) + x * 3;
        dst[0] = (uint8_t)ar, dst[1] = (uint8_t)ag, dst[2] = (uint8_t)ab;
        dst[row] = pb[0], dst[row + 1] = pb[1], dst[row + 2] = pb[2];
        dst += 2 * row;
        dst[0] = (uint8_t)r, dst[1] = (uint8_t)g, dst[2] = (uint8_t)b;
    } else {
        uint8_t* dst = fo + at * 3;
        dst[0] = (uint8_t)r, dst[1] = (uint8_t)g, dst[2] = (uint8_t)b;
    }
}

// The side layout's rows of a chunk, for a kernel that walks chunks: the `valid` pixels from pixel `base` of a frame on, whose A, B and
// map bytes start at pa, pb and so (LDS or global: the call is inlined and the address spaces are the caller's), into the frame's three
// panels at fo; row: the bytes of a panel's row.  VEC: 16-byte copies -- row is a multiple of 48, so valid is a multiple of 16 and a
// 16-byte run lies within one row, and fo, pa, pb and so are 16-byte aligned; otherwise bytes.
template <bool VEC>
__device__ __forceinline__ void de_side_rows_out(uint8_t* fo, size_t row, size_t base, int valid, const uint8_t* pa, const uint8_t* pb, const uint8_t* so) {
    constexpr int kRun = VEC ? 16 : 1;
    for (int j = threadIdx.x; j < valid * 3 / kRun; j += kThreads) {
        const size_t q = base * 3 + (size_t)j * kRun;  // byte of the frame
        const size_t y = q / row, xb = q - y * row;
        uint8_t* dst = fo + y * (3 * row) + xb;
        if (VEC) {
            *reinterpret_cast<uint4*>(dst) = reinterpret_cast<const uint4*>(pa)[j];
            *reinterpret_cast<uint4*>(dst + row) = reinterpret_cast<const uint4*>(pb)[j];
            *reinterpret_cast<uint4*>(dst + 2 * row) = reinterpret_cast<const uint4*>(so)[j];
        } else {
            dst[0] = pa[j], dst[row] = pb[j], dst[2 * row] = so[j];
        }
    }
}

// A workgroup's share of a frame's record, called by all kThreads threads with their tallies.  The sum goes to *partial in
// ssim_window.h's fixed order, everything else into the record with integer atomics; the key lies in the bytes of (max_de, max_x) until
// the finishing kernel takes it apart.
__device__ __forceinline__ void de_record_share(const DeTally& t, DeRecLds& l, double* partial, avx_delta_e_rec* rec) {
    const int tid = threadIdx.x;
    const unsigned zeros = wave_sum_u32(t.zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&l.hist[0], zeros);
    double s[1] = {t.sum};
    workgroup_sum(s, l.red);
    unsigned long long key = t.key;
    unsigned beyond = t.beyond;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_down(key, o);
        key = k > key ? k : key;
        beyond += __shfl_down(beyond, o);
    }
    if ((tid & 63) == 0) l.wred[tid >> 6] = key, l.bred[tid >> 6] = beyond;
    __syncthreads();
    if (tid == 0) {
        *partial = s[0];
        unsigned long long k = l.wred[0];
        unsigned n = l.bred[0];
        for (int w = 1; w < kThreads / 64; ++w) k = l.wred[w] > k ? l.wred[w] : k, n += l.bred[w];
        if (k >> 32) atomicMax(reinterpret_cast<unsigned long long*>(&rec->max_de), k);  // dE == 0 everywhere leaves the zeroed record
        if (n) atomicAdd(&rec->beyond, n);
    }
    hist_flush(l.hist, 256, rec->hist);
}

// The body of the finishing kernel (delta_e.hip's k_delta_e_final, grid (frames)): the frame's partials in index order -> sum; the key
// in the bytes of (max_de, max_x) -> (max_de, max_x, max_y)
__device__ __forceinline__ void de_final(const double* __restrict__ partials, size_t n_partials, int W, avx_delta_e_rec* __restrict__ rec) {
    __shared__ double red[kThreads];
    const int f = blockIdx.x;
    const double s = tile_partials_sum(partials + (size_t)f * n_partials, n_partials, red);
    if (threadIdx.x == 0) {
        const unsigned long long key = *reinterpret_cast<const unsigned long long*>(&rec[f].max_de);
        const uint32_t bits = (uint32_t)(key >> 32), index = 0xFFFFFFFFu - (uint32_t)key;
        rec[f].sum = s;
        rec[f].max_de = __uint_as_float(bits);
        rec[f].max_x = bits ? index % (uint32_t)W : 0u;
        rec[f].max_y = bits ? index / (uint32_t)W : 0u;
    }
}

// ---- host side: `fn` is the entry's name, for the messages ---------------------------------------------------------------------
// the checks that every entry makes
inline int de_check_options(avx_ctx* ctx, const char* fn, int n_frames, int H, int W, int mode, float gain, float threshold, int layout,
                            const avx_delta_e_rec* rec_dev, const float* de_out) {
    AVX_REQUIRE(ctx, rec_dev, "%s: NULL buffer (rec %p)", fn, (const void*)rec_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "%s: n_frames must be 1..16 (got %d)", fn, n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 32), "%s: bad frame size %d x %d (H * W must be below 2^32)", fn, H, W);
    AVX_REQUIRE(ctx, mode == AVX_DELTA_E_HEAT || mode == AVX_DELTA_E_PLAIN, "%s: bad mode %d", fn, mode);
    AVX_REQUIRE(ctx, layout == AVX_DELTA_E_MAP || layout == AVX_DELTA_E_SIDE, "%s: bad layout %d", fn, layout);
    AVX_REQUIRE(ctx, std::isfinite(gain) && gain > 0.0f && gain <= 255.0f, "%s: the gain must be above 0 and at most 255 (got %g)", fn, (double)gain);
    AVX_REQUIRE(ctx, std::isfinite(threshold) && threshold >= 0.0f, "%s: the threshold must be finite and at least 0 (got %g)", fn, (double)threshold);
    AVX_REQUIRE(ctx, ((uintptr_t)rec_dev & 7) == 0, "%s: rec_dev must be 8-byte aligned", fn);
    AVX_REQUIRE(ctx, ((uintptr_t)de_out & 3) == 0, "%s: de_out must be 4-byte aligned", fn);
    return AVX_OK;
}

// the checks of two uint8 batches, after de_check_options
inline int de_check_pair(avx_ctx* ctx, const char* fn, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int layout,
                         const uint8_t* map_out) {
    AVX_REQUIRE(ctx, a_hwc && b_hwc, "%s: NULL buffer (a %p, b %p)", fn, (const void*)a_hwc, (const void*)b_hwc);
    const size_t in_bytes = (size_t)n_frames * H * W * 3, map_bytes = in_bytes * (layout == AVX_DELTA_E_SIDE ? 3 : 1);
    AVX_REQUIRE(ctx, !map_out || (!overlaps(map_out, map_bytes, a_hwc, in_bytes) && !overlaps(map_out, map_bytes, b_hwc, in_bytes)),
                "%s: map_out overlaps an input (a %p, b %p, map %p)", fn, (const void*)a_hwc, (const void*)b_hwc, (const void*)map_out);
    return AVX_OK;
}

// The launch frame around an entry's own kernels.  de_begin: the stream and its workspace with scratch_bytes of scratch, the records
// zeroed.  de_finish: the check of the entry's last launch, then the finishing kernel over n_partials partials a frame.
inline int de_begin(avx_ctx* ctx, void* stream, size_t scratch_bytes, avx_delta_e_rec* rec_dev, int n_frames, hipStream_t* s, avx_ws** ws) {
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    *s = avx_pick_stream(ctx, stream);
    *ws = avx_workspace(ctx, *s);
    if (!*ws) return AVX_ERR_NOMEM;
    if (const int rc = avx_ensure_scratch(ctx, *ws, scratch_bytes)) return rc;
    AVX_HIP(ctx, hipMemsetAsync(rec_dev, 0, sizeof(avx_delta_e_rec) * (size_t)n_frames, *s));
    return AVX_OK;
}

inline int de_finish(avx_ctx* ctx, hipStream_t s, const double* partials, size_t n_partials, int W, avx_delta_e_rec* rec_dev, int n_frames) {
    AVX_HIP(ctx, hipGetLastError());
    return avx_delta_e_final_launch(ctx, partials, n_partials, W, rec_dev, n_frames, s);
}

}  // namespace
