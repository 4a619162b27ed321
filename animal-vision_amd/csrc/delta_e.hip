// csrc/delta_e.hip -- CIEDE2000 colour difference maps on the device (the definition is include/avx.h's): per pixel of
// two uint8 sRGB batches the colour difference dE00 in CIELAB (D65), as a float32 plane, as a picture (AVX_DELTA_E_HEAT, _PLAIN; the
// map alone or A | B | map side by side) and as a record per frame: the histogram of dE in bins of 0.5, the float64 sum, the largest
// dE with the first pixel that attains it, and the number of pixels beyond the threshold.
//
// k_delta_e: grid (chunks, frames); a workgroup owns kChunk = 4096 consecutive pixels of a frame -- a function of H and W alone, so
// that the float64 sum of a frame is formed in one order whatever the batch.  The chunk of both frames goes into LDS first (VEC: W a
// multiple of 16 and every buffer 16-byte aligned, 16-byte loads; otherwise byte loads, any size and alignment); thread t then takes
// pixels t, t + 256, ... of the chunk: Lab of both (a 256-entry decode table in LDS, the anchored matrix form, cbrtf), dE00 in radians
// throughout (the four cosines of T from one sincosf by the multiple-angle formulas), and the map's bytes go back into LDS; the
// workgroup writes the panels out in 16-byte stores (VEC: a 16-byte run never leaves its row, and the panels of the side layout start
// at multiples of 48 bytes in rows of 9 W bytes) or bytes.  A pixel whose codes are equal is 0 by definition and skips the arithmetic;
// the branch is taken by a wave whose 64 pixels are all equal.  The arithmetic is the vector unit's: nothing here is bound by bytes.
// The record: the histogram is counted in LDS (zeros in a register) and flushed with one atomic per non-empty bin; a thread adds its
// pixels' dE in float64 in pixel order, the workgroup sums in ssim_window.h's fixed order into partials[frame][chunk], and
// k_delta_e_final adds a frame's partials in index order: no float atomics.  The largest dE is one 64-bit integer maximum over
// (float bits of dE << 32) | (0xFFFFFFFF - pixel index): dE is never negative, so its bits order as its value, and among equals the
// earlier pixel wins; the key lies in the bytes of (max_de, max_x) until k_delta_e_final takes it apart.
#include "lab_tables.h"
#include "map_common.h"
#include "ssim_window.h"

namespace {

constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // pixels of a workgroup: 12288 bytes of each frame, a multiple of 48
constexpr float kPi = 3.14159265358979f, kTwoPi = 6.28318530717959f;

// M': the sRGB -> XYZ (D65) matrix with every row divided by its own sum; columns 0 and 2, the anchored form needs no other
constexpr double kSX = 0.4124564 + 0.3575761 + 0.1804375, kSY = 0.2126729 + 0.7151522 + 0.0721750, kSZ = 0.0193339 + 0.1191920 + 0.9503041;
constexpr float kX0 = (float)(0.4124564 / kSX), kX2 = (float)(0.1804375 / kSX);
constexpr float kY0 = (float)(0.2126729 / kSY), kY2 = (float)(0.0721750 / kSY);
constexpr float kZ0 = (float)(0.0193339 / kSZ), kZ2 = (float)(0.9503041 / kSZ);
constexpr float kLabEps = (float)(216.0 / 24389.0);      // (6/29)^3
constexpr float kLabSlope = (float)(841.0 / 108.0);      // 1 / (3 (6/29)^2)
constexpr float kLabOffset = (float)(4.0 / 29.0);
constexpr float k25p7 = 6103515625.0f;                   // 25^7

// one rounding each, 1 ulp: v_sqrt_f32, v_rcp_f32
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fdiv(float x, float y) { return x * __builtin_amdgcn_rcpf(y); }

__device__ __forceinline__ float lab_f(float t) { return t > kLabEps ? cbrtf(t) : t * kLabSlope + kLabOffset; }

// r, g, b: decoded (linear) samples.  t_i = g + M'_i0 (r - g) + M'_i2 (b - g): r = g = b gives t_X = t_Y = t_Z = g exactly, a = b = 0
__device__ __forceinline__ void lab_of(float r, float g, float b, float& L, float& A, float& B) {
    const float dr = r - g, db = b - g;
    const float fx = lab_f((g + kX0 * dr) + kX2 * db);
    const float fy = lab_f((g + kY0 * dr) + kY2 * db);
    const float fz = lab_f((g + kZ0 * dr) + kZ2 * db);
    L = 116.0f * fy - 16.0f;
    A = 500.0f * (fx - fy);
    B = 200.0f * (fy - fz);
}

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

struct DeArgs {
    const uint8_t* a;
    const uint8_t* b;
    uint8_t* out;      // NULL: no map
    float* de;         // NULL: no float plane
    double* partials;  // [frame][chunk]
    avx_delta_e_rec* rec;
    int H, W, mode, side;
    float gain, threshold;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_delta_e(DeArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t sa[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t sb[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t so[kChunk * 3];
    __shared__ float lut[256];
    __shared__ unsigned hist[256];
    __shared__ double red[kThreads / 64];
    __shared__ unsigned long long wred[kThreads / 64];
    __shared__ unsigned bred[kThreads / 64];
    const int tid = threadIdx.x, f = blockIdx.y;
    const size_t npx = (size_t)p.H * p.W;  // below 2^32
    const size_t base = (size_t)blockIdx.x * kChunk;
    const int valid = (int)min((size_t)kChunk, npx - base);  // pixels of this chunk; VEC: a multiple of 16
    const uint8_t* fa = p.a + ((size_t)f * npx + base) * 3;
    const uint8_t* fb = p.b + ((size_t)f * npx + base) * 3;
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    hist[tid] = 0;
    if (VEC) {
        for (int j = tid; j < valid * 3 / 16; j += kThreads) {
            reinterpret_cast<uint4*>(sa)[j] = reinterpret_cast<const uint4*>(fa)[j];
            reinterpret_cast<uint4*>(sb)[j] = reinterpret_cast<const uint4*>(fb)[j];
        }
    } else {
        for (int j = tid; j < valid * 3; j += kThreads) sa[j] = fa[j], sb[j] = fb[j];
    }
    __syncthreads();

    const float G = p.gain, T = p.threshold;
    double sum = 0.0;
    unsigned long long key = 0;
    unsigned beyond = 0, zeros = 0;
    float* de_out = p.de ? p.de + (size_t)f * npx + base : nullptr;
#pragma unroll 1
    for (int i = tid; i < valid; i += kThreads) {
        const int ar = sa[3 * i], ag = sa[3 * i + 1], ab = sa[3 * i + 2];
        const int br = sb[3 * i], bg = sb[3 * i + 1], bb = sb[3 * i + 2];
        float de = 0.0f;  // equal codes: 0 by definition
        if (ar != br || ag != bg || ab != bb) {
            float L1, a1, b1, L2, a2, b2;
            lab_of(lut[ar], lut[ag], lut[ab], L1, a1, b1);
            lab_of(lut[br], lut[bg], lut[bb], L2, a2, b2);
            de = ciede2000(L1, a1, b1, L2, a2, b2);
        }
        const int bin = min(255, (int)(de + de));  // floor(2 dE): dE >= 0
        if (bin == 0) ++zeros;
        else atomicAdd(&hist[bin], 1u);
        sum += (double)de;
        beyond += de > T ? 1u : 0u;
        const unsigned long long k = ((unsigned long long)__float_as_uint(de) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(base + i));
        key = k > key ? k : key;
        if (de_out) de_out[i] = de;
        if (p.out) {
            // the quantiser: float32, one rounding per operation, multiply and add never fused
            const float x = p.mode == AVX_DELTA_E_HEAT ? __fsub_rn(de, T) : de;
            const float v = fminf(floorf(__fadd_rn(__fmul_rn(G, x), 0.5f)), 255.0f);
            uint32_t r, g, b;
            pal((int)fmaxf(v, 0.0f), r, g, b);
            if (p.mode == AVX_DELTA_E_HEAT && !(de > T)) r = g = b = dim_grey(ar, ag, ab);
            so[3 * i] = (uint8_t)r, so[3 * i + 1] = (uint8_t)g, so[3 * i + 2] = (uint8_t)b;
        }
    }
    zeros = wave_sum_u32(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&hist[0], zeros);
    __syncthreads();

    // ---- the panels out of LDS ----
    if (p.out) {
        const size_t row = (size_t)p.W * 3;  // bytes of a panel's row
        uint8_t* fo = p.out + (size_t)f * npx * 3 * (p.side ? 3 : 1);
        if (VEC) {
            for (int j = tid; j < valid * 3 / 16; j += kThreads) {
                const size_t q = base * 3 + (size_t)j * 16;  // byte of the frame: a 16-byte run lies within one row (row % 48 == 0)
                if (p.side) {
                    const size_t y = q / row, xb = q - y * row;
                    uint8_t* dst = fo + y * (3 * row) + xb;
                    *reinterpret_cast<uint4*>(dst) = reinterpret_cast<const uint4*>(sa)[j];
                    *reinterpret_cast<uint4*>(dst + row) = reinterpret_cast<const uint4*>(sb)[j];
                    *reinterpret_cast<uint4*>(dst + 2 * row) = reinterpret_cast<const uint4*>(so)[j];
                } else {
                    *reinterpret_cast<uint4*>(fo + q) = reinterpret_cast<const uint4*>(so)[j];
                }
            }
        } else {
            for (int j = tid; j < valid * 3; j += kThreads) {
                const size_t q = base * 3 + (size_t)j;
                if (p.side) {
                    const size_t y = q / row, xb = q - y * row;
                    uint8_t* dst = fo + y * (3 * row) + xb;
                    dst[0] = sa[j], dst[row] = sb[j], dst[2 * row] = so[j];
                } else {
                    fo[q] = so[j];
                }
            }
        }
    }

    // ---- the record ----
    avx_delta_e_rec* rec = p.rec + f;
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
        p.partials[(size_t)f * gridDim.x + blockIdx.x] = s[0];
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

}  // namespace

static_assert(sizeof(avx_delta_e_rec) == 1048 && offsetof(avx_delta_e_rec, max_de) == 1032, "avx_delta_e_rec: the key needs 8 aligned bytes at max_de");

extern "C" int avx_delta_e_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold,
                              int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a_hwc && b_hwc && rec_dev, "avx_delta_e_u8: NULL buffer (a %p, b %p, rec %p)", (const void*)a_hwc, (const void*)b_hwc, (void*)rec_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "avx_delta_e_u8: n_frames must be 1..16 (got %d)", n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 32), "avx_delta_e_u8: bad frame size %d x %d (H * W must be below 2^32)", H, W);
    AVX_REQUIRE(ctx, mode == AVX_DELTA_E_HEAT || mode == AVX_DELTA_E_PLAIN, "avx_delta_e_u8: bad mode %d", mode);
    AVX_REQUIRE(ctx, layout == AVX_DELTA_E_MAP || layout == AVX_DELTA_E_SIDE, "avx_delta_e_u8: bad layout %d", layout);
    AVX_REQUIRE(ctx, std::isfinite(gain) && gain > 0.0f && gain <= 255.0f, "avx_delta_e_u8: the gain must be above 0 and at most 255 (got %g)", (double)gain);
    AVX_REQUIRE(ctx, std::isfinite(threshold) && threshold >= 0.0f, "avx_delta_e_u8: the threshold must be finite and at least 0 (got %g)", (double)threshold);
    AVX_REQUIRE(ctx, ((uintptr_t)rec_dev & 7) == 0, "avx_delta_e_u8: rec_dev must be 8-byte aligned");
    AVX_REQUIRE(ctx, ((uintptr_t)de_out & 3) == 0, "avx_delta_e_u8: de_out must be 4-byte aligned");
    const size_t npx = (size_t)H * W, in_bytes = (size_t)n_frames * npx * 3, map_bytes = in_bytes * (layout == AVX_DELTA_E_SIDE ? 3 : 1);
    AVX_REQUIRE(ctx, !map_out || (!overlaps(map_out, map_bytes, a_hwc, in_bytes) && !overlaps(map_out, map_bytes, b_hwc, in_bytes)),
                "avx_delta_e_u8: map_out overlaps an input (a %p, b %p, map %p)", (const void*)a_hwc, (const void*)b_hwc, (void*)map_out);
    const size_t nchunks = (npx + kChunk - 1) / kChunk;  // below 2^20
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    const int rc = avx_ensure_scratch(ctx, ws, sizeof(double) * nchunks * (size_t)n_frames);
    if (rc) return rc;
    AVX_HIP(ctx, hipMemsetAsync(rec_dev, 0, sizeof(avx_delta_e_rec) * (size_t)n_frames, s));
    DeArgs p;
    p.a = a_hwc, p.b = b_hwc, p.out = map_out, p.de = de_out, p.partials = (double*)ws->d_scratch, p.rec = rec_dev;
    p.H = H, p.W = W, p.mode = mode, p.side = layout == AVX_DELTA_E_SIDE, p.gain = gain, p.threshold = threshold;
    const bool vec = W % 16 == 0 && (((uintptr_t)a_hwc | (uintptr_t)b_hwc | (uintptr_t)map_out) & 15) == 0;
    const dim3 grid((unsigned)nchunks, n_frames);
    if (vec) hipLaunchKernelGGL(k_delta_e<true>, grid, dim3(kThreads), 0, s, p);
    else hipLaunchKernelGGL(k_delta_e<false>, grid, dim3(kThreads), 0, s, p);
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_delta_e_final, dim3(n_frames), dim3(kThreads), 0, s, (const double*)ws->d_scratch, nchunks, W, rec_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
