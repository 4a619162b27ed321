// csrc/delta_e_walk.h -- the chunk walk of the pointwise colour difference kernels (delta_e.hip: dE00 of two Lab triples;
// receptor.hip: the receptor-noise-limited distance of two sets of catches), in one copy: what a workgroup does with its kChunk = 4096
// consecutive pixels of a frame pair is the same whatever the measure, and only the value of a pixel whose codes differ is the caller's.
//
// de_chunk_walk: grid (chunks, frames); a chunk is a function of H and W alone, so that the float64 sum of a frame is formed in one
// order whatever the batch.  The chunk of both frames goes into LDS first (VEC: W a multiple of 16 and every buffer 16-byte aligned,
// 16-byte loads; otherwise byte loads, any size and alignment); thread t then takes pixels t, t + 256, ... of the chunk: the value
// (the decode table is in LDS), the record's share, the float plane, and the map's bytes, which go back into LDS; the workgroup
// writes the panels out in 16-byte stores (VEC: a 16-byte run never leaves its row, and the panels of the side layout start at
// multiples of 48 bytes in rows of 9 W bytes) or bytes.  A pixel whose codes are equal is 0 by definition and skips the arithmetic;
// the branch is taken by a wave whose 64 pixels are all equal.  The quantiser of the map is float32 with one rounding per operation.
#pragma once
#include <cmath>

#include "delta_e_common.h"

namespace {

constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // pixels of a workgroup: 12288 bytes of each frame, a multiple of 48

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

// value(lut, ar, ag, ab, br, bg, bb): the float32 value, never negative, of a pixel whose codes differ; lut is the decode table
template <bool VEC, class Value>
__device__ __forceinline__ void de_chunk_walk(const DeArgs& p, const Value& value) {
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
        if (ar != br || ag != bg || ab != bb) de = value(lut, ar, ag, ab, br, bg, bb);
        const int bin = min(255, (int)(de + de));  // floor(2 dE): dE >= 0
        if (bin == 0) ++zeros;
        else atomicAdd(&hist[bin], 1u);
        sum += (double)de;
        beyond += de > T ? 1u : 0u;
        const unsigned long long k = de_key(de, (uint32_t)(base + i));
        key = k > key ? k : key;
        if (de_out) de_out[i] = de;
        if (p.out) {
            // the quantiser: float32, one rounding per operation, multiply and add never fused
            const float x = p.mode == AVX_DELTA_E_HEAT ? __fsub_rn(de, T) : de;
            const float v = fminf(floorf(__fadd_rn(__fmul_rn(G, x), 0.5f)), 255.0f);
            uint32_t r, g, b;
            de_colour(v, de, T, p.mode, ar, ag, ab, r, g, b);
            so[3 * i] = (uint8_t)r, so[3 * i + 1] = (uint8_t)g, so[3 * i + 2] = (uint8_t)b;
        }
    }
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
    de_record_share(sum, key, beyond, zeros, hist, red, wred, bred, p.partials + ((size_t)f * gridDim.x + blockIdx.x), p.rec + f);
}

// The host side of an entry that walks chunks (`fn` is its name, for the messages): the checks of avx_delta_e_u8 ...
inline int de_walk_check(avx_ctx* ctx, const char* fn, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain,
                         float threshold, int layout, const uint8_t* map_out, const avx_delta_e_rec* rec_dev, const float* de_out) {
    AVX_REQUIRE(ctx, a_hwc && b_hwc && rec_dev, "%s: NULL buffer (a %p, b %p, rec %p)", fn, (const void*)a_hwc, (const void*)b_hwc, (const void*)rec_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "%s: n_frames must be 1..16 (got %d)", fn, n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 32), "%s: bad frame size %d x %d (H * W must be below 2^32)", fn, H, W);
    AVX_REQUIRE(ctx, mode == AVX_DELTA_E_HEAT || mode == AVX_DELTA_E_PLAIN, "%s: bad mode %d", fn, mode);
    AVX_REQUIRE(ctx, layout == AVX_DELTA_E_MAP || layout == AVX_DELTA_E_SIDE, "%s: bad layout %d", fn, layout);
    AVX_REQUIRE(ctx, std::isfinite(gain) && gain > 0.0f && gain <= 255.0f, "%s: the gain must be above 0 and at most 255 (got %g)", fn, (double)gain);
    AVX_REQUIRE(ctx, std::isfinite(threshold) && threshold >= 0.0f, "%s: the threshold must be finite and at least 0 (got %g)", fn, (double)threshold);
    AVX_REQUIRE(ctx, ((uintptr_t)rec_dev & 7) == 0, "%s: rec_dev must be 8-byte aligned", fn);
    AVX_REQUIRE(ctx, ((uintptr_t)de_out & 3) == 0, "%s: de_out must be 4-byte aligned", fn);
    const size_t npx = (size_t)H * W, in_bytes = (size_t)n_frames * npx * 3, map_bytes = in_bytes * (layout == AVX_DELTA_E_SIDE ? 3 : 1);
    AVX_REQUIRE(ctx, !map_out || (!overlaps(map_out, map_bytes, a_hwc, in_bytes) && !overlaps(map_out, map_bytes, b_hwc, in_bytes)),
                "%s: map_out overlaps an input (a %p, b %p, map %p)", fn, (const void*)a_hwc, (const void*)b_hwc, (const void*)map_out);
    return AVX_OK;
}

// ... and its launches, after the checks: the records zeroed, the partials in the workspace scratch, launch(vec, grid, stream, args)
// for the entry's own kernel (vec: the 16-byte path), then k_delta_e_final
template <class Launch>
int de_walk_launch(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold, int layout,
                   uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream, const Launch& launch) {
    const size_t npx = (size_t)H * W, nchunks = (npx + kChunk - 1) / kChunk;  // below 2^20
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
    launch(vec, dim3((unsigned)nchunks, n_frames), s, p);
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_delta_e_final, dim3(n_frames), dim3(kThreads), 0, s, (const double*)ws->d_scratch, nchunks, W, rec_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

}  // namespace
