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
// the branch is taken by a wave whose 64 pixels are all equal.  The thread's tally, the workgroup's share of the record, the map's
// quantiser and colour and the rows of the side layout are delta_e_common.h's, shared with the other colour difference kernels; so are
// the host side's checks and launch frame, on which de_walk_launch is built.
#pragma once
#include "delta_e_common.h"

namespace {

constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // pixels of a workgroup: 12288 bytes of each frame, a multiple of 48

struct DeArgs {
    const uint8_t* a;
    const uint8_t* b;
    DeOut o;
};

// value(lut, ar, ag, ab, br, bg, bb): the float32 value, never negative, of a pixel whose codes differ; lut is the decode table
template <bool VEC, class Value>
__device__ __forceinline__ void de_chunk_walk(const DeArgs& p, const Value& value) {
    __shared__ __attribute__((aligned(16))) uint8_t sa[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t sb[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t so[kChunk * 3];
    __shared__ float lut[256];
    __shared__ DeRecLds lds;
    const DeOut& o = p.o;
    const int tid = threadIdx.x, f = blockIdx.y;
    const size_t npx = (size_t)o.H * o.W;  // below 2^32
    const size_t base = (size_t)blockIdx.x * kChunk;
    const int valid = (int)min((size_t)kChunk, npx - base);  // pixels of this chunk; VEC: a multiple of 16
    const uint8_t* fa = p.a + ((size_t)f * npx + base) * 3;
    const uint8_t* fb = p.b + ((size_t)f * npx + base) * 3;
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    lds.hist[tid] = 0;
    if (VEC) {
        for (int j = tid; j < valid * 3 / 16; j += kThreads) {
            reinterpret_cast<uint4*>(sa)[j] = reinterpret_cast<const uint4*>(fa)[j];
            reinterpret_cast<uint4*>(sb)[j] = reinterpret_cast<const uint4*>(fb)[j];
        }
    } else {
        for (int j = tid; j < valid * 3; j += kThreads) sa[j] = fa[j], sb[j] = fb[j];
    }
    __syncthreads();

    const float G = o.gain, T = o.threshold;
    DeTally tally;
    float* de_out = o.de ? o.de + (size_t)f * npx + base : nullptr;
#pragma unroll 1
    for (int i = tid; i < valid; i += kThreads) {
        const int ar = sa[3 * i], ag = sa[3 * i + 1], ab = sa[3 * i + 2];
        const int br = sb[3 * i], bg = sb[3 * i + 1], bb = sb[3 * i + 2];
        float de = 0.0f;  // equal codes: 0 by definition
        if (ar != br || ag != bg || ab != bb) de = value(lut, ar, ag, ab, br, bg, bb);
        tally.add(de, (uint32_t)(base + i), T, lds.hist);
        if (de_out) de_out[i] = de;
        if (o.out) {
            uint32_t r, g, b;
            de_map_colour(de, G, T, o.mode, ar, ag, ab, r, g, b);
            so[3 * i] = (uint8_t)r, so[3 * i + 1] = (uint8_t)g, so[3 * i + 2] = (uint8_t)b;
        }
    }
    __syncthreads();

    // ---- the panels out of LDS ----
    if (o.out && o.side) {
        de_side_rows_out<VEC>(o.out + (size_t)f * npx * 9, (size_t)o.W * 3, base, valid, sa, sb, so);
    } else if (o.out) {
        uint8_t* fo = o.out + ((size_t)f * npx + base) * 3;
        if (VEC) {
            for (int j = tid; j < valid * 3 / 16; j += kThreads) reinterpret_cast<uint4*>(fo)[j] = reinterpret_cast<const uint4*>(so)[j];
        } else {
            for (int j = tid; j < valid * 3; j += kThreads) fo[j] = so[j];
        }
    }

    // ---- the record ----
    de_record_share(tally, lds, o.partials + ((size_t)f * gridDim.x + blockIdx.x), o.rec + f);
}

// The host side of an entry that walks chunks, after the checks: de_begin with the partials in the workspace scratch,
// launch(vec, grid, stream, args) for the entry's own kernel (vec: the 16-byte path), then de_finish
template <class Launch>
int de_walk_launch(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold, int layout,
                   uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream, const Launch& launch) {
    const size_t npx = (size_t)H * W, nchunks = (npx + kChunk - 1) / kChunk;  // below 2^20
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, sizeof(double) * nchunks * (size_t)n_frames, rec_dev, n_frames, &s, &ws)) return rc;
    const DeArgs p = {a_hwc, b_hwc, {map_out, de_out, (double*)ws->d_scratch, rec_dev, H, W, mode, layout == AVX_DELTA_E_SIDE, gain, threshold}};
    const bool vec = W % 16 == 0 && (((uintptr_t)a_hwc | (uintptr_t)b_hwc | (uintptr_t)map_out) & 15) == 0;
    launch(vec, dim3((unsigned)nchunks, n_frames), s, p);
    return de_finish(ctx, s, p.o.partials, nchunks, W, rec_dev, n_frames);
}

}  // namespace
