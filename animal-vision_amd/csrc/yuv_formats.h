// csrc/yuv_formats.h -- what the raw video kernel families share (yuv_raw.hip: DESIGN §4.9; yuv_hdr.hip: §4.10): the formats' traits,
// sample-run loads, frame sizes, the vector path's condition and the launch grid.  Everything sits in an anonymous namespace: each
// translation unit gets its own copy.
#pragma once
#include "avx_internal.h"

namespace {

constexpr int kYT = 256;

// T: the sample type; SX, SY: log2 of the chroma subsampling; IL: U and V interleaved in one plane (else two planes); SH: the
// sample's value sits SH bits up (p010le); LUMA: no chroma planes at all
template <typename T_, int SX_, int SY_, bool IL_, int SH_, bool LUMA_>
struct Fmt {
    using T = T_;
    static constexpr int SX = SX_, SY = SY_, SH = SH_;
    static constexpr bool IL = IL_, LUMA = LUMA_;
};
using F420 = Fmt<uint8_t, 1, 1, false, 0, false>;
using FNV12 = Fmt<uint8_t, 1, 1, true, 0, false>;
using F422 = Fmt<uint8_t, 1, 0, false, 0, false>;
using F444 = Fmt<uint8_t, 0, 0, false, 0, false>;
using FGRAY = Fmt<uint8_t, 0, 0, false, 0, true>;
using F420_10 = Fmt<uint16_t, 1, 1, false, 0, false>;
using F422_10 = Fmt<uint16_t, 1, 0, false, 0, false>;
using F444_10 = Fmt<uint16_t, 0, 0, false, 0, false>;
using FP010 = Fmt<uint16_t, 1, 1, true, 6, false>;

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 0xffu; }

// N samples (8, 16 or 32 bytes, aligned to min(bytes, 16)) <-> ints; SH: the value's position inside the sample
template <typename T, int N, int SH>
__device__ __forceinline__ void load_samples(const uint8_t* p, int (&o)[N]) {
    constexpr int B = N * (int)sizeof(T);
    static_assert(B == 8 || B == 16 || B == 32, "8-, 16- or 32-byte runs");
    uint32_t w[B / 4];
    if constexpr (B == 8) {
        const uint2 a = *(const uint2*)p;
        w[0] = a.x; w[1] = a.y;
    } else {
#pragma unroll
        for (int i = 0; i < B / 16; ++i) {
            const uint4 a = ((const uint4*)p)[i];
            w[4 * i] = a.x; w[4 * i + 1] = a.y; w[4 * i + 2] = a.z; w[4 * i + 3] = a.w;
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if constexpr (sizeof(T) == 1) o[k] = (int)byte_of(w[k >> 2], k & 3);
        else o[k] = (int)(((w[k >> 1] >> (16 * (k & 1))) & 0xffffu) >> SH);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
struct Traits { int sx, sy, il, bps, luma, depth; };
const Traits kTraits[AVX_PIX_FMT_COUNT] = {
    {1, 1, 0, 1, 0, 8},   // yuv420p
    {1, 1, 1, 1, 0, 8},   // nv12
    {1, 0, 0, 1, 0, 8},   // yuv422p
    {0, 0, 0, 1, 0, 8},   // yuv444p
    {0, 0, 0, 1, 1, 8},   // gray
    {1, 1, 0, 2, 0, 10},  // yuv420p10le
    {1, 0, 0, 2, 0, 10},  // yuv422p10le
    {0, 0, 0, 2, 0, 10},  // yuv444p10le
    {1, 1, 1, 2, 0, 10},  // p010le
};

bool fmt_ok(int fmt) { return fmt >= 0 && fmt < AVX_PIX_FMT_COUNT; }

size_t chroma_blocks(const Traits& t, int H, int W) {
    return (size_t)((H + (1 << t.sy) - 1) >> t.sy) * (size_t)((W + (1 << t.sx) - 1) >> t.sx);
}

size_t frame_size(const Traits& t, int H, int W) { return ((size_t)H * W + (t.luma ? 0 : 2 * chroma_blocks(t, H, W))) * t.bps; }

bool raw_vec(const Traits& t, const void* a, const void* b, int H, int W) {
    return t.sx == 1 && t.sy == 1 && W % 16 == 0 && H % 2 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

unsigned raw_grid(avx_ctx* ctx, size_t units) {
    const size_t want = (units + kYT - 1) / kYT, cap = (size_t)ctx->num_cus * 32;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace
