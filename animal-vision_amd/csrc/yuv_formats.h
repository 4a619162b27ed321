// csrc/yuv_formats.h -- what the raw video kernel families share (yuv_raw.hip: DESIGN §4.9; yuv_hdr.hip: §4.10; the scaled decodes:
// §4.11, §4.13): the formats' traits and the switches over them, sample-run loads, frame sizes, the argument checks every entry
// point makes, the vector path's condition and the launch grid.  Everything sits in an anonymous namespace: each translation unit
// gets its own copy.
#pragma once
#include <cmath>

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

// N samples (8, 16 or 32 bytes, aligned to min(bytes, 16)) <-> ints; SH: the value's position inside the sample.  One sample
// or one pair (a chroma block's) is read sample by sample.
template <typename T, int N, int SH>
__device__ __forceinline__ void load_samples(const uint8_t* p, int (&o)[N]) {
    constexpr int B = N * (int)sizeof(T);
    static_assert(N <= 2 || B == 8 || B == 16 || B == 32, "one sample or one pair, or 8-, 16- or 32-byte runs");
    if constexpr (N <= 2 && B < 8) {
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = (int)(((const T*)p)[k] >> SH);
    } else {
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
}

// One switch over the nine formats and one over the four 10-bit ones: `call` is a macro of one argument, the format's Fmt
#define AVX_FMT_DISPATCH(fmt, call)                     \
    switch (fmt) {                                      \
        case AVX_PIX_YUV420P: call(F420); break;        \
        case AVX_PIX_NV12: call(FNV12); break;          \
        case AVX_PIX_YUV422P: call(F422); break;        \
        case AVX_PIX_YUV444P: call(F444); break;        \
        case AVX_PIX_GRAY: call(FGRAY); break;          \
        case AVX_PIX_YUV420P10LE: call(F420_10); break; \
        case AVX_PIX_YUV422P10LE: call(F422_10); break; \
        case AVX_PIX_YUV444P10LE: call(F444_10); break; \
        default: call(FP010); break;                    \
    }
#define AVX_FMT10_DISPATCH(fmt, call)                   \
    switch (fmt) {                                      \
        case AVX_PIX_YUV420P10LE: call(F420_10); break; \
        case AVX_PIX_YUV422P10LE: call(F422_10); break; \
        case AVX_PIX_YUV444P10LE: call(F444_10); break; \
        default: call(FP010); break;                    \
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

// What every decode entry point refuses about its buffers and sizes, under its own name; the plain decodes pass Hd = H, Wd = W
int frames_check(avx_ctx* ctx, const char* fn, const Traits& t, const uint8_t* yuv, const uint8_t* rgb, int n_frames, int H, int W, int Hd, int Wd) {
    AVX_REQUIRE(ctx, yuv && rgb, "%s: NULL buffer", fn);
    AVX_REQUIRE(ctx, n_frames >= 1 && H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15), "%s: bad shape (%d frames of %d x %d)", fn, n_frames, H, W);
    AVX_REQUIRE(ctx, Hd >= 1 && Wd >= 1, "%s: bad destination size %d x %d", fn, Hd, Wd);
    AVX_REQUIRE(ctx, Hd <= H && Wd <= W, "%s: %d x %d -> %d x %d enlarges (INTER_AREA reduces; enlarging is not supported)", fn, H, W, Hd, Wd);
    AVX_REQUIRE(ctx, (size_t)n_frames * H * W * 3 < ((size_t)1 << 40), "%s: %d frames of %d x %d is too large", fn, n_frames, H, W);
    const size_t ny = (size_t)n_frames * frame_size(t, H, W), nr = (size_t)n_frames * Hd * Wd * 3;
    AVX_REQUIRE(ctx, yuv + ny <= rgb || rgb + nr <= yuv, "%s: the source and destination must not overlap", fn);
    AVX_REQUIRE(ctx, ((uintptr_t)yuv & (t.bps - 1)) == 0, "%s: 16-bit samples need a 2-byte aligned payload", fn);
    return AVX_OK;
}

// what the SDR entry points refuse, under the entry point's name; the plain conversions pass Hd = H, Wd = W
int sdr_check(avx_ctx* ctx, const char* fn, int fmt, const uint8_t* yuv, const uint8_t* rgb, int n_frames, int H, int W, int Hd, int Wd, int matrix,
              int full_range) {
    AVX_REQUIRE(ctx, fmt_ok(fmt), "%s: pixel format %d (0 .. %d, enum avx_pix_fmt)", fn, fmt, AVX_PIX_FMT_COUNT - 1);
    if (const int rc = frames_check(ctx, fn, kTraits[fmt], yuv, rgb, n_frames, H, W, Hd, Wd)) return rc;
    AVX_REQUIRE(ctx, matrix == AVX_YUV_BT601 || matrix == AVX_YUV_BT709, "%s: matrix %d (0 bt601, 1 bt709)", fn, matrix);
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", fn, full_range);
    return AVX_OK;
}

// what the HDR entry points refuse, under the entry point's name; the plain decode passes Hd = H, Wd = W
int hdr_check(avx_ctx* ctx, const char* fn, int fmt, const uint8_t* yuv, const uint8_t* rgb, int n_frames, int H, int W, int Hd, int Wd,
              int full_range, int transfer, int tonemap, double peak_nits, double sdr_white) {
    AVX_REQUIRE(ctx, fmt_ok(fmt) && kTraits[fmt].depth == 10,
                "%s: pixel format %d (the 10-bit formats of enum avx_pix_fmt: %d yuv420p10le, %d yuv422p10le, %d yuv444p10le, %d p010le)", fn, fmt,
                AVX_PIX_YUV420P10LE, AVX_PIX_YUV422P10LE, AVX_PIX_YUV444P10LE, AVX_PIX_P010LE);
    if (const int rc = frames_check(ctx, fn, kTraits[fmt], yuv, rgb, n_frames, H, W, Hd, Wd)) return rc;
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", fn, full_range);
    AVX_REQUIRE(ctx, transfer == AVX_TRANSFER_PQ || transfer == AVX_TRANSFER_HLG, "%s: transfer %d (1 pq, 2 hlg)", fn, transfer);
    AVX_REQUIRE(ctx, tonemap == AVX_TONEMAP_CLIP || tonemap == AVX_TONEMAP_MOBIUS, "%s: tonemap %d (0 clip, 1 mobius)", fn, tonemap);
    AVX_REQUIRE(ctx, std::isfinite(peak_nits) && std::isfinite(sdr_white) && sdr_white > 0.0 && peak_nits > sdr_white,
                "%s: peak_nits %g and sdr_white %g must be finite, positive and peak_nits > sdr_white", fn, peak_nits, sdr_white);
    return AVX_OK;
}

bool raw_vec(const Traits& t, const void* a, const void* b, int H, int W) {
    return t.sx == 1 && t.sy == 1 && W % 16 == 0 && H % 2 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

unsigned raw_grid(avx_ctx* ctx, size_t units) {
    const size_t want = (units + kYT - 1) / kYT, cap = (size_t)ctx->num_cus * 32;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace
