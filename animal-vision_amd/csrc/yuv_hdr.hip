// csrc/yuv_hdr.hip -- HDR video in: 10-bit BT.2020 Y'CbCr with a PQ (SMPTE ST 2084) or HLG (BT.2100) transfer -> tone-mapped SDR
// sRGB, interleaved RGB uint8.  The formats are the four 10-bit ones of §4.9 (yuv_formats.h); the output is what
// avx_yuv_to_rgb_u8 writes, so every species downstream takes it as it is.
//
// Per pixel, in float32: Y'CbCr -> R'G'B' (BT.2020 non-constant luminance, clamp to [0, 1]) -> display light over sdr_white (the PQ
// EOTF, or the HLG inverse OETF and OOTF at 1000 nits) -> hue-preserving tone map on the largest channel (a Moebius curve above a
// knee; "clip" is the same curve with the knee at 1) -> BT.2020 to BT.709 primaries in difference form -> the project's sRGB
// encoder (the threshold tables of srgb_tables.h through the bucketed quantiser of dichromat_common.h).  The curves are evaluated
// with the hardware's exp2 / log2 / rcp (v_exp_f32, v_log_f32, v_rcp_f32: about 1 ulp each), not with a table: §4.10 says why.
// Every parameter is computed once on the host in float64 and reaches the kernels as a launch argument.  tests/_hdr_ref.py is the
// float64 definition; tests/test_hdr_host.py restates this file's float32 arithmetic and holds it within 1 code of the definition.
// The per-pixel decode itself (HdrC, the curves, hdr_px, the quantiser's tables, the host's hdr_constants) is yuv_hdr_px.h, the one
// copy this file and yuv_hdr_scale.hip (the decode fused with the INTER_AREA reduction, §4.13) compile.
//
// Streaming kernels, grid-stride over the batch, no scratch; 3 KiB of LDS hold the quantiser's two tables:
//   * block path (any size >= 1 x 1, the four formats): one thread per chroma block of 1, 2 or 4 pixels;
//   * vector path (yuv420p10le and p010le when W % 16 == 0, H is even and both buffers are 16-byte aligned, the condition of
//     k_yuv420_to_rgb_v16): one thread owns an 8-pixel x 2-row strip -- 16 bytes of luma per row, 24 bytes of RGB -- because the
//     16-pixel strip of the SDR kernel costs this one its occupancy (124-182 VGPRs against 86-98).
#include "yuv_hdr_px.h"

namespace {

// ---- vector path: kHdrStrip x 2 pixels per thread, yuv420p10le and p010le --------------------------------------------------
#ifndef AVX_HDR_STRIP
#define AVX_HDR_STRIP 8
#endif
constexpr int kHdrStrip = AVX_HDR_STRIP;  // 8 or 16 pixels of a row per thread (W % 16 == 0 admits both); DESIGN §4.10 has the figures

template <class F, int TR, int PW>
__global__ __launch_bounds__(kYT) void k_yuv420_hdr_to_rgb_vec(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                int W, HdrC c, Quant q) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA && sizeof(T) == 2, "10-bit 4:2:0 only");
    static_assert(PW == 8 || PW == 16, "8- or 16-pixel strips");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    const uint8_t* coarse = (const uint8_t*)coarse_w;
    const int ux = W / PW, uy = H >> 1;                  // units per strip row, strips per frame
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = (ysz + 2 * csz) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * uy);
        const int r = (int)(t - f * ux * uy);
        const int sy = r / ux, x0 = (r - sy * ux) * PW;
        const uint8_t* fr = yuv + f * fsz;
        int u[PW / 2], v[PW / 2];
        if constexpr (F::IL) {
            int uv[PW];
            load_samples<T, PW, F::SH>(fr + (ysz + (size_t)sy * W + x0) * sizeof(T), uv);
#pragma unroll
            for (int j = 0; j < PW / 2; ++j) { u[j] = uv[2 * j]; v[j] = uv[2 * j + 1]; }
        } else {
            const size_t co = (size_t)sy * (W >> 1) + (x0 >> 1);
            load_samples<T, PW / 2, F::SH>(fr + (ysz + co) * sizeof(T), u);
            load_samples<T, PW / 2, F::SH>(fr + (ysz + csz + co) * sizeof(T), v);
        }
        float dr[PW / 2], dg[PW / 2], db[PW / 2];
#pragma unroll
        for (int j = 0; j < PW / 2; ++j) {
            const float cb = (float)(u[j] - 512) * c.cs, cr = (float)(v[j] - 512) * c.cs;
            dr[j] = c.rv * cr; dg[j] = c.gu * cb + c.gv * cr; db[j] = c.bu * cb;
        }
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            int y[PW];
            load_samples<T, PW, F::SH>(fr + ((size_t)(2 * sy + row) * W + x0) * sizeof(T), y);
            uint32_t o[3 * PW / 4];                          // PW RGB pixels = 3 PW bytes
#pragma unroll
            for (int k = 0; k < PW / 4; ++k) {               // pixels 4k .. 4k + 3 -> words 3k .. 3k + 2, each word written once
                uint32_t pr[4], pg[4], pb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = (4 * k + i) >> 1;
                    hdr_px<TR>(c, thr, coarse, q.lo_key, (float)(y[4 * k + i] - c.yo) * c.ys, dr[j], dg[j], db[j], pr[i], pg[i], pb[i]);
                }
                o[3 * k] = pr[0] | pg[0] << 8 | pb[0] << 16 | pr[1] << 24;
                o[3 * k + 1] = pg[1] | pb[1] << 8 | pr[2] << 16 | pg[2] << 24;
                o[3 * k + 2] = pb[2] | pr[3] << 8 | pg[3] << 16 | pb[3] << 24;
            }
            uint8_t* d = rgb + (f * ysz + (size_t)(2 * sy + row) * W + x0) * 3;
            if constexpr (PW == 16) {
#pragma unroll
                for (int k = 0; k < 3; ++k) ((uint4*)d)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            } else {                                         // 24 bytes at a multiple of 24: 8-byte aligned
#pragma unroll
                for (int k = 0; k < 3; ++k) ((uint2*)d)[k] = make_uint2(o[2 * k], o[2 * k + 1]);
            }
        }
    }
}

// ---- block path: one chroma block (1, 2 or 4 pixels) per thread, any size, the four 10-bit formats --------------------------
template <class F, int TR>
__global__ __launch_bounds__(kYT) void k_yuv_hdr_to_rgb_blk(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                             HdrC c, Quant q) {
    using T = typename F::T;
    static_assert(!F::LUMA && sizeof(T) == 2, "10-bit formats with chroma only");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    const uint8_t* coarse = (const uint8_t*)coarse_w;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + 2 * csz) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / csz;
        const size_t r = t - f * csz;
        const int by = (int)(r / cw), bx = (int)(r - (size_t)by * cw);
        const T* fr = (const T*)(yuv + f * fsz);
        int u, v;
        if constexpr (F::IL) { u = (int)(fr[ysz + 2 * r] >> F::SH); v = (int)(fr[ysz + 2 * r + 1] >> F::SH); }
        else { u = (int)(fr[ysz + r] >> F::SH); v = (int)(fr[ysz + csz + r] >> F::SH); }
        const float cb = (float)(u - 512) * c.cs, cr = (float)(v - 512) * c.cs;
        const float dr = c.rv * cr, dg = c.gu * cb + c.gv * cr, db = c.bu * cb;
#pragma unroll
        for (int dy = 0; dy < BH; ++dy) {
            const int y = BH * by + dy;
            if (y >= H) break;
#pragma unroll
            for (int dx = 0; dx < BW; ++dx) {
                const int x = BW * bx + dx;
                if (x >= W) break;
                uint32_t pr, pg, pb;
                hdr_px<TR>(c, thr, coarse, q.lo_key, (float)((int)(fr[(size_t)y * W + x] >> F::SH) - c.yo) * c.ys, dr, dg, db, pr, pg, pb);
                uint8_t* d = rgb + (f * ysz + (size_t)y * W + x) * 3;
                d[0] = (uint8_t)pr; d[1] = (uint8_t)pg; d[2] = (uint8_t)pb;
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <class F, int TR>
void launch_hdr(avx_ctx* ctx, hipStream_t s, bool vec, const uint8_t* yuv, uint8_t* rgb, int n, int H, int W, const HdrC& c, const Quant& q) {
    if constexpr (F::SX == 1 && F::SY == 1) {
        if (vec) {
            const size_t units = (size_t)n * (W / kHdrStrip) * (H / 2);
            hipLaunchKernelGGL((k_yuv420_hdr_to_rgb_vec<F, TR, kHdrStrip>), dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, c, q);
            return;
        }
    }
    const size_t units = (size_t)n * ((H + (1 << F::SY) - 1) >> F::SY) * ((W + (1 << F::SX) - 1) >> F::SX);
    hipLaunchKernelGGL((k_yuv_hdr_to_rgb_blk<F, TR>), dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, c, q);
}

template <int TR>
void dispatch_hdr(avx_ctx* ctx, hipStream_t s, int fmt, bool vec, const uint8_t* yuv, uint8_t* rgb, int n, int H, int W, const HdrC& c, const Quant& q) {
    switch (fmt) {
        case AVX_PIX_YUV420P10LE: launch_hdr<F420_10, TR>(ctx, s, vec, yuv, rgb, n, H, W, c, q); break;
        case AVX_PIX_YUV422P10LE: launch_hdr<F422_10, TR>(ctx, s, vec, yuv, rgb, n, H, W, c, q); break;
        case AVX_PIX_YUV444P10LE: launch_hdr<F444_10, TR>(ctx, s, vec, yuv, rgb, n, H, W, c, q); break;
        default: launch_hdr<FP010, TR>(ctx, s, vec, yuv, rgb, n, H, W, c, q); break;
    }
}

}  // namespace

extern "C" int avx_yuv_hdr_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int full_range,
                                     int transfer, int tonemap, double peak_nits, double sdr_white, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const char* fn = "avx_yuv_hdr_to_rgb_u8";
    AVX_REQUIRE(ctx, fmt_ok(fmt) && kTraits[fmt].depth == 10,
                "%s: pixel format %d (the 10-bit formats of enum avx_pix_fmt: %d yuv420p10le, %d yuv422p10le, %d yuv444p10le, %d p010le)", fn, fmt,
                AVX_PIX_YUV420P10LE, AVX_PIX_YUV422P10LE, AVX_PIX_YUV444P10LE, AVX_PIX_P010LE);
    AVX_REQUIRE(ctx, yuv && rgb_hwc, "%s: NULL buffer", fn);
    AVX_REQUIRE(ctx, n_frames >= 1 && H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15), "%s: bad shape (%d frames of %d x %d)", fn, n_frames, H, W);
    AVX_REQUIRE(ctx, (size_t)n_frames * H * W * 3 < ((size_t)1 << 40), "%s: %d frames of %d x %d is too large", fn, n_frames, H, W);
    const Traits& t = kTraits[fmt];
    const size_t ny = (size_t)n_frames * frame_size(t, H, W), nr = (size_t)n_frames * H * W * 3;
    AVX_REQUIRE(ctx, yuv + ny <= rgb_hwc || rgb_hwc + nr <= yuv, "%s: the source and destination must not overlap", fn);
    AVX_REQUIRE(ctx, ((uintptr_t)yuv & 1) == 0, "%s: 16-bit samples need a 2-byte aligned payload", fn);
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", fn, full_range);
    AVX_REQUIRE(ctx, transfer == AVX_TRANSFER_PQ || transfer == AVX_TRANSFER_HLG, "%s: transfer %d (1 pq, 2 hlg)", fn, transfer);
    AVX_REQUIRE(ctx, tonemap == AVX_TONEMAP_CLIP || tonemap == AVX_TONEMAP_MOBIUS, "%s: tonemap %d (0 clip, 1 mobius)", fn, tonemap);
    AVX_REQUIRE(ctx, std::isfinite(peak_nits) && std::isfinite(sdr_white) && sdr_white > 0.0 && peak_nits > sdr_white,
                "%s: peak_nits %g and sdr_white %g must be finite, positive and peak_nits > sdr_white", fn, peak_nits, sdr_white);
    const HdrC c = hdr_constants(full_range, transfer, tonemap, peak_nits, sdr_white);
    const Quant q = {ctx->d_enc_thr_f32, ctx->d_coarse_f32, ctx->coarse_lo_key[0]};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(t, yuv, rgb_hwc, H, W);
    if (transfer == AVX_TRANSFER_PQ) dispatch_hdr<AVX_TRANSFER_PQ>(ctx, s, fmt, vec, yuv, rgb_hwc, n_frames, H, W, c, q);
    else dispatch_hdr<AVX_TRANSFER_HLG>(ctx, s, fmt, vec, yuv, rgb_hwc, n_frames, H, W, c, q);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
