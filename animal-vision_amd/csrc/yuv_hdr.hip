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
// The per-pixel decode itself (HdrC, the curves, hdr_px, HdrStage, the quantiser's tables, the host's hdr_constants) is
// yuv_hdr_px.h, the one copy this file and yuv_hdr_scale.hip (the decode fused with the INTER_AREA reduction, §4.13) compile.
//
// The kernels are the block walk and the strip walk of yuv_walks.h on HdrStage; 3 KiB of LDS hold the quantiser's two tables.  The
// strip is 8 pixels x 2 rows -- 16 bytes of luma per row, 24 bytes of RGB -- because the 16-pixel strip of the SDR kernel costs
// this one its occupancy (DESIGN §4.10 has the figures).
#include "yuv_hdr_px.h"
#include "yuv_walks.h"

namespace {

// ---- vector path: kHdrStrip x 2 pixels per thread, yuv420p10le and p010le --------------------------------------------------
#ifndef AVX_HDR_STRIP
#define AVX_HDR_STRIP 8
#endif
constexpr int kHdrStrip = AVX_HDR_STRIP;  // 8 or 16 pixels of a row per thread (W % 16 == 0 admits both); DESIGN §4.10 has the figures

template <class F, int TR, int PW>
__global__ __launch_bounds__(kYT) void k_yuv420_hdr_to_rgb_vec(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                int W, HdrC c, Quant q) {
    static_assert(sizeof(typename F::T) == 2, "10-bit formats only");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    walk_strip<F, HdrStage<TR>, PW>(yuv, rgb, units, H, W, HdrStage<TR>{c, thr, (const uint8_t*)coarse_w, q.lo_key});
}

// ---- block path: one chroma block (1, 2 or 4 pixels) per thread, any size, the four 10-bit formats --------------------------
template <class F, int TR>
__global__ __launch_bounds__(kYT) void k_yuv_hdr_to_rgb_blk(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                             HdrC c, Quant q) {
    static_assert(!F::LUMA && sizeof(typename F::T) == 2, "10-bit formats with chroma only");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    walk_blk<F>(yuv, rgb, units, H, W, HdrStage<TR>{c, thr, (const uint8_t*)coarse_w, q.lo_key});
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

}  // namespace

extern "C" int avx_yuv_hdr_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int full_range,
                                     int transfer, int tonemap, double peak_nits, double sdr_white, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = hdr_check(ctx, "avx_yuv_hdr_to_rgb_u8", fmt, yuv, rgb_hwc, n_frames, H, W, H, W, full_range, transfer, tonemap, peak_nits, sdr_white))
        return rc;
    const HdrC c = hdr_constants(full_range, transfer, tonemap, peak_nits, sdr_white);
    const Quant q = {ctx->d_enc_thr_f32, ctx->d_coarse_f32, ctx->coarse_lo_key[0]};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(kTraits[fmt], yuv, rgb_hwc, H, W);
#define AVX_HDR_DEC(F)                                                                                             \
    (transfer == AVX_TRANSFER_PQ ? launch_hdr<F, AVX_TRANSFER_PQ>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, c, q) \
                                 : launch_hdr<F, AVX_TRANSFER_HLG>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, c, q))
    AVX_FMT10_DISPATCH(fmt, AVX_HDR_DEC)
#undef AVX_HDR_DEC
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
