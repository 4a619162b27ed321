// csrc/cat_wide.hip -- Cat's two frames for the stream (animals/cat.py:74-109), batches of uint8 frames:
//   avx_cat_wide_u8     the wide view in ONE launch: binocular warp (two remaps + cos^2 blend) -> float32 sRGB decode ->
//                       L/M-merge colour tail (float64) -> separable Gaussian (float64) -> encode.  Defined as, and byte for
//                       byte equal to, avx_binocular_warp_u8 -> avx_dichromat_u8(in_f32 = 1) frame by frame.  The kernel is the
//                       double + L/M-merge instantiation of k_wide_fused (dichromat_wide.hip), which serves
//                       every dichromat; this entry keeps Cat's own checks and its AVX_CAT_TILE switch.
//   avx_center_zoom_u8  the baseline: cv2.resize(frame[y0:y0+ch, x0:x0+cw], (W, H), INTER_LINEAR) on uint8 (AVX_LINEAR_U8 with
//                       avx_resize_hwc's cached tables), the crop read in place through the frame's row stride.
#include <cstdlib>

#include "dichromat_common.h"
#include "resize_common.h"

using namespace avxk;

// geom.hip: the INTER_LINEAR tables avx_resize_hwc runs an H x W -> Hd x Wd resize with, out of the workspace's cache
int avx_geom_linear_tables(avx_ctx* ctx, avx_ws* ws, hipStream_t s, int H, int W, int Hd, int Wd, avx_lin_tab* ax, avx_lin_tab* ay);

namespace {

constexpr int kCT = 256;

// One thread per destination pixel of one frame; the source is the crop inside the full frame (row stride W pixels).
__global__ __launch_bounds__(kCT) void k_center_zoom_u8(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int x0, int y0, int ch,
                                                       int blocks_per_frame, avx_lin_tab ax, avx_lin_tab ay) {
    const int f = blockIdx.x / blocks_per_frame, b = blockIdx.x - f * blocks_per_frame;
    const size_t frame = (size_t)H * W * 3;
    const uint8_t* src = in + (size_t)f * frame + ((size_t)y0 * W + x0) * 3;
    uint8_t* dst = out + (size_t)f * frame;
    const unsigned npx = (unsigned)H * (unsigned)W;  // the host checks H * W < 2^31
    for (unsigned p = (unsigned)b * kCT + threadIdx.x; p < npx; p += (unsigned)blocks_per_frame * kCT) {
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
#pragma unroll
        for (int c = 0; c < 3; ++c) AVX_LINEAR_U8(dst[(size_t)p * 3 + c], src, ch, W, 3, c, x, y, ax, ay);  // resize_common.h
    }
}

}  // namespace

extern "C" int avx_cat_wide_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, const avx_dichromat_desc* d,
                               const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, d != nullptr && d->struct_size == sizeof(avx_dichromat_desc), "avx_cat_wide_u8: desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, in_hwc_u8 && out_hwc_u8, "avx_cat_wide_u8: NULL frame pointer");
    AVX_REQUIRE(ctx, d_xL && d_xR && d_ymap && d_wL && d_wR, "avx_cat_wide_u8: NULL warp table pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_cat_wide_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, d->color_mode == AVX_COLOR_CAT_MERGE, "avx_cat_wide_u8: color_mode %d is not AVX_COLOR_CAT_MERGE", d->color_mode);
    AVX_REQUIRE(ctx, d->post_mode == AVX_POST_GAUSS || d->post_mode == AVX_POST_NONE, "avx_cat_wide_u8: post_mode %d is neither AVX_POST_GAUSS nor AVX_POST_NONE",
                d->post_mode);
    AVX_REQUIRE(ctx, !d->chroma_enable, "avx_cat_wide_u8: chroma compression is not part of Cat's tail");
    if (d->post_mode == AVX_POST_GAUSS) {
        AVX_REQUIRE(ctx, d->ksize >= 1 && d->ksize <= AVX_MAX_KSIZE && (d->ksize & 1), "avx_cat_wide_u8: ksize %d must be odd, 1..%d", d->ksize, AVX_MAX_KSIZE);
        AVX_REQUIRE(ctx, d->taps_host != nullptr, "avx_cat_wide_u8: taps_host is NULL");
    }
    if (n_frames == 0) return AVX_OK;
    return avx_wide_run(ctx, "avx_cat_wide_u8", "AVX_CAT_TILE", in_hwc_u8, out_hwc_u8, n_frames, H, W, d, d_xL, d_xR, d_ymap, d_wL, d_wR, stream);
}

extern "C" int avx_center_zoom_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, int x0, int y0, int cw, int ch,
                                  void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, in_hwc_u8 && out_hwc_u8 && in_hwc_u8 != out_hwc_u8, "avx_center_zoom_u8: NULL or aliased frame pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_center_zoom_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, cw >= 1 && ch >= 1 && x0 >= 0 && y0 >= 0 && x0 <= W - cw && y0 <= H - ch,
                "avx_center_zoom_u8: crop %dx%d at (%d, %d) is empty or leaves the %dx%d frame", cw, ch, x0, y0, W, H);
    AVX_REQUIRE(ctx, (size_t)H * W < ((size_t)1 << 31), "avx_center_zoom_u8: frame larger than 2^31 pixels");
    if (n_frames == 0) return AVX_OK;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    avx_lin_tab ax{}, ay{};
    const int rc = avx_geom_linear_tables(ctx, ws, s, ch, cw, H, W, &ax, &ay);  // what avx_resize_hwc builds for (ch, cw) -> (H, W)
    if (rc) return rc;
    const int bpf = avx_blocks_per_frame(ctx, (size_t)H * W, n_frames);
    AVX_REQUIRE(ctx, (long long)bpf * n_frames < (1LL << 31), "avx_center_zoom_u8: batch too large");
    hipLaunchKernelGGL(k_center_zoom_u8, dim3((unsigned)(bpf * n_frames)), dim3(kCT), 0, s, in_hwc_u8, out_hwc_u8, H, W, x0, y0, ch, bpf, ax, ay);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
