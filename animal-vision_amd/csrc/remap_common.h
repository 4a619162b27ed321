// csrc/remap_common.h -- the per-sample arithmetic of cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) on a uint8 frame with
// get_normalized_image's per-frame rule, shared by geom.hip (avx_binocular_warp_u8, avx_remap_linear_planes) and
// cat_wide.hip (avx_cat_wide_u8) so that both compute the same bits.  Plain float arithmetic in source order (-ffp-contract=off).
#pragma once
#include <climits>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

// cvRound(v * 32) of a remap coordinate as x86 cv2 computes it: NaN and products outside int32 convert to INT_MIN, which the
// saturation to short below turns into column / row -32768, so the pixel takes the border value.  (__float2int_rn alone
// saturates +-inf and +-1e30 the same way but turns NaN into 0, which samples pixel (0, 0).)
__device__ __forceinline__ int remap_round(float v) {
    const float q = v * 32.f;
    return (q >= -2147483648.f && q < 2147483648.f) ? __float2int_rn(q) : INT_MIN;
}

// get_normalized_image of one byte: norm is 255 when the frame holds a byte above 1, else 1 (the frame is not divided)
__device__ __forceinline__ float remap_norm(float v, float norm) {
    const float n = norm == 1.f ? v : v / 255.0f;
    return n < 0.f ? 0.f : (n > 1.f ? 1.f : n);
}

// One remapped RGB sample from the 1/32-pixel coordinates (fx, fy) = remap_round(map x / y); nrm(byte) is the normalised value.
template <typename NormFn>
__device__ __forceinline__ void remap_px_q(const uint8_t* in, int H, int W, int fx, int fy, NormFn nrm, float (&o)[3]) {
    int sx = fx >> 5, sy = fy >> 5;
    sx = sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx);
    sy = sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy);
    const float tx = (fx & 31) * (1.f / 32), ty = (fy & 31) * (1.f / 32);
    const float w0 = (1.f - ty) * (1.f - tx), w1 = (1.f - ty) * tx, w2 = ty * (1.f - tx), w3 = ty * tx;
    if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) { o[0] = o[1] = o[2] = 0.f; return; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        auto at = [&](int yy, int xx) {
            if ((unsigned)xx >= (unsigned)W || (unsigned)yy >= (unsigned)H) return 0.f;  // BORDER_CONSTANT, value 0
            return nrm(in[((size_t)yy * W + xx) * 3 + c]);
        };
        o[c] = at(sy, sx) * w0 + at(sy, sx + 1) * w1 + at(sy + 1, sx) * w2 + at(sy + 1, sx + 1) * w3;
    }
}

__device__ __forceinline__ void remap_px(const uint8_t* in, int H, int W, float mx, float my, float norm, float (&o)[3]) {
    remap_px_q(in, H, W, remap_round(mx), remap_round(my), [norm](uint8_t b) { return remap_norm((float)b, norm); }, o);
}

// The cos^2 blend of the two eyes' samples (cat_widevision_utils.py:94-98): wsum = (wl + wr) + 1e-8f, a true division, a clip.
__device__ __forceinline__ float binocular_blend(float l, float r, float wl, float wr, float wsum) {
    const float v = (l * wl + r * wr) / wsum;
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

}  // namespace
