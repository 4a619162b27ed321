// csrc/label_common.h -- the pixel arithmetic of a Hershey-simplex label (labels.hip's k_draw_label), shared with gallery.hip's
// montage so that a label drawn there is the one avx_draw_label_u8 draws.  Segments: [n][6] {ax, ay, dx, dy, 1 / (dx^2 + dy^2)
// (0 for a point), unused} in the pixel coordinates of the image the label is drawn on.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// anti-aliased coverage of a stroke of half-thickness half_t at distance d: clamp(half_t + 0.5 - d, 0, 1)
__device__ __forceinline__ float cover(float d, float half_t) {
    const float c = half_t + 0.5f - d;
    return c < 0.f ? 0.f : (c > 1.f ? 1.f : c);
}

// distance from pixel (px, py) to the nearest of the nseg segments (round caps and joins)
__device__ __forceinline__ float label_dist(const float* seg, int nseg, float px, float py) {
    float d2 = 3.0e38f;
    for (int s = 0; s < nseg; ++s) {
        const float* g = seg + 6 * s;
        const float qx = px - g[0], qy = py - g[1];
        float t = (qx * g[2] + qy * g[3]) * g[4];
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
        const float ex = qx - t * g[2], ey = qy - t * g[3];
        const float e2 = ex * ex + ey * ey;
        d2 = e2 < d2 ? e2 : d2;
    }
    return __fsqrt_rn(d2);
}

// one channel: 60 % black box (inside it), black outline at coverage co, white text at coverage ct
__device__ __forceinline__ uint8_t label_blend(uint8_t in, bool inbox, float co, float ct) {
    float v = (float)in;
    if (inbox) v = rintf(v * 0.4f);       // addWeighted(overlay, 0.6, img, 0.4): the overlay is black inside the box
    v = rintf(v - v * co);                // black outline: v + (0 - v) * coverage
    v = rintf(v + (255.f - v) * ct);      // white text
    return (uint8_t)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

}  // namespace
