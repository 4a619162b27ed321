// csrc/resize_common.h -- the per-pixel arithmetic of cv2.resize's INTER_AREA and INTER_LINEAR paths and the host
// construction of their per-axis tables, shared by geom.hip (avx_resize_hwc) and gallery.hip (avx_gallery_compose_u8) so
// that both compute the same bits.  Plain float arithmetic in source order (-ffp-contract=off).
#pragma once
#include <cmath>
#include <utility>
#include <vector>

#include "stack_up.h"

namespace {

struct AxisLin { int* ofs; float* f; int dmax; };
struct AxisArea { int* start; int* cnt; float* alpha; int maxcnt; };  // alpha [d][maxcnt]

// cv::saturate_cast<uchar>(float): cvRound (round half to even), clamped
__device__ __forceinline__ void put_area(float* d, float v) { *d = v; }
__device__ __forceinline__ void put_area(uint8_t* d, float v) { const float r = rintf(v); *d = (uint8_t)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r)); }

// INTER_AREA, integer ratio (an isx x isy source block per destination sample): sample (x, y) of channel c stored through `dptr`
// as saturate_cast<T>(block sum * scale).  cv::resize of a uint8 image: resizeAreaFast_<uchar, int> sums integers -- exact in
// float32 below 2^24 -- and its 8-bit 2x2 special case rounds (sum + 2) >> 2 instead.
// A statement macro, not a function (as is AVX_LINEAR_U8 below): expanded in place, k_resize_area_fast_f32 / k_resize_linear_u8
// compile to the instructions they compiled to before this code was shared; an extra inlining level reorders them.
#define AVX_AREA_FAST(T, dptr, src, W, C, c, x, y, isx, isy, area, scale)                                                              \
    {                                                                                                                                 \
        const T* S = (src) + ((size_t)((y) * (isy)) * (W) + (size_t)(x) * (isx)) * (C) + (c);                                         \
        auto at = [&](int k) { const int sy = k / (isx), sx = k - sy * (isx); return (float)S[((size_t)sy * (W) + sx) * (C)]; };      \
        float sum = 0;                                                                                                                \
        int k = 0;                                                                                                                    \
        for (; k <= (area) - 4; k += 4) sum += at(k) + at(k + 1) + at(k + 2) + at(k + 3);  /* resizeAreaFast_: groups of four */     \
        for (; k < (area); ++k) sum += at(k);                                                                                         \
        if (sizeof(T) == 1 && (isx) == 2 && (isy) == 2) put_area(dptr, (float)(((int)sum + 2) >> 2));  /* ResizeAreaFastVec, 8-bit 2x2 */ \
        else put_area(dptr, sum * (scale));                                                                                           \
    }

// INTER_AREA, general ratio: destination sample (x, y) of channel c, before saturation
template <typename T>
__device__ __forceinline__ float area_sum(const T* src, int W, int C, int c, int x, int y, const AxisArea& ax, const AxisArea& ay) {
    const int x0 = ax.start[x], nx = ax.cnt[x], y0 = ay.start[y], ny = ay.cnt[y];
    const float* al = ax.alpha + (size_t)x * ax.maxcnt;
    const float* be = ay.alpha + (size_t)y * ay.maxcnt;
    float sum = 0.f;
    for (int j = 0; j < ny; ++j) {
        const T* S = src + ((size_t)(y0 + j) * W + x0) * C + c;
        float buf = 0.f;
        for (int k = 0; k < nx; ++k) buf += (float)S[(size_t)k * C] * al[k];  // ResizeArea_Invoker: buf[dx] += S*alpha
        sum = j == 0 ? be[j] * buf : sum + be[j] * buf;               // first row of a dy starts the sum
    }
    return sum;
}

// INTER_LINEAR of a uint8 image, 11-bit fixed point: sample (x, y) of channel c assigned to the uint8_t lvalue `out`
#define AVX_LINEAR_U8(out, src, H, W, C, c, x, y, ax, ay)                                                                             \
    {                                                                                                                                 \
        const int sx = (ax).ofs[x], sy0 = (ay).ofs[y], sy1 = sy0 + 1 < (H) ? sy0 + 1 : sy0;                                           \
        const int a0 = __float2int_rn((1.f - (ax).f[x]) * 2048.f), a1 = __float2int_rn((ax).f[x] * 2048.f);  /* saturate_cast<short>: |v| <= 2048 */ \
        const int b0 = __float2int_rn((1.f - (ay).f[y]) * 2048.f), b1 = __float2int_rn((ay).f[y] * 2048.f);                          \
        const uint8_t* S0 = (src) + ((size_t)sy0 * (W) + sx) * (C) + (c);                                                             \
        const uint8_t* S1 = (src) + ((size_t)sy1 * (W) + sx) * (C) + (c);                                                             \
        int r0, r1;                                                                                                                   \
        if ((x) < (ax).dmax) { r0 = S0[0] * a0 + S0[C] * a1; r1 = S1[0] * a0 + S1[C] * a1; }                                          \
        else { r0 = S0[0] * 2048; r1 = S1[0] * 2048; }                                                                                \
        int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;                                                      \
        out = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));                                                                             \
    }

// INTER_LINEAR of a float32 image: destination sample (x, y) of channel c (k_resize_linear_f32's statement: stack_lerp)
__device__ __forceinline__ float linear_f32_px(const float* src, int H, int W, int C, int c, int x, int y, const AxisLin& ax, const AxisLin& ay) {
    const int sx = ax.ofs[x], sy0 = ay.ofs[y], sy1 = sy0 + 1 < H ? sy0 + 1 : sy0;
    const float a1 = ax.f[x], a0 = 1.f - a1, b1 = ay.f[y], b0 = 1.f - b1;
    const float* S0 = src + ((size_t)sy0 * W + sx) * C;
    const float* S1 = src + ((size_t)sy1 * W + sx) * C;
    const bool inner = x < ax.dmax;
    const int o = inner ? C : 0;
    return stack_lerp(S0[c], S0[o + c], S1[c], S1[o + c], a0, a1, b0, b1, inner);
}

// ---- host-side coefficient tables (same construction as OpenCV's resizeGeneric_ / computeResizeAreaTab) ----
struct HostLin { std::vector<int> ofs; std::vector<float> f; int dmax; };
inline HostLin host_lin(int ssize, int dsize) {
    HostLin t; t.ofs.resize(dsize); t.f.resize(dsize); t.dmax = dsize;
    const double scale = 1.0 / ((double)dsize / ssize);
    for (int d = 0; d < dsize; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { f = 0; s = 0; }
        if (s + 1 >= ssize) { if (t.dmax > d) t.dmax = d; if (s >= ssize - 1) { f = 0; s = ssize - 1; } }
        t.ofs[d] = s; t.f[d] = f;
    }
    return t;
}
inline void host_area(int ssize, int dsize, std::vector<int>& start, std::vector<int>& cnt, std::vector<float>& alpha, int& maxcnt) {
    const double scale = (double)ssize / dsize;
    std::vector<std::vector<std::pair<int, float>>> ent(dsize);
    maxcnt = 1;
    for (int dx = 0; dx < dsize; ++dx) {
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cell = std::fmin(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
        sx1 = sx1 < sx2 ? sx1 : sx2;
        if (sx1 - fsx1 > 1e-3) ent[dx].push_back({sx1 - 1, (float)((sx1 - fsx1) / cell)});
        for (int sx = sx1; sx < sx2; ++sx) ent[dx].push_back({sx, (float)(1.0 / cell)});
        if (fsx2 - sx2 > 1e-3) ent[dx].push_back({sx2, (float)(std::fmin(std::fmin(fsx2 - sx2, 1.), cell) / cell)});
        if ((int)ent[dx].size() > maxcnt) maxcnt = (int)ent[dx].size();
    }
    start.assign(dsize, 0); cnt.assign(dsize, 0); alpha.assign((size_t)dsize * maxcnt, 0.f);
    for (int dx = 0; dx < dsize; ++dx) {
        cnt[dx] = (int)ent[dx].size();
        start[dx] = cnt[dx] ? ent[dx][0].first : 0;
        for (int k = 0; k < cnt[dx]; ++k) alpha[(size_t)dx * maxcnt + k] = ent[dx][k].second;  // entries are consecutive source indices
    }
}

}  // namespace
