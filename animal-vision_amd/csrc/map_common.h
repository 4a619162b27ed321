// csrc/map_common.h -- what the map kernels share (diff_map.hip, delta_e.hip): the palette, the dim grey of a pixel, the overlap test.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

// pal(v) = (min(255, 3v), clamp(3v - 255, 0, 255), clamp(3v - 510, 0, 255)): black - red - yellow - white; the sum is 3v
__device__ __forceinline__ void pal(int v, uint32_t& r, uint32_t& g, uint32_t& b) {
    const int t = 3 * v;
    r = (uint32_t)min(255, t);
    g = (uint32_t)min(255, max(0, t - 255));
    b = (uint32_t)max(0, t - 510);
}

// what a heat map shows where the pixel is within the threshold: a quarter of the pixel's luma
__device__ __forceinline__ uint32_t dim_grey(int r, int g, int b) { return (uint32_t)(((77 * r + 150 * g + 29 * b + 128) >> 8) >> 2); }

inline bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace
