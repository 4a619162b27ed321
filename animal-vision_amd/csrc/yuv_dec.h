// csrc/yuv_dec.h -- the per-pixel YUV -> RGB decode of DESIGN §4.9, shared by the kernel families that restate it (yuv_raw.hip: the
// plain decode; yuv_scale.hip: the decode fused with the INTER_AREA reduction, §4.11) so that both compute the same bits.  In an
// anonymous namespace, as yuv_formats.h: each translation unit gets its own copy.
#pragma once
#include "avx_internal.h"

namespace {

struct DecC { int cy, crv, cgu, cgv, cbu, yo, cc; };                    // cc: the chroma centre 2^(d-1)

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// clamp(x >> 16, 0, 255) as a clamp of the 16.16 value before the shift: the form DESIGN §4.8 settled on (see yuv.hip)
__device__ __forceinline__ uint32_t q16_to_u8(int x) { return (uint32_t)(x < 0 ? 0 : (x > 0xffffff ? 0xffffff : x)) >> 16; }

__device__ __forceinline__ void dec_px(const DecC& c, int Y, int u, int v, uint32_t& r, uint32_t& g, uint32_t& b) {
    const int ly = c.cy * (Y - c.yo) + (1 << 15);
    r = q16_to_u8(ly + c.crv * v);
    g = q16_to_u8(ly + c.cgu * u + c.cgv * v);
    b = q16_to_u8(ly + c.cbu * u);
}

}  // namespace
