// csrc/yuv_dec.h -- the per-pixel YUV -> RGB decode of DESIGN §4.9, shared by the kernel families that restate it (yuv_raw.hip: the
// plain decode; yuv_scale.hip: the decode fused with the INTER_AREA reduction, §4.11) so that both compute the same bits, and the
// stage that hands it to the shared walks (yuv_walks.h).  In an anonymous namespace, as yuv_formats.h: each translation unit gets
// its own copy.
#pragma once
#include "yuv_formats.h"

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

// The SDR colour stage of the walks of yuv_walks.h: chroma terms are the centred pair; a gray frame's stay {0, 0}.
struct DecStage {
    struct Chroma { int u, v; };
    const DecC& c;
    __device__ __forceinline__ Chroma chroma(int u_raw, int v_raw) const { return {u_raw - c.cc, v_raw - c.cc}; }
    __device__ __forceinline__ void px(int y_raw, const Chroma& k, uint32_t& r, uint32_t& g, uint32_t& b) const {
        dec_px(c, y_raw, k.u, k.v, r, g, b);
    }
};

// ---- host side -------------------------------------------------------------------------------------------------------------
DecC dec_constants(int matrix, int full_range, int depth) {
    int d[6], e[10];
    avx_yuv_coefficients_d(matrix, full_range, depth, d, e);
    return {d[0], d[1], d[2], d[3], d[4], d[5], 1 << (depth - 1)};
}

}  // namespace
