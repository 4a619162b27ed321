// csrc/yuv_hdr_px.h -- the per-pixel HDR decode of DESIGN §4.10, shared by the kernel families that restate it (yuv_hdr.hip: the
// plain decode; yuv_hdr_scale.hip: the decode fused with the INTER_AREA reduction, §4.13) so that both compute the same bits: the
// launch constants, the PQ / HLG curves on the hardware's exp2 / log2 / rcp, hdr_px, the quantiser's tables staged into LDS, and the
// host side that computes the constants in float64.  In an anonymous namespace, as yuv_formats.h: each translation unit gets its
// own copy.
#pragma once
#include <cmath>

#include "dichromat_common.h"
#include "yuv_formats.h"

namespace {

using avxk::kCoarseNFix;
using avxk::kCoarseTableBytes;

struct HdrC {
    float ys, cs;                          // y = (Y - yo) * ys; cb = (U - 512) * cs, cr = (V - 512) * cs
    int yo;
    float rv, gu, gv, bu;                  // R' = y + rv cr; G' = y + (gu cb + gv cr); B' = y + bu cb
    float gain, hlg_c;                     // pq: 10000 / sdr_white; hlg: 1000 / sdr_white, and BT.2100's c = 1/2 - a ln(4a)
    float knee, peak, inv_pk, ma, mb;      // t(m) = knee + mb u / (u + ma), u = (min(m, peak) - knee) inv_pk, for m > knee
    float m01, m02, m10, m12, m20, m21;    // the off-diagonal entries of the BT.2020 -> BT.709 matrix
};

// SMPTE ST 2084 and BT.2100 HLG constants, from their defining fractions in float64
constexpr double kPqM1 = 2610.0 / 16384.0, kPqM2 = 2523.0 / 4096.0 * 128.0;
constexpr float kPqInvM1 = (float)(1.0 / kPqM1), kPqInvM2 = (float)(1.0 / kPqM2);
constexpr float kPqC1 = (float)(3424.0 / 4096.0), kPqC2 = (float)(2413.0 / 4096.0 * 32.0), kPqC3 = (float)(2392.0 / 4096.0 * 32.0);
constexpr double kHlgA = 0.17883277, kHlgB = 1.0 - 4.0 * kHlgA;
constexpr float kHlgBf = (float)kHlgB, kHlgK = (float)(1.4426950408889634 / kHlgA);  // log2(e) / a
constexpr float kThird = (float)(1.0 / 3.0), kTwelfth = (float)(1.0 / 12.0);
constexpr float kLumR = 0.2627f, kLumG = 0.6780f, kLumB = 0.0593f, kHlgGammaM1 = 0.2f;

// x^e for x >= 0 by the hardware's log2 and exp2; 0 at x = 0
__device__ __forceinline__ float pw(float x, float e) { return x > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)) : 0.0f; }

__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

__device__ __forceinline__ float pq_eotf(float e) {  // E' in [0, 1] -> display light / 10000
    const float p = pw(e, kPqInvM2);
    const float num = p - kPqC1, den = kPqC2 - kPqC3 * p;
    return pw((num > 0.0f ? num : 0.0f) * __builtin_amdgcn_rcpf(den), kPqInvM1);
}

__device__ __forceinline__ float hlg_inv_oetf(float e, float hlg_c) {  // E' in [0, 1] -> scene light in [0, 1]
    return e <= 0.5f ? e * e * kThird : (__builtin_amdgcn_exp2f((e - hlg_c) * kHlgK) + kHlgBf) * kTwelfth;
}

// TR: AVX_TRANSFER_PQ or AVX_TRANSFER_HLG.  y: scaled luma; dr, dg, db: the chroma block's terms of R', G', B'.
template <int TR>
__device__ __forceinline__ void hdr_px(const HdrC& c, const float* thr, const uint8_t* coarse, uint32_t lo_key, float y, float dr, float dg,
                                       float db, uint32_t& r, uint32_t& g, uint32_t& b) {
    const float er = clamp01(y + dr), eg = clamp01(y + dg), eb = clamp01(y + db);
    float vr, vg, vb;
    if constexpr (TR == AVX_TRANSFER_PQ) {
        vr = c.gain * pq_eotf(er); vg = c.gain * pq_eotf(eg); vb = c.gain * pq_eotf(eb);
    } else {
        const float sr = hlg_inv_oetf(er, c.hlg_c), sg = hlg_inv_oetf(eg, c.hlg_c), sb = hlg_inv_oetf(eb, c.hlg_c);
        const float f = c.gain * pw(kLumR * sr + kLumG * sg + kLumB * sb, kHlgGammaM1);  // the OOTF's Ys^(gamma - 1), 0 at Ys = 0
        vr = f * sr; vg = f * sg; vb = f * sb;
    }
    const float m = fmaxf(vr, fmaxf(vg, vb));
    const float u = (fminf(m, c.peak) - c.knee) * c.inv_pk;
    const float t = c.knee + c.mb * u * __builtin_amdgcn_rcpf(u + c.ma);
    const float s = m > c.knee ? t * __builtin_amdgcn_rcpf(m) : 1.0f;
    const float xr = vr * s, xg = vg * s, xb = vb * s;
    const float orr = xr + (c.m01 * (xg - xr) + c.m02 * (xb - xr));
    const float og = xg + (c.m10 * (xr - xg) + c.m12 * (xb - xg));
    const float ob = xb + (c.m20 * (xr - xb) + c.m21 * (xg - xb));
    r = avxk::quantize_coarse<float, kCoarseNFix>(orr, thr, coarse, lo_key);
    g = avxk::quantize_coarse<float, kCoarseNFix>(og, thr, coarse, lo_key);
    b = avxk::quantize_coarse<float, kCoarseNFix>(ob, thr, coarse, lo_key);
}

struct Quant { const float* thr; const uint8_t* coarse; uint32_t lo_key; };  // device tables of the ctx (avx_core.hip)

// the quantiser's tables into LDS: 2 KiB of buckets and 256 thresholds (255 and a huge pad)
__device__ __forceinline__ void stage_tables(const Quant& q, uint32_t* coarse_w, float* thr) {
    for (int i = threadIdx.x; i < kCoarseTableBytes / 4; i += kYT) coarse_w[i] = ((const uint32_t*)q.coarse)[i];
    for (int i = threadIdx.x; i < 256; i += kYT) thr[i] = q.thr[i];
    __syncthreads();
}

// The HDR colour stage of the walks of yuv_walks.h, over the tables a kernel staged into its LDS: chroma terms are the block's
// terms of R', G', B', formed once per block.
template <int TR>
struct HdrStage {
    struct Chroma { float dr, dg, db; };
    const HdrC& c;
    const float* thr;
    const uint8_t* coarse;
    uint32_t lo_key;
    __device__ __forceinline__ Chroma chroma(int u_raw, int v_raw) const {
        const float cb = (float)(u_raw - 512) * c.cs, cr = (float)(v_raw - 512) * c.cs;
        return {c.rv * cr, c.gu * cb + c.gv * cr, c.bu * cb};
    }
    __device__ __forceinline__ void px(int y_raw, const Chroma& k, uint32_t& r, uint32_t& g, uint32_t& b) const {
        hdr_px<TR>(c, thr, coarse, lo_key, (float)(y_raw - c.yo) * c.ys, k.dr, k.dg, k.db, r, g, b);
    }
};

// ---- host side -------------------------------------------------------------------------------------------------------------
bool inv3(const double (&a)[3][3], double (&o)[3][3]) {
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
    if (det == 0.0) return false;
    o[0][0] = c00 / det; o[1][0] = c01 / det; o[2][0] = c02 / det;
    o[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det; o[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det; o[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    o[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det; o[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det; o[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    return true;
}

// RGB -> XYZ of a set of primaries and a white point (x, y chromaticities), as BT.2087 derives it: the primaries' XYZ columns
// scaled so that RGB = (1, 1, 1) is the white point
void rgb_to_xyz(const double (&p)[3][2], const double (&w)[2], double (&m)[3][3]) {
    double P[3][3], Pi[3][3];
    for (int j = 0; j < 3; ++j) { P[0][j] = p[j][0] / p[j][1]; P[1][j] = 1.0; P[2][j] = (1.0 - p[j][0] - p[j][1]) / p[j][1]; }
    const double W[3] = {w[0] / w[1], 1.0, (1.0 - w[0] - w[1]) / w[1]};
    inv3(P, Pi);
    for (int j = 0; j < 3; ++j) {
        const double s = Pi[j][0] * W[0] + Pi[j][1] * W[1] + Pi[j][2] * W[2];
        for (int i = 0; i < 3; ++i) m[i][j] = P[i][j] * s;
    }
}

// linear BT.2020 -> linear BT.709: inverse(RGB709 -> XYZ) x (RGB2020 -> XYZ), both at D65
void gamut_2020_to_709(double (&m)[3][3]) {
    const double p2020[3][2] = {{0.708, 0.292}, {0.170, 0.797}, {0.131, 0.046}}, p709[3][2] = {{0.64, 0.33}, {0.30, 0.60}, {0.15, 0.06}};
    const double d65[2] = {0.3127, 0.3290};
    double a[3][3], b[3][3], bi[3][3];
    rgb_to_xyz(p2020, d65, a);
    rgb_to_xyz(p709, d65, b);
    inv3(b, bi);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[i][j] = bi[i][0] * a[0][j] + bi[i][1] * a[1][j] + bi[i][2] * a[2][j];
}

HdrC hdr_constants(int full_range, int transfer, int tonemap, double peak_nits, double sdr_white) {
    const double kr = 0.2627, kb = 0.0593, kg = 1.0 - kr - kb;
    HdrC c;
    c.ys = (float)(full_range ? 1.0 / 1023.0 : 1.0 / 876.0);
    c.cs = (float)(full_range ? 1.0 / 1023.0 : 1.0 / 896.0);
    c.yo = full_range ? 0 : 64;
    c.rv = (float)(2.0 * (1.0 - kr)); c.bu = (float)(2.0 * (1.0 - kb));
    c.gu = (float)(-2.0 * kb * (1.0 - kb) / kg); c.gv = (float)(-2.0 * kr * (1.0 - kr) / kg);
    c.gain = (float)((transfer == AVX_TRANSFER_PQ ? 10000.0 : 1000.0) / sdr_white);
    c.hlg_c = (float)(0.5 - kHlgA * std::log(4.0 * kHlgA));
    const double P = peak_nits / sdr_white, k = tonemap == AVX_TONEMAP_MOBIUS ? 0.75 : 1.0, a = (1.0 - k) / (P - 1.0);
    c.knee = (float)k; c.peak = (float)P; c.inv_pk = (float)(1.0 / (P - k)); c.ma = (float)a; c.mb = (float)((1.0 - k) * (1.0 + a));
    double m[3][3];
    gamut_2020_to_709(m);
    c.m01 = (float)m[0][1]; c.m02 = (float)m[0][2]; c.m10 = (float)m[1][0]; c.m12 = (float)m[1][2]; c.m20 = (float)m[2][0]; c.m21 = (float)m[2][1];
    return c;
}

}  // namespace
