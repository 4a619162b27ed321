// csrc/yuv.hip -- YUV 4:2:0 (I420, the Y4M payload) <-> interleaved RGB uint8, int32 fixed point with 16 fractional bits.
//
// The arithmetic is the definition in DESIGN §4.8; tests/test_y4m_host.py restates it in NumPy and tests/test_yuv_gpu.py holds
// these kernels to that restatement bit for bit.  The coefficient tables are built here, on the host, from the (matrix, range)
// enums -- the only copy on the product side -- and travel to the kernels as launch arguments (no LDS, no constant upload).
//
// Layout of one frame: Y (H x W), then U and V (ceil(H/2) x ceil(W/2) each); frames back to back.  Pure streaming kernels:
//   * vector path (W % 16 == 0, H even, 16-byte aligned buffers -- 1080p, 4K): one thread owns a 16-pixel x 2-row strip, i.e. a
//     run of eight 2x2 blocks: 2 x 16 B of luma, 8 B of each chroma plane, 2 x 48 B of RGB, all in 8/16-byte accesses;
//   * scalar path (any other size): one thread per 2x2 block with byte accesses; an odd last column / row is replicated.
#include <cmath>

#include "avx_internal.h"

namespace {

constexpr int kYT = 256;

struct DecCoef { int cy, crv, cgu, cgv, cbu, yo; };             // R = cy y + crv v, G = cy y + cgu u + cgv v, B = cy y + cbu u
struct EncCoef { int yr, yg, yb, ur, ug, ub, vr, vg, vb, yo; };

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// clamp(x >> 16, 0, 255), written as a clamp of the 16.16 value before the shift (the same for every x).  The shift-then-clamp
// form of two neighbouring output bytes was selected as v_ashr_pk_u8_i32 (ROCm 7.2.0 hipcc), and those bytes came out wrong on
// the MI355X; not root-caused, see DESIGN §4.8.
__device__ __forceinline__ uint32_t q16_to_u8(int x) { return (uint32_t)(x < 0 ? 0 : (x > 0xffffff ? 0xffffff : x)) >> 16; }

// one pixel: (Y, U, V) -> R, G, B; u, v already centred
__device__ __forceinline__ void dec_px(const DecCoef& c, int Y, int u, int v, uint32_t& r, uint32_t& g, uint32_t& b) {
    const int ly = c.cy * (Y - c.yo) + (1 << 15);
    r = q16_to_u8(ly + c.crv * v);
    g = q16_to_u8(ly + c.cgu * u + c.cgv * v);
    b = q16_to_u8(ly + c.cbu * u);
}

__device__ __forceinline__ int enc_y(const EncCoef& c, int r, int g, int b) {
    return clamp255(((c.yr * r + c.yg * g + c.yb * b + (1 << 15)) >> 16) + c.yo);
}
// chroma of a 2x2 block from its channel sums
__device__ __forceinline__ void enc_uv(const EncCoef& c, int sr, int sg, int sb, int& u, int& v) {
    u = clamp255(128 + ((c.ur * sr + c.ug * sg + c.ub * sb + (1 << 17)) >> 18));
    v = clamp255(128 + ((c.vr * sr + c.vg * sg + c.vb * sb + (1 << 17)) >> 18));
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 0xffu; }

// ---- vector path: 16 x 2 pixels per thread -------------------------------------------------------------------------------
__global__ __launch_bounds__(kYT) void k_i420_to_rgb_v16(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units,
                                                          int H, int W, DecCoef c) {
    const int ux = W >> 4, uy = H >> 1;                 // units per strip row, strips per frame
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = ysz + 2 * csz;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * uy);
        const int r = (int)(t - f * ux * uy);
        const int sy = r / ux, x0 = (r - sy * ux) << 4;
        const uint8_t* fr = yuv + f * fsz;
        const uint4 y0 = *(const uint4*)(fr + (size_t)(2 * sy) * W + x0);
        const uint4 y1 = *(const uint4*)(fr + (size_t)(2 * sy + 1) * W + x0);
        const size_t co = (size_t)sy * (W >> 1) + (x0 >> 1);
        const uint2 U = *(const uint2*)(fr + ysz + co);
        const uint2 V = *(const uint2*)(fr + ysz + csz + co);
        const uint32_t yw[2][4] = {{y0.x, y0.y, y0.z, y0.w}, {y1.x, y1.y, y1.z, y1.w}};
        const uint32_t uw[2] = {U.x, U.y}, vw[2] = {V.x, V.y};
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            uint32_t o[12];                                 // 16 RGB pixels = 48 bytes = 12 words
#pragma unroll
            for (int q = 0; q < 4; ++q) {                   // pixels 4q .. 4q + 3 -> words 3q .. 3q + 2, each word written once
                uint32_t r[4], g[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 4 * q + i;
                    const int u = (int)byte_of(uw[k >> 3], (k >> 1) & 3) - 128, v = (int)byte_of(vw[k >> 3], (k >> 1) & 3) - 128;
                    dec_px(c, (int)byte_of(yw[row][q], i), u, v, r[i], g[i], b[i]);
                }
                o[3 * q] = r[0] | g[0] << 8 | b[0] << 16 | r[1] << 24;
                o[3 * q + 1] = g[1] | b[1] << 8 | r[2] << 16 | g[2] << 24;
                o[3 * q + 2] = b[2] | r[3] << 8 | g[3] << 16 | b[3] << 24;
            }
            uint4* d = (uint4*)(rgb + (f * ysz + (size_t)(2 * sy + row) * W + x0) * 3);
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
    }
}

__global__ __launch_bounds__(kYT) void k_rgb_to_i420_v16(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yuv, size_t units,
                                                          int H, int W, EncCoef c) {
    const int ux = W >> 4, uy = H >> 1;
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = ysz + 2 * csz;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * uy);
        const int r = (int)(t - f * ux * uy);
        const int sy = r / ux, x0 = (r - sy * ux) << 4;
        uint8_t* fr = yuv + f * fsz;
        int sr[8] = {}, sg[8] = {}, sb[8] = {};
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const uint4* s = (const uint4*)(rgb + (f * ysz + (size_t)(2 * sy + row) * W + x0) * 3);
            const uint4 a = s[0], b = s[1], d = s[2];
            const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
            uint32_t yo[4] = {};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int b0 = 3 * k;
                const int pr = (int)byte_of(w[b0 >> 2], b0 & 3), pg = (int)byte_of(w[(b0 + 1) >> 2], (b0 + 1) & 3),
                          pb = (int)byte_of(w[(b0 + 2) >> 2], (b0 + 2) & 3);
                yo[k >> 2] |= (uint32_t)enc_y(c, pr, pg, pb) << (8 * (k & 3));
                sr[k >> 1] += pr; sg[k >> 1] += pg; sb[k >> 1] += pb;
            }
            *(uint4*)(fr + (size_t)(2 * sy + row) * W + x0) = make_uint4(yo[0], yo[1], yo[2], yo[3]);
        }
        uint32_t uo[2] = {}, vo[2] = {};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int u, v;
            enc_uv(c, sr[j], sg[j], sb[j], u, v);
            uo[j >> 2] |= (uint32_t)u << (8 * (j & 3));
            vo[j >> 2] |= (uint32_t)v << (8 * (j & 3));
        }
        const size_t co = (size_t)sy * (W >> 1) + (x0 >> 1);
        *(uint2*)(fr + ysz + co) = make_uint2(uo[0], uo[1]);
        *(uint2*)(fr + ysz + csz + co) = make_uint2(vo[0], vo[1]);
    }
}

// ---- scalar path: one 2x2 block per thread, any size --------------------------------------------------------------------
__global__ __launch_bounds__(kYT) void k_i420_to_rgb_px(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units,
                                                         int H, int W, DecCoef c) {
    const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = ysz + 2 * csz;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / csz;
        const int r = (int)(t - f * csz);
        const int by = r / cw, bx = r - by * cw;
        const uint8_t* fr = yuv + f * fsz;
        const int u = (int)fr[ysz + r] - 128, v = (int)fr[ysz + csz + r] - 128;
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * by + dy;
            if (y >= H) break;
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * bx + dx;
                if (x >= W) break;
                uint32_t pr, pg, pb;
                dec_px(c, (int)fr[(size_t)y * W + x], u, v, pr, pg, pb);
                uint8_t* d = rgb + (f * ysz + (size_t)y * W + x) * 3;
                d[0] = (uint8_t)pr; d[1] = (uint8_t)pg; d[2] = (uint8_t)pb;
            }
        }
    }
}

__global__ __launch_bounds__(kYT) void k_rgb_to_i420_px(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yuv, size_t units,
                                                         int H, int W, EncCoef c) {
    const int cw = (W + 1) >> 1, ch = (H + 1) >> 1;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = ysz + 2 * csz;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / csz;
        const int r = (int)(t - f * csz);
        const int by = r / cw, bx = r - by * cw;
        uint8_t* fr = yuv + f * fsz;
        int sr = 0, sg = 0, sb = 0;
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * by + dy < H ? 2 * by + dy : H - 1;  // an odd last row is replicated into its block
            for (int dx = 0; dx < 2; ++dx) {
                const int x = 2 * bx + dx < W ? 2 * bx + dx : W - 1;
                const uint8_t* s = rgb + (f * ysz + (size_t)y * W + x) * 3;
                const int pr = s[0], pg = s[1], pb = s[2];
                sr += pr; sg += pg; sb += pb;
                if (2 * by + dy < H && 2 * bx + dx < W) fr[(size_t)y * W + x] = (uint8_t)enc_y(c, pr, pg, pb);
            }
        }
        int u, v;
        enc_uv(c, sr, sg, sb, u, v);
        fr[ysz + r] = (uint8_t)u;
        fr[ysz + csz + r] = (uint8_t)v;
    }
}

// ---- coefficient tables -------------------------------------------------------------------------------------
int q16(double c) { return (int)std::round(c * 65536.0); }  // std::round: half away from zero

void kr_kb(int matrix, double& kr, double& kb) {
    if (matrix == AVX_YUV_BT709) { kr = 0.2126; kb = 0.0722; }
    else { kr = 0.299; kb = 0.114; }
}

// depth d of the samples (8 or 10): s = 2^(d-8); at d = 8 these are the §4.8 values to the bit
void scales(int full_range, int depth, double& ys, double& cs, int& yo) {
    const double s = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
    if (full_range) { ys = top / 255.0; cs = top / 255.0; yo = 0; }
    else { ys = 219.0 * s / 255.0; cs = 224.0 * s / 255.0; yo = 16 << (depth - 8); }
}

DecCoef dec_coef(int matrix, int full_range, int depth = 8) {
    double kr, kb, ys, cs;
    int yo;
    kr_kb(matrix, kr, kb);
    scales(full_range, depth, ys, cs, yo);
    const double kg = 1.0 - kr - kb;
    DecCoef c;
    c.cy = q16(1.0 / ys);
    c.crv = q16(2.0 * (1.0 - kr) / cs);
    c.cgu = q16(-2.0 * kb * (1.0 - kb) / (kg * cs));
    c.cgv = q16(-2.0 * kr * (1.0 - kr) / (kg * cs));
    c.cbu = q16(2.0 * (1.0 - kb) / cs);
    c.yo = yo;
    return c;
}

EncCoef enc_coef(int matrix, int full_range, int depth = 8) {
    double kr, kb, ys, cs;
    int yo;
    kr_kb(matrix, kr, kb);
    scales(full_range, depth, ys, cs, yo);
    EncCoef c;
    // in each row the G coefficient is derived, so Y sums to round(ys 2^16) and U, V sum to 0 (greys encode to 128 exactly)
    c.yr = q16(ys * kr); c.yb = q16(ys * kb); c.yg = q16(ys) - c.yr - c.yb;
    c.ur = q16(-cs * kr / (2.0 * (1.0 - kb))); c.ub = q16(cs * 0.5); c.ug = -c.ur - c.ub;
    c.vr = q16(cs * 0.5); c.vb = q16(-cs * kb / (2.0 * (1.0 - kr))); c.vg = -c.vr - c.vb;
    c.yo = yo;
    return c;
}

// which path, and how many thread units; 0 on bad arguments (the message is set)
int yuv_check(avx_ctx* ctx, const char* fn, const void* a, const void* b, int n_frames, int H, int W, int matrix, int full_range) {
    AVX_REQUIRE(ctx, a && b, "%s: NULL buffer", fn);
    AVX_REQUIRE(ctx, a != b, "%s: the source and destination must not be the same buffer", fn);
    AVX_REQUIRE(ctx, n_frames >= 1 && H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15), "%s: bad shape (%d frames of %d x %d)", fn, n_frames, H, W);
    AVX_REQUIRE(ctx, (size_t)n_frames * H * W * 3 < ((size_t)1 << 40), "%s: %d frames of %d x %d is too large", fn, n_frames, H, W);
    AVX_REQUIRE(ctx, matrix == AVX_YUV_BT601 || matrix == AVX_YUV_BT709, "%s: matrix %d (0 bt601, 1 bt709)", fn, matrix);
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", fn, full_range);
    return AVX_OK;
}

bool yuv_vec(const void* a, const void* b, int H, int W) {
    return W % 16 == 0 && H % 2 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

unsigned yuv_grid(avx_ctx* ctx, size_t units) {
    const size_t want = (units + kYT - 1) / kYT, cap = (size_t)ctx->num_cus * 32;
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace

extern "C" int avx_i420_to_rgb_u8(avx_ctx* ctx, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int matrix, int full_range,
                                  void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = yuv_check(ctx, "avx_i420_to_rgb_u8", yuv, rgb_hwc, n_frames, H, W, matrix, full_range);
    if (rc) return rc;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const DecCoef c = dec_coef(matrix, full_range);
    if (yuv_vec(yuv, rgb_hwc, H, W)) {
        const size_t units = (size_t)n_frames * (W / 16) * (H / 2);
        hipLaunchKernelGGL(k_i420_to_rgb_v16, dim3(yuv_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb_hwc, units, H, W, c);
    } else {
        const size_t units = (size_t)n_frames * ((H + 1) / 2) * ((W + 1) / 2);
        hipLaunchKernelGGL(k_i420_to_rgb_px, dim3(yuv_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb_hwc, units, H, W, c);
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_rgb_to_i420_u8(avx_ctx* ctx, const uint8_t* rgb_hwc, uint8_t* yuv, int n_frames, int H, int W, int matrix, int full_range,
                                  void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = yuv_check(ctx, "avx_rgb_to_i420_u8", rgb_hwc, yuv, n_frames, H, W, matrix, full_range);
    if (rc) return rc;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const EncCoef c = enc_coef(matrix, full_range);
    if (yuv_vec(rgb_hwc, yuv, H, W)) {
        const size_t units = (size_t)n_frames * (W / 16) * (H / 2);
        hipLaunchKernelGGL(k_rgb_to_i420_v16, dim3(yuv_grid(ctx, units)), dim3(kYT), 0, s, rgb_hwc, yuv, units, H, W, c);
    } else {
        const size_t units = (size_t)n_frames * ((H + 1) / 2) * ((W + 1) / 2);
        hipLaunchKernelGGL(k_rgb_to_i420_px, dim3(yuv_grid(ctx, units)), dim3(kYT), 0, s, rgb_hwc, yuv, units, H, W, c);
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_yuv_coefficients_d(int matrix, int full_range, int depth, int dec_out[6], int enc_out[10]) {
    if ((matrix != AVX_YUV_BT601 && matrix != AVX_YUV_BT709) || (full_range != 0 && full_range != 1) || (depth != 8 && depth != 10) || !dec_out ||
        !enc_out)
        return AVX_ERR_INVALID;
    const DecCoef d = dec_coef(matrix, full_range, depth);
    const EncCoef e = enc_coef(matrix, full_range, depth);
    const int dv[6] = {d.cy, d.crv, d.cgu, d.cgv, d.cbu, d.yo};
    const int ev[10] = {e.yr, e.yg, e.yb, e.ur, e.ug, e.ub, e.vr, e.vg, e.vb, e.yo};
    memcpy(dec_out, dv, sizeof dv);
    memcpy(enc_out, ev, sizeof ev);
    return AVX_OK;
}

extern "C" int avx_yuv_coefficients(int matrix, int full_range, int dec_out[6], int enc_out[10]) {
    return avx_yuv_coefficients_d(matrix, full_range, 8, dec_out, enc_out);
}
