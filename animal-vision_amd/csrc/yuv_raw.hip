// csrc/yuv_raw.hip -- raw video pixel formats (ffmpeg's -pix_fmt names: yuv420p, nv12, yuv422p, yuv444p, gray, yuv4xxp10le, p010le)
// <-> interleaved RGB uint8.  One decode and one encode family, parameterised by the format's traits (Fmt, yuv_formats.h).
//
// The arithmetic is DESIGN §4.9, the generalisation of §4.8 (csrc/yuv.hip) to 10-bit samples and other chroma layouts: int32 fixed
// point with 16 fractional bits, the tables built on the host by avx_yuv_coefficients_d (yuv.hip: the only copy) and handed to the
// kernels as launch arguments.  tests/_rawyuv_ref.py restates it in NumPy; tests/test_rawyuv_gpu.py holds these kernels to it bit
// for bit.  Pure streaming kernels, no LDS, no scratch, grid-stride over the batch.  The decode kernels are the block walk and the
// 16-pixel strip walk of yuv_walks.h on DecStage; the encode kernels are this file's own, on the same two shapes (an odd last
// column / row is replicated into its block).
#include "yuv_dec.h"  // DecC, DecStage, clampi: shared with yuv_scale.hip
#include "yuv_walks.h"

namespace {

struct EncC { int yr, yg, yb, ur, ug, ub, vr, vg, vb, yo, cc, top; };  // top: 2^d - 1

__device__ __forceinline__ int enc_y(const EncC& c, int r, int g, int b) {
    return clampi(((c.yr * r + c.yg * g + c.yb * b + (1 << 15)) >> 16) + c.yo, c.top);
}
// chroma of a block of 2^LG pixels from its channel sums
template <int LG>
__device__ __forceinline__ void enc_uv(const EncC& c, int sr, int sg, int sb, int& u, int& v) {
    u = clampi(c.cc + ((c.ur * sr + c.ug * sg + c.ub * sb + (1 << (15 + LG))) >> (16 + LG)), c.top);
    v = clampi(c.cc + ((c.vr * sr + c.vg * sg + c.vb * sb + (1 << (15 + LG))) >> (16 + LG)), c.top);
}

template <typename T, int N, int SH>
__device__ __forceinline__ void store_samples(uint8_t* p, const int (&v)[N]) {
    constexpr int B = N * (int)sizeof(T);
    static_assert(B == 8 || B == 16 || B == 32, "8-, 16- or 32-byte runs");
    uint32_t w[B / 4] = {};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if constexpr (sizeof(T) == 1) w[k >> 2] |= (uint32_t)v[k] << (8 * (k & 3));
        else w[k >> 1] |= ((uint32_t)v[k] << SH) << (16 * (k & 1));
    }
    if constexpr (B == 8) {
        *(uint2*)p = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int i = 0; i < B / 16; ++i) ((uint4*)p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
}

// ---- vector path: 16 x 2 pixels per thread, the 4:2:0 formats ---------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv420_to_rgb_v16(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                            int W, DecC c) {
    walk_strip<F, DecStage, 16>(yuv, rgb, units, H, W, DecStage{c});
}

template <class F>
__global__ __launch_bounds__(kYT) void k_rgb_to_yuv420_v16(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yuv, size_t units, int H,
                                                            int W, EncC c) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA, "4:2:0 only");
    const int ux = W >> 4, uy = H >> 1;
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = (ysz + 2 * csz) * sizeof(T);
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
            int y[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int b0 = 3 * k;
                const int pr = (int)byte_of(w[b0 >> 2], b0 & 3), pg = (int)byte_of(w[(b0 + 1) >> 2], (b0 + 1) & 3),
                          pb = (int)byte_of(w[(b0 + 2) >> 2], (b0 + 2) & 3);
                y[k] = enc_y(c, pr, pg, pb);
                sr[k >> 1] += pr; sg[k >> 1] += pg; sb[k >> 1] += pb;
            }
            store_samples<T, 16, F::SH>(fr + ((size_t)(2 * sy + row) * W + x0) * sizeof(T), y);
        }
        int u[8], v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) enc_uv<2>(c, sr[j], sg[j], sb[j], u[j], v[j]);
        if constexpr (F::IL) {
            int uv[16];
#pragma unroll
            for (int j = 0; j < 8; ++j) { uv[2 * j] = u[j]; uv[2 * j + 1] = v[j]; }
            store_samples<T, 16, F::SH>(fr + (ysz + (size_t)sy * W + x0) * sizeof(T), uv);
        } else {
            const size_t co = (size_t)sy * (W >> 1) + (x0 >> 1);
            store_samples<T, 8, F::SH>(fr + (ysz + co) * sizeof(T), u);
            store_samples<T, 8, F::SH>(fr + (ysz + csz + co) * sizeof(T), v);
        }
    }
}

// ---- block path: one chroma block (1, 2 or 4 pixels) per thread, any size, any format -------------------------------------
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv_to_rgb_blk(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                         DecC c) {
    walk_blk<F>(yuv, rgb, units, H, W, DecStage{c});
}

template <class F>
__global__ __launch_bounds__(kYT) void k_rgb_to_yuv_blk(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ yuv, size_t units, int H, int W,
                                                         EncC c) {
    using T = typename F::T;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + (F::LUMA ? 0 : 2 * csz)) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / csz;
        const size_t r = t - f * csz;
        const int by = (int)(r / cw), bx = (int)(r - (size_t)by * cw);
        T* fr = (T*)(yuv + f * fsz);
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int dy = 0; dy < BH; ++dy) {
            const int y = BH * by + dy < H ? BH * by + dy : H - 1;  // an odd last row is replicated into its block
#pragma unroll
            for (int dx = 0; dx < BW; ++dx) {
                const int x = BW * bx + dx < W ? BW * bx + dx : W - 1;
                const uint8_t* s = rgb + (f * ysz + (size_t)y * W + x) * 3;
                const int pr = s[0], pg = s[1], pb = s[2];
                sr += pr; sg += pg; sb += pb;
                if (BH * by + dy < H && BW * bx + dx < W) fr[(size_t)y * W + x] = (T)(enc_y(c, pr, pg, pb) << F::SH);
            }
        }
        if constexpr (!F::LUMA) {
            int u, v;
            enc_uv<F::SX + F::SY>(c, sr, sg, sb, u, v);
            if constexpr (F::IL) { fr[ysz + 2 * r] = (T)(u << F::SH); fr[ysz + 2 * r + 1] = (T)(v << F::SH); }
            else { fr[ysz + r] = (T)(u << F::SH); fr[ysz + csz + r] = (T)(v << F::SH); }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <class F>
void launch_dec(avx_ctx* ctx, hipStream_t s, bool vec, const uint8_t* yuv, uint8_t* rgb, int n, int H, int W, const DecC& c) {
    if constexpr (F::SX == 1 && F::SY == 1) {
        if (vec) {
            const size_t units = (size_t)n * (W / 16) * (H / 2);
            hipLaunchKernelGGL(k_yuv420_to_rgb_v16<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, c);
            return;
        }
    }
    const size_t units = (size_t)n * ((H + (1 << F::SY) - 1) >> F::SY) * ((W + (1 << F::SX) - 1) >> F::SX);
    hipLaunchKernelGGL(k_yuv_to_rgb_blk<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, c);
}

template <class F>
void launch_enc(avx_ctx* ctx, hipStream_t s, bool vec, const uint8_t* rgb, uint8_t* yuv, int n, int H, int W, const EncC& c) {
    if constexpr (F::SX == 1 && F::SY == 1) {
        if (vec) {
            const size_t units = (size_t)n * (W / 16) * (H / 2);
            hipLaunchKernelGGL(k_rgb_to_yuv420_v16<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, rgb, yuv, units, H, W, c);
            return;
        }
    }
    const size_t units = (size_t)n * ((H + (1 << F::SY) - 1) >> F::SY) * ((W + (1 << F::SX) - 1) >> F::SX);
    hipLaunchKernelGGL(k_rgb_to_yuv_blk<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, rgb, yuv, units, H, W, c);
}

}  // namespace

extern "C" size_t avx_yuv_frame_size(int fmt, int H, int W) {
    if (!fmt_ok(fmt) || H < 1 || W < 1 || H > (1 << 15) || W > (1 << 15)) return 0;
    return frame_size(kTraits[fmt], H, W);
}

extern "C" int avx_yuv_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int matrix,
                                 int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = sdr_check(ctx, "avx_yuv_to_rgb_u8", fmt, yuv, rgb_hwc, n_frames, H, W, H, W, matrix, full_range);
    if (rc) return rc;
    const Traits& t = kTraits[fmt];
    const DecC c = dec_constants(matrix, full_range, t.depth);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(t, yuv, rgb_hwc, H, W);
#define AVX_RAW_DEC(F) launch_dec<F>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, c)
    AVX_FMT_DISPATCH(fmt, AVX_RAW_DEC)
#undef AVX_RAW_DEC
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_rgb_to_yuv_u8(avx_ctx* ctx, int fmt, const uint8_t* rgb_hwc, uint8_t* yuv, int n_frames, int H, int W, int matrix,
                                 int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = sdr_check(ctx, "avx_rgb_to_yuv_u8", fmt, yuv, rgb_hwc, n_frames, H, W, H, W, matrix, full_range);
    if (rc) return rc;
    const Traits& t = kTraits[fmt];
    int d[6], e[10];
    avx_yuv_coefficients_d(matrix, full_range, t.depth, d, e);
    const EncC c = {e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8], e[9], 1 << (t.depth - 1), (1 << t.depth) - 1};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(t, rgb_hwc, yuv, H, W);
#define AVX_RAW_ENC(F) launch_enc<F>(ctx, s, vec, rgb_hwc, yuv, n_frames, H, W, c)
    AVX_FMT_DISPATCH(fmt, AVX_RAW_ENC)
#undef AVX_RAW_ENC
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
