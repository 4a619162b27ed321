// csrc/yuv_raw.hip -- raw video pixel formats (ffmpeg's -pix_fmt names: yuv420p, nv12, yuv422p, yuv444p, gray, yuv4xxp10le, p010le)
// <-> interleaved RGB uint8.  One decode and one encode family, parameterised by the format's traits (Fmt, yuv_formats.h).
//
// The arithmetic is DESIGN §4.9, the generalisation of §4.8 (csrc/yuv.hip) to 10-bit samples and other chroma layouts: int32 fixed
// point with 16 fractional bits, the tables built on the host by avx_yuv_coefficients_d (yuv.hip: the only copy) and handed to the
// kernels as launch arguments.  tests/_rawyuv_ref.py restates it in NumPy; tests/test_rawyuv_gpu.py holds these kernels to it bit
// for bit.  Pure streaming kernels, no LDS, no scratch, grid-stride over the batch:
//   * block path (any size >= 1 x 1, any format): one thread per chroma block (1, 2 or 4 pixels) with sample-sized accesses; an
//     odd last column / row is replicated into its block on encode;
//   * vector path (the 4:2:0 formats when W % 16 == 0, H is even and both buffers are 16-byte aligned): one thread owns a 16-pixel
//     x 2-row strip, as k_i420_to_rgb_v16 does, and moves it in 8- and 16-byte accesses (32 B of luma per row at 16 bits).
#include "yuv_dec.h"  // DecC, dec_px, q16_to_u8, clampi: shared with yuv_scale.hip
#include "yuv_formats.h"

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
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA, "4:2:0 only");
    const int ux = W >> 4, uy = H >> 1;                  // units per strip row, strips per frame
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = (ysz + 2 * csz) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * uy);
        const int r = (int)(t - f * ux * uy);
        const int sy = r / ux, x0 = (r - sy * ux) << 4;
        const uint8_t* fr = yuv + f * fsz;
        int u[8], v[8];
        if constexpr (F::IL) {
            int uv[16];
            load_samples<T, 16, F::SH>(fr + (ysz + (size_t)sy * W + x0) * sizeof(T), uv);
#pragma unroll
            for (int j = 0; j < 8; ++j) { u[j] = uv[2 * j] - c.cc; v[j] = uv[2 * j + 1] - c.cc; }
        } else {
            const size_t co = (size_t)sy * (W >> 1) + (x0 >> 1);
            load_samples<T, 8, F::SH>(fr + (ysz + co) * sizeof(T), u);
            load_samples<T, 8, F::SH>(fr + (ysz + csz + co) * sizeof(T), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) { u[j] -= c.cc; v[j] -= c.cc; }
        }
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            int y[16];
            load_samples<T, 16, F::SH>(fr + ((size_t)(2 * sy + row) * W + x0) * sizeof(T), y);
            uint32_t o[12];                                  // 16 RGB pixels = 48 bytes = 12 words
#pragma unroll
            for (int q = 0; q < 4; ++q) {                    // pixels 4q .. 4q + 3 -> words 3q .. 3q + 2, each word written once
                uint32_t pr[4], pg[4], pb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) dec_px(c, y[4 * q + i], u[(4 * q + i) >> 1], v[(4 * q + i) >> 1], pr[i], pg[i], pb[i]);
                o[3 * q] = pr[0] | pg[0] << 8 | pb[0] << 16 | pr[1] << 24;
                o[3 * q + 1] = pg[1] | pb[1] << 8 | pr[2] << 16 | pg[2] << 24;
                o[3 * q + 2] = pb[2] | pr[3] << 8 | pg[3] << 16 | pb[3] << 24;
            }
            uint4* d = (uint4*)(rgb + (f * ysz + (size_t)(2 * sy + row) * W + x0) * 3);
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
    }
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
    using T = typename F::T;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + (F::LUMA ? 0 : 2 * csz)) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / csz;
        const size_t r = t - f * csz;
        const int by = (int)(r / cw), bx = (int)(r - (size_t)by * cw);
        const T* fr = (const T*)(yuv + f * fsz);
        int u = 0, v = 0;
        if constexpr (!F::LUMA) {
            if constexpr (F::IL) { u = (int)(fr[ysz + 2 * r] >> F::SH) - c.cc; v = (int)(fr[ysz + 2 * r + 1] >> F::SH) - c.cc; }
            else { u = (int)(fr[ysz + r] >> F::SH) - c.cc; v = (int)(fr[ysz + csz + r] >> F::SH) - c.cc; }
        }
#pragma unroll
        for (int dy = 0; dy < BH; ++dy) {
            const int y = BH * by + dy;
            if (y >= H) break;
#pragma unroll
            for (int dx = 0; dx < BW; ++dx) {
                const int x = BW * bx + dx;
                if (x >= W) break;
                uint32_t pr, pg, pb;
                dec_px(c, (int)(fr[(size_t)y * W + x] >> F::SH), u, v, pr, pg, pb);
                uint8_t* d = rgb + (f * ysz + (size_t)y * W + x) * 3;
                d[0] = (uint8_t)pr; d[1] = (uint8_t)pg; d[2] = (uint8_t)pb;
            }
        }
    }
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
int raw_check(avx_ctx* ctx, const char* fn, int fmt, const uint8_t* yuv, const uint8_t* rgb, int n_frames, int H, int W, int matrix,
              int full_range) {
    AVX_REQUIRE(ctx, fmt_ok(fmt), "%s: pixel format %d (0 .. %d, enum avx_pix_fmt)", fn, fmt, AVX_PIX_FMT_COUNT - 1);
    AVX_REQUIRE(ctx, yuv && rgb, "%s: NULL buffer", fn);
    AVX_REQUIRE(ctx, n_frames >= 1 && H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15), "%s: bad shape (%d frames of %d x %d)", fn, n_frames, H, W);
    AVX_REQUIRE(ctx, (size_t)n_frames * H * W * 3 < ((size_t)1 << 40), "%s: %d frames of %d x %d is too large", fn, n_frames, H, W);
    const Traits& t = kTraits[fmt];
    const size_t ny = (size_t)n_frames * frame_size(t, H, W), nr = (size_t)n_frames * H * W * 3;
    AVX_REQUIRE(ctx, yuv + ny <= rgb || rgb + nr <= yuv, "%s: the source and destination must not overlap", fn);
    AVX_REQUIRE(ctx, ((uintptr_t)yuv & (t.bps - 1)) == 0, "%s: 16-bit samples need a 2-byte aligned payload", fn);
    AVX_REQUIRE(ctx, matrix == AVX_YUV_BT601 || matrix == AVX_YUV_BT709, "%s: matrix %d (0 bt601, 1 bt709)", fn, matrix);
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", fn, full_range);
    return AVX_OK;
}

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

#define AVX_RAW_DISPATCH(fmt, call)                   \
    switch (fmt) {                                    \
        case AVX_PIX_YUV420P: call(F420); break;      \
        case AVX_PIX_NV12: call(FNV12); break;        \
        case AVX_PIX_YUV422P: call(F422); break;      \
        case AVX_PIX_YUV444P: call(F444); break;      \
        case AVX_PIX_GRAY: call(FGRAY); break;        \
        case AVX_PIX_YUV420P10LE: call(F420_10); break; \
        case AVX_PIX_YUV422P10LE: call(F422_10); break; \
        case AVX_PIX_YUV444P10LE: call(F444_10); break; \
        default: call(FP010); break;                  \
    }

extern "C" int avx_yuv_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int matrix,
                                 int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = raw_check(ctx, "avx_yuv_to_rgb_u8", fmt, yuv, rgb_hwc, n_frames, H, W, matrix, full_range);
    if (rc) return rc;
    const Traits& t = kTraits[fmt];
    int d[6], e[10];
    avx_yuv_coefficients_d(matrix, full_range, t.depth, d, e);
    const DecC c = {d[0], d[1], d[2], d[3], d[4], d[5], 1 << (t.depth - 1)};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(t, yuv, rgb_hwc, H, W);
#define AVX_RAW_DEC(F) launch_dec<F>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, c)
    AVX_RAW_DISPATCH(fmt, AVX_RAW_DEC)
#undef AVX_RAW_DEC
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_rgb_to_yuv_u8(avx_ctx* ctx, int fmt, const uint8_t* rgb_hwc, uint8_t* yuv, int n_frames, int H, int W, int matrix,
                                 int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    const int rc = raw_check(ctx, "avx_rgb_to_yuv_u8", fmt, yuv, rgb_hwc, n_frames, H, W, matrix, full_range);
    if (rc) return rc;
    const Traits& t = kTraits[fmt];
    int d[6], e[10];
    avx_yuv_coefficients_d(matrix, full_range, t.depth, d, e);
    const EncC c = {e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8], e[9], 1 << (t.depth - 1), (1 << t.depth) - 1};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const bool vec = raw_vec(t, rgb_hwc, yuv, H, W);
#define AVX_RAW_ENC(F) launch_enc<F>(ctx, s, vec, rgb_hwc, yuv, n_frames, H, W, c)
    AVX_RAW_DISPATCH(fmt, AVX_RAW_ENC)
#undef AVX_RAW_ENC
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
