// csrc/yuv_scale.hip -- raw video pixel formats -> interleaved RGB uint8 at a smaller size, in one launch per batch.
//
// The definition, byte for byte, is the chain it replaces: avx_yuv_to_rgb_u8 (yuv_raw.hip, §4.9) into a full-size RGB frame, then
// avx_resize_hwc(uint8, INTER_AREA) of that frame (geom.hip, resize_common.h).  These kernels restate both steps per destination
// pixel and never write the full-size frame:
//   * the decode is dec_px (yuv_dec.h) with chroma replicated over its block: source pixel (sx, sy) takes chroma (sx >> SX, sy >> SY);
//   * integer ratios (W = isx Wd, H = isy Hd) restate AVX_AREA_FAST for uint8: the integer sum of the isx x isy decoded samples per
//     channel -- below 2^24, so an int accumulator holds the bits resizeAreaFast_'s float sum holds, in any order -- then
//     (sum + 2) >> 2 for 2 x 2 and rintf((float)sum * (1.f / area)) otherwise;
//   * any other ratio restates area_sum with the table cache's own per-axis tables (avx_geom_area_tables): buf += S * alpha[k] along
//     x, sum = beta[0] * buf for the first row and sum + beta[j] * buf after it, put_area at the end; float32, in that order
//     (-ffp-contract=off).  The three channels are independent chains: one thread decodes a source pixel once and feeds all three.
// Pure streaming kernels in the style of yuv_raw.hip: templates over the Fmt traits, kYT threads, raw_grid, grid-stride over the
// batch, no LDS, no scratch.  tests/test_yuv_scale_gpu.py holds them to the chain bit for bit.
#include <cfloat>
#include <cmath>

#include "resize_common.h"
#include "yuv_dec.h"
#include "yuv_formats.h"

namespace {

// the chroma pair of block r (row-major over the frame's chroma blocks) of frame `fr`, centred
template <class F>
__device__ __forceinline__ void load_uv(const typename F::T* fr, size_t ysz, size_t csz, size_t r, int cc, int& u, int& v) {
    if constexpr (F::IL) { u = (int)(fr[ysz + 2 * r] >> F::SH) - cc; v = (int)(fr[ysz + 2 * r + 1] >> F::SH) - cc; }
    else { u = (int)(fr[ysz + r] >> F::SH) - cc; v = (int)(fr[ysz + csz + r] >> F::SH) - cc; }
}

// ---- integer ratio: one thread per destination pixel, any format, any size ----------------------------------------------------
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv_to_rgb_area_int(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                              int Hd, int Wd, int isx, int isy, DecC c) {
    using T = typename F::T;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + (F::LUMA ? 0 : 2 * csz)) * sizeof(T);
    const size_t dsz = (size_t)Hd * Wd;
    const bool two = isx == 2 && isy == 2;       // ResizeAreaFastVec, 8-bit 2 x 2
    const float scale = 1.f / (isx * isy);       // k_resize_area_fast_f32's
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / dsz;
        const size_t r = t - f * dsz;
        const int dy = (int)(r / Wd), dx = (int)(r - (size_t)dy * Wd);
        const T* fr = (const T*)(yuv + f * fsz);
        int sr = 0, sg = 0, sb = 0, u = 0, v = 0, cbx = -1, cby = -1;
        for (int j = 0; j < isy; ++j) {
            const int y = dy * isy + j;          // < H: H = isy Hd
            const T* yrow = fr + (size_t)y * W;
            for (int k = 0; k < isx; ++k) {
                const int x = dx * isx + k;      // < W
                if constexpr (!F::LUMA) {
                    const int bx = x >> F::SX, by = y >> F::SY;
                    if (bx != cbx || by != cby) {  // reloaded only when the chroma block changes
                        cbx = bx; cby = by;
                        load_uv<F>(fr, ysz, csz, (size_t)by * cw + bx, c.cc, u, v);
                    }
                }
                uint32_t pr, pg, pb;
                dec_px(c, (int)(yrow[x] >> F::SH), u, v, pr, pg, pb);
                sr += (int)pr; sg += (int)pg; sb += (int)pb;
            }
        }
        uint8_t* d = rgb + t * 3;
        if (two) { d[0] = (uint8_t)((sr + 2) >> 2); d[1] = (uint8_t)((sg + 2) >> 2); d[2] = (uint8_t)((sb + 2) >> 2); }
        else { put_area(d, (float)sr * scale); put_area(d + 1, (float)sg * scale); put_area(d + 2, (float)sb * scale); }
    }
}

// ---- 2 x 2 of the 4:2:0 formats, vector path: 8 destination pixels of one row per thread ----------------------------------------
// An output pixel is exactly one chroma block.  W % 32 == 0, H even, both buffers 16-byte aligned (half_vec below): every run is
// aligned to its access.  Same sums, same (sum + 2) >> 2 as k_yuv_to_rgb_area_int: byte-identical output.
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv420_to_rgb_half_vec(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                 int W, DecC c) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA, "4:2:0 only");
    const int Hd = H >> 1, Wd = W >> 1, ux = Wd >> 3;      // units per destination row
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = (ysz + 2 * csz) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * Hd);
        const int r = (int)(t - f * ux * Hd);
        const int dy = r / ux, x0 = (r - dy * ux) << 4;    // x0: the first source column
        const uint8_t* fr = yuv + f * fsz;
        int u[8], v[8];
        if constexpr (F::IL) {
            int uv[16];
            load_samples<T, 16, F::SH>(fr + (ysz + (size_t)dy * W + x0) * sizeof(T), uv);
#pragma unroll
            for (int j = 0; j < 8; ++j) { u[j] = uv[2 * j] - c.cc; v[j] = uv[2 * j + 1] - c.cc; }
        } else {
            const size_t co = (size_t)dy * (W >> 1) + (x0 >> 1);
            load_samples<T, 8, F::SH>(fr + (ysz + co) * sizeof(T), u);
            load_samples<T, 8, F::SH>(fr + (ysz + csz + co) * sizeof(T), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) { u[j] -= c.cc; v[j] -= c.cc; }
        }
        int sr[8] = {}, sg[8] = {}, sb[8] = {};
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            int y[16];
            load_samples<T, 16, F::SH>(fr + ((size_t)(2 * dy + row) * W + x0) * sizeof(T), y);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                uint32_t pr, pg, pb;
                dec_px(c, y[k], u[k >> 1], v[k >> 1], pr, pg, pb);
                sr[k >> 1] += (int)pr; sg[k >> 1] += (int)pg; sb[k >> 1] += (int)pb;
            }
        }
        uint32_t b[24];                                    // 8 RGB pixels = 24 bytes = three 8-byte stores
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            b[3 * i] = (uint32_t)(sr[i] + 2) >> 2; b[3 * i + 1] = (uint32_t)(sg[i] + 2) >> 2; b[3 * i + 2] = (uint32_t)(sb[i] + 2) >> 2;
        }
        uint32_t o[6];
#pragma unroll
        for (int w = 0; w < 6; ++w) o[w] = b[4 * w] | b[4 * w + 1] << 8 | b[4 * w + 2] << 16 | b[4 * w + 3] << 24;
        uint2* d = (uint2*)(rgb + ((f * Hd + dy) * (size_t)Wd + (x0 >> 1)) * 3);
        d[0] = make_uint2(o[0], o[1]);
        d[1] = make_uint2(o[2], o[3]);
        d[2] = make_uint2(o[4], o[5]);
    }
}

// ---- any other ratio: one thread per destination pixel, the table cache's INTER_AREA tables ---------------------------------------
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv_to_rgb_area_gen(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                              int Hd, int Wd, AxisArea ax, AxisArea ay, DecC c) {
    using T = typename F::T;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + (F::LUMA ? 0 : 2 * csz)) * sizeof(T);
    const size_t dsz = (size_t)Hd * Wd;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / dsz;
        const size_t r = t - f * dsz;
        const int dy = (int)(r / Wd), dx = (int)(r - (size_t)dy * Wd);
        const T* fr = (const T*)(yuv + f * fsz);
        const int x0 = ax.start[dx], nx = ax.cnt[dx], y0 = ay.start[dy], ny = ay.cnt[dy];  // area_sum's walk (resize_common.h)
        const float* al = ax.alpha + (size_t)dx * ax.maxcnt;
        const float* be = ay.alpha + (size_t)dy * ay.maxcnt;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        int u = 0, v = 0, cbx = -1, cby = -1;
        for (int j = 0; j < ny; ++j) {
            const int y = y0 + j;
            const T* yrow = fr + (size_t)y * W;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = 0; k < nx; ++k) {
                const int x = x0 + k;
                if constexpr (!F::LUMA) {
                    const int bx = x >> F::SX, by = y >> F::SY;
                    if (bx != cbx || by != cby) {
                        cbx = bx; cby = by;
                        load_uv<F>(fr, ysz, csz, (size_t)by * cw + bx, c.cc, u, v);
                    }
                }
                uint32_t pr, pg, pb;
                dec_px(c, (int)(yrow[x] >> F::SH), u, v, pr, pg, pb);
                const float a = al[k];
                b0 += (float)pr * a; b1 += (float)pg * a; b2 += (float)pb * a;  // ResizeArea_Invoker: buf[dx] += S*alpha
            }
            const float w = be[j];
            if (j == 0) { s0 = w * b0; s1 = w * b1; s2 = w * b2; }            // first row of a dy starts the sum
            else { s0 = s0 + w * b0; s1 = s1 + w * b1; s2 = s2 + w * b2; }
        }
        uint8_t* d = rgb + t * 3;
        put_area(d, s0); put_area(d + 1, s1); put_area(d + 2, s2);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
constexpr const char* kFn = "avx_yuv_to_rgb_scaled_u8";

int scale_check(avx_ctx* ctx, int fmt, const uint8_t* yuv, const uint8_t* rgb, int n_frames, int H, int W, int Hd, int Wd, int matrix,
                int full_range) {
    AVX_REQUIRE(ctx, fmt_ok(fmt), "%s: pixel format %d (0 .. %d, enum avx_pix_fmt)", kFn, fmt, AVX_PIX_FMT_COUNT - 1);
    AVX_REQUIRE(ctx, yuv && rgb, "%s: NULL buffer", kFn);
    AVX_REQUIRE(ctx, n_frames >= 1 && H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15), "%s: bad shape (%d frames of %d x %d)", kFn, n_frames, H, W);
    AVX_REQUIRE(ctx, Hd >= 1 && Wd >= 1, "%s: bad destination size %d x %d", kFn, Hd, Wd);
    AVX_REQUIRE(ctx, Hd <= H && Wd <= W, "%s: %d x %d -> %d x %d enlarges (INTER_AREA reduces; enlarging is not supported)", kFn, H, W, Hd, Wd);
    AVX_REQUIRE(ctx, (size_t)n_frames * H * W * 3 < ((size_t)1 << 40), "%s: %d frames of %d x %d is too large", kFn, n_frames, H, W);
    const Traits& t = kTraits[fmt];
    const size_t ny = (size_t)n_frames * frame_size(t, H, W), nr = (size_t)n_frames * Hd * Wd * 3;
    AVX_REQUIRE(ctx, yuv + ny <= rgb || rgb + nr <= yuv, "%s: the source and destination must not overlap", kFn);
    AVX_REQUIRE(ctx, ((uintptr_t)yuv & (t.bps - 1)) == 0, "%s: 16-bit samples need a 2-byte aligned payload", kFn);
    AVX_REQUIRE(ctx, matrix == AVX_YUV_BT601 || matrix == AVX_YUV_BT709, "%s: matrix %d (0 bt601, 1 bt709)", kFn, matrix);
    AVX_REQUIRE(ctx, full_range == 0 || full_range == 1, "%s: full_range %d (0 limited, 1 full)", kFn, full_range);
    return AVX_OK;
}

// the vector path's condition: a 4:2:0 format at exactly 2 x 2, W % 32 == 0 (8 destination pixels per thread, Wd % 16 == 0), H even
bool half_vec(const Traits& t, const void* a, const void* b, int H, int W, int isx, int isy) {
    return t.sx == 1 && t.sy == 1 && isx == 2 && isy == 2 && W % 32 == 0 && H % 2 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

template <class F>
void launch_int(avx_ctx* ctx, hipStream_t s, bool vec, const uint8_t* yuv, uint8_t* rgb, int n, int H, int W, int Hd, int Wd, int isx, int isy,
                const DecC& c) {
    if constexpr (F::SX == 1 && F::SY == 1) {
        if (vec) {
            const size_t units = (size_t)n * (H / 2) * (W / 16);
            hipLaunchKernelGGL(k_yuv420_to_rgb_half_vec<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, c);
            return;
        }
    }
    const size_t units = (size_t)n * Hd * Wd;
    hipLaunchKernelGGL(k_yuv_to_rgb_area_int<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, Hd, Wd, isx, isy, c);
}

template <class F>
void launch_gen(avx_ctx* ctx, hipStream_t s, const uint8_t* yuv, uint8_t* rgb, int n, int H, int W, int Hd, int Wd, const AxisArea& ax,
                const AxisArea& ay, const DecC& c) {
    const size_t units = (size_t)n * Hd * Wd;
    hipLaunchKernelGGL(k_yuv_to_rgb_area_gen<F>, dim3(raw_grid(ctx, units)), dim3(kYT), 0, s, yuv, rgb, units, H, W, Hd, Wd, ax, ay, c);
}

}  // namespace

#define AVX_SCALE_DISPATCH(fmt, call)                 \
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

extern "C" int avx_yuv_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, int Wd,
                                        int matrix, int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    int rc = scale_check(ctx, fmt, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, matrix, full_range);
    if (rc) return rc;
    if (Hd == H && Wd == W)  // the 1 x 1 block is rintf(sum * 1.f): the plain decode, which has the wider kernels for it
        return avx_yuv_to_rgb_u8(ctx, fmt, yuv, rgb_hwc, n_frames, H, W, matrix, full_range, stream);
    // avx_resize_hwc's own test for the integer-ratio route
    const double sx = (double)W / Wd, sy = (double)H / Hd;
    const int isx = (int)std::lrint(sx), isy = (int)std::lrint(sy);
    const bool integer = std::fabs(sx - isx) < DBL_EPSILON && std::fabs(sy - isy) < DBL_EPSILON;
    AVX_REQUIRE(ctx, !integer || (size_t)isx * isy <= 65536, "%s: a %d x %d block is more than 65536 samples per output pixel", kFn, isx, isy);
    const Traits& t = kTraits[fmt];
    int d[6], e[10];
    avx_yuv_coefficients_d(matrix, full_range, t.depth, d, e);
    const DecC c = {d[0], d[1], d[2], d[3], d[4], d[5], 1 << (t.depth - 1)};
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (integer) {
        const bool vec = half_vec(t, yuv, rgb_hwc, H, W, isx, isy);
#define AVX_SCALE_INT(F) launch_int<F>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, isx, isy, c)
        AVX_SCALE_DISPATCH(fmt, AVX_SCALE_INT)
#undef AVX_SCALE_INT
    } else {
        avx_ws* ws = avx_workspace(ctx, s);
        if (!ws) return AVX_ERR_NOMEM;
        avx_area_tab tx{}, ty{};
        if ((rc = avx_geom_area_tables(ctx, ws, s, H, W, Hd, Wd, &tx, &ty))) return rc;
        const AxisArea ax{const_cast<int*>(tx.start), const_cast<int*>(tx.cnt), const_cast<float*>(tx.alpha), tx.maxcnt};
        const AxisArea ay{const_cast<int*>(ty.start), const_cast<int*>(ty.cnt), const_cast<float*>(ty.alpha), ty.maxcnt};
#define AVX_SCALE_GEN(F) launch_gen<F>(ctx, s, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, ax, ay, c)
        AVX_SCALE_DISPATCH(fmt, AVX_SCALE_GEN)
#undef AVX_SCALE_GEN
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
