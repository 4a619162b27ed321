// csrc/yuv_scale.hip -- raw video pixel formats -> interleaved RGB uint8 at a smaller size, in one launch per batch.
//
// The definition, byte for byte, is the chain it replaces: avx_yuv_to_rgb_u8 (yuv_raw.hip, §4.9) into a full-size RGB frame, then
// avx_resize_hwc(uint8, INTER_AREA) of that frame (geom.hip, resize_common.h).  The kernels restate both steps per destination
// pixel and never write the full-size frame: the integer-ratio walk of yuv_walks.h and this file's 2 x 2 vector kernel on DecStage
// (yuv_dec.h), the stage yuv_raw.hip decodes with, and this file's general-ratio kernel on dec_px; chroma replicated over its
// block.  No LDS, no scratch.  tests/test_yuv_scale_gpu.py holds them to the chain bit for bit.
#include "yuv_dec.h"
#include "yuv_walks.h"

namespace {

// the chroma pair of block r (row-major over the frame's chroma blocks) of frame `fr`, centred
template <class F>
__device__ __forceinline__ void load_uv(const typename F::T* fr, size_t ysz, size_t csz, size_t r, int cc, int& u, int& v) {
    if constexpr (F::IL) { u = (int)(fr[ysz + 2 * r] >> F::SH) - cc; v = (int)(fr[ysz + 2 * r + 1] >> F::SH) - cc; }
    else { u = (int)(fr[ysz + r] >> F::SH) - cc; v = (int)(fr[ysz + csz + r] >> F::SH) - cc; }
}

template <class F>
__global__ __launch_bounds__(kYT) void k_yuv_to_rgb_area_int(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H, int W,
                                                              int Hd, int Wd, int isx, int isy, DecC c) {
    walk_area_int<F>(yuv, rgb, units, H, W, Hd, Wd, isx, isy, DecStage{c});
}

// ---- 2 x 2 of the 4:2:0 formats, vector path: 8 destination pixels of one row per thread ----------------------------------------
// A destination pixel is exactly one chroma block, finished before the next begins so that only loaded words stay live (the shape
// of k_yuv420_hdr_to_rgb_half_vec; the sums are integers, so the order does not reach the bytes).  W % 32 == 0, H even, both
// buffers 16-byte aligned (half_vec): every run is aligned to its access.  Same sums, same (sum + 2) >> 2 as walk_area_int.
template <class F>
__global__ __launch_bounds__(kYT) void k_yuv420_to_rgb_half_vec(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                 int W, DecC c) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA, "4:2:0 only");
    const DecStage st{c};
    const Frame<F> L(H, W);
    const int Hd = H >> 1, Wd = W >> 1, ux = Wd >> 3;      // units per destination row
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * Hd);
        const int r = (int)(t - f * ux * Hd);
        const int dy = r / ux, x0 = (r - dy * ux) << 4;    // x0: the first source column
        const uint8_t* fr = yuv + f * L.fsz;
        int u[8], v[8], y0[16], y1[16];
        L.uv(fr, (size_t)dy * L.cw + (x0 >> 1), u, v);
        load_samples<T, 16, F::SH>(fr + ((size_t)(2 * dy) * W + x0) * sizeof(T), y0);
        load_samples<T, 16, F::SH>(fr + ((size_t)(2 * dy + 1) * W + x0) * sizeof(T), y1);
        RgbRun<8> out;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const DecStage::Chroma k = st.chroma(u[i], v[i]);
            const int ys[4] = {y0[2 * i], y0[2 * i + 1], y1[2 * i], y1[2 * i + 1]};
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t pr, pg, pb;
                st.px(ys[j], k, pr, pg, pb);
                sr += (int)pr; sg += (int)pg; sb += (int)pb;
            }
            out.put(i, (uint32_t)(sr + 2) >> 2, (uint32_t)(sg + 2) >> 2, (uint32_t)(sb + 2) >> 2);
        }
        out.store(rgb + ((f * Hd + dy) * (size_t)Wd + (x0 >> 1)) * 3);
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

extern "C" int avx_yuv_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, int Wd,
                                        int matrix, int full_range, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    int rc = sdr_check(ctx, kFn, fmt, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, matrix, full_range);
    if (rc) return rc;
    if (Hd == H && Wd == W)  // the 1 x 1 block is rintf(sum * 1.f): the plain decode, which has the wider kernels for it
        return avx_yuv_to_rgb_u8(ctx, fmt, yuv, rgb_hwc, n_frames, H, W, matrix, full_range, stream);
    const AreaRoute a = area_route(H, W, Hd, Wd);
    AVX_REQUIRE(ctx, !a.integer || (size_t)a.isx * a.isy <= 65536, "%s: a %d x %d block is more than 65536 samples per output pixel", kFn, a.isx, a.isy);
    const Traits& t = kTraits[fmt];
    const DecC c = dec_constants(matrix, full_range, t.depth);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (a.integer) {
        const bool vec = half_vec(t, yuv, rgb_hwc, H, W, a.isx, a.isy, 8);
#define AVX_SCALE_INT(F) launch_int<F>(ctx, s, vec, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, a.isx, a.isy, c)
        AVX_FMT_DISPATCH(fmt, AVX_SCALE_INT)
#undef AVX_SCALE_INT
    } else {
        AxisArea ax, ay;
        if ((rc = area_axes(ctx, s, H, W, Hd, Wd, &ax, &ay))) return rc;
#define AVX_SCALE_GEN(F) launch_gen<F>(ctx, s, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, ax, ay, c)
        AVX_FMT_DISPATCH(fmt, AVX_SCALE_GEN)
#undef AVX_SCALE_GEN
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
