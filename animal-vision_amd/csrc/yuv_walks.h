// csrc/yuv_walks.h -- the kernel walks of the raw-video decode, once for the SDR integer decode (yuv_raw.hip, yuv_scale.hip: DESIGN
// §4.9, §4.11) and the HDR float decode (yuv_hdr.hip, yuv_hdr_scale.hip: §4.10, §4.13).  A walk is everything of a kernel but its
// colour: the index arithmetic, the frame layout, the chroma fetch, the reduction and the stores.  The colour is a Stage
// (DecStage, yuv_dec.h; HdrStage<TR>, yuv_hdr_px.h):
//   Stage::Chroma                     what a chroma block contributes to its pixels
//   st.chroma(u_raw, v_raw)           ... formed from the block's shifted samples
//   st.px(y_raw, chroma, r, g, b)     one luma sample -> three uint8 codes
// The __global__ kernels stay in their files: each stages what its stage needs and calls its walk (walk_blk, walk_strip,
// walk_area_int).  Kernels whose registers or time were worse on a shared walk keep their own loops: the two
// 2 x 2 vector kernels (the SDR one on Frame and RgbRun, the HDR one on nothing of this header) and the two general-ratio kernels.
// The host side below is what the scaled entry points share.  In an anonymous namespace, as yuv_formats.h: each translation unit
// gets its own copy.
#pragma once
#include <cfloat>
#include <cmath>

#include "resize_common.h"
#include "yuv_formats.h"

namespace {

// One frame of format F at H x W: the luma plane, then the chroma plane(s) of cw x ch blocks
template <class F>
struct Frame {
    using T = typename F::T;
    static constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    int W, cw, ch;
    size_t ysz, csz, fsz;  // luma samples, chroma blocks, bytes
    __device__ __forceinline__ Frame(int H, int W_)
        : W(W_), cw((W_ + BW - 1) >> F::SX), ch((H + BH - 1) >> F::SY), ysz((size_t)H * W_), csz((size_t)ch * cw),
          fsz((ysz + (F::LUMA ? 0 : 2 * csz)) * sizeof(T)) {}

    __device__ __forceinline__ int luma(const uint8_t* fr, int y, int x) const { return (int)(((const T*)fr)[(size_t)y * W + x] >> F::SH); }

    // the shifted chroma samples of the N blocks from block r on (row-major over the frame's blocks); a run of N > 1 is aligned
    template <int N>
    __device__ __forceinline__ void uv(const uint8_t* fr, size_t r, int (&u)[N], int (&v)[N]) const {
        const T* s = (const T*)fr;
        if constexpr (F::IL) {
            int p[2 * N];
            load_samples<T, 2 * N, F::SH>((const uint8_t*)(s + (ysz + 2 * r)), p);
#pragma unroll
            for (int j = 0; j < N; ++j) { u[j] = p[2 * j]; v[j] = p[2 * j + 1]; }
        } else {
            load_samples<T, N, F::SH>((const uint8_t*)(s + (ysz + r)), u);
            load_samples<T, N, F::SH>((const uint8_t*)(s + (ysz + csz + r)), v);
        }
    }

    // the chroma terms of block r; a frame without chroma has the stage's zero
    template <class Stage>
    __device__ __forceinline__ typename Stage::Chroma chroma(const Stage& st, const uint8_t* fr, size_t r) const {
        typename Stage::Chroma k{};
        if constexpr (!F::LUMA) {
            int u[1], v[1];
            uv(fr, r, u, v);
            k = st.chroma(u[0], v[0]);
        }
        return k;
    }
};

// A run of N RGB pixels on its way out: each pixel's codes are packed into the run's words as it is put, and the words are stored
// in 16-byte (N = 16: 48 bytes at a multiple of 48 from a 16-byte aligned buffer) or 8-byte (N = 8: 24 bytes at a multiple of 24) pieces
template <int N>
struct RgbRun {
    static_assert(N == 8 || N == 16, "24- or 48-byte runs");
    uint32_t o[3 * N / 4] = {};
    __device__ __forceinline__ void put(int i, uint32_t r, uint32_t g, uint32_t b) {
        const uint32_t c[3] = {r, g, b};
#pragma unroll
        for (int k = 0; k < 3; ++k) o[(3 * i + k) >> 2] |= c[k] << (8 * ((3 * i + k) & 3));
    }
    __device__ __forceinline__ void store(uint8_t* d) const {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if constexpr (N == 16) ((uint4*)d)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            else ((uint2*)d)[k] = make_uint2(o[2 * k], o[2 * k + 1]);
        }
    }
};

// ---- one thread per chroma block (1, 2 or 4 pixels), any size, sample-sized accesses ---------------------------------------------
template <class F, class Stage>
__device__ __forceinline__ void walk_blk(const uint8_t* yuv, uint8_t* rgb, size_t units, int H, int W, const Stage& st) {
    const Frame<F> L(H, W);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / L.csz;
        const size_t r = t - f * L.csz;
        const int by = (int)(r / L.cw), bx = (int)(r - (size_t)by * L.cw);
        const uint8_t* fr = yuv + f * L.fsz;
        const typename Stage::Chroma k = L.chroma(st, fr, r);
#pragma unroll
        for (int dy = 0; dy < L.BH; ++dy) {
            const int y = L.BH * by + dy;
            if (y >= H) break;
#pragma unroll
            for (int dx = 0; dx < L.BW; ++dx) {
                const int x = L.BW * bx + dx;
                if (x >= W) break;
                uint32_t pr, pg, pb;
                st.px(L.luma(fr, y, x), k, pr, pg, pb);
                uint8_t* d = rgb + (f * L.ysz + (size_t)y * W + x) * 3;
                d[0] = (uint8_t)pr; d[1] = (uint8_t)pg; d[2] = (uint8_t)pb;
            }
        }
    }
}

// ---- the 4:2:0 formats, one strip of PW x 2 pixels per thread, vector accesses (raw_vec's condition; W % PW == 0) ------------------
template <class F, class Stage, int PW>
__device__ __forceinline__ void walk_strip(const uint8_t* yuv, uint8_t* rgb, size_t units, int H, int W, const Stage& st) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA, "4:2:0 only");
    static_assert(PW == 8 || PW == 16, "8- or 16-pixel strips");
    const Frame<F> L(H, W);
    const int ux = W / PW, uy = H >> 1;                  // units per strip row, strips per frame
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * uy);
        const int r = (int)(t - f * ux * uy);
        const int sy = r / ux, x0 = (r - sy * ux) * PW;
        const uint8_t* fr = yuv + f * L.fsz;
        int u[PW / 2], v[PW / 2];
        L.uv(fr, (size_t)sy * L.cw + (x0 >> 1), u, v);
        typename Stage::Chroma k[PW / 2];
#pragma unroll
        for (int j = 0; j < PW / 2; ++j) k[j] = st.chroma(u[j], v[j]);
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            int y[PW];
            load_samples<T, PW, F::SH>(fr + ((size_t)(2 * sy + row) * W + x0) * sizeof(T), y);
            RgbRun<PW> out;
#pragma unroll
            for (int i = 0; i < PW; ++i) {
                uint32_t pr, pg, pb;
                st.px(y[i], k[i >> 1], pr, pg, pb);
                out.put(i, pr, pg, pb);
            }
            out.store(rgb + (f * L.ysz + (size_t)(2 * sy + row) * W + x0) * 3);
        }
    }
}

// ---- INTER_AREA, integer ratio (W = isx Wd, H = isy Hd): one thread per destination pixel, any size ------------------------------
// AVX_AREA_FAST for uint8 on the decoded codes: their integer sum (below 2^24: the bits resizeAreaFast_'s float sum holds, in
// any order), then (sum + 2) >> 2 for 2 x 2 and rintf((float)sum * (1.f / area)) otherwise.
template <class F, class Stage>
__device__ __forceinline__ void walk_area_int(const uint8_t* yuv, uint8_t* rgb, size_t units, int H, int W, int Hd,
                                              int Wd, int isx, int isy, const Stage& st) {
    using T = typename F::T;
    const Frame<F> L(H, W);
    const size_t dsz = (size_t)Hd * Wd;
    const bool two = isx == 2 && isy == 2;       // ResizeAreaFastVec, 8-bit 2 x 2
    const float scale = 1.f / (isx * isy);       // k_resize_area_fast_f32's
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / dsz;
        const size_t r = t - f * dsz;
        const int dy = (int)(r / Wd), dx = (int)(r - (size_t)dy * Wd);
        const T* fr = (const T*)(yuv + f * L.fsz);
        typename Stage::Chroma c{};
        int sr = 0, sg = 0, sb = 0, cbx = -1, cby = -1;
        for (int j = 0; j < isy; ++j) {
            const int y = dy * isy + j;          // < H: H = isy Hd
            const T* yrow = fr + (size_t)y * W;
            for (int k = 0; k < isx; ++k) {
                const int x = dx * isx + k;      // < W
                if constexpr (!F::LUMA) {
                    const int bx = x >> F::SX, by = y >> F::SY;
                    if (bx != cbx || by != cby) {  // fetched, and the terms formed, only when the chroma block changes
                        cbx = bx; cby = by;
                        c = L.chroma(st, (const uint8_t*)fr, (size_t)by * L.cw + bx);
                    }
                }
                uint32_t pr, pg, pb;
                st.px((int)(yrow[x] >> F::SH), c, pr, pg, pb);
                sr += (int)pr; sg += (int)pg; sb += (int)pb;
            }
        }
        uint8_t* d = rgb + t * 3;
        if (two) { d[0] = (uint8_t)((sr + 2) >> 2); d[1] = (uint8_t)((sg + 2) >> 2); d[2] = (uint8_t)((sb + 2) >> 2); }
        else { put_area(d, (float)sr * scale); put_area(d + 1, (float)sg * scale); put_area(d + 2, (float)sb * scale); }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// avx_resize_hwc's own test for the integer-ratio route
struct AreaRoute { bool integer; int isx, isy; };
AreaRoute area_route(int H, int W, int Hd, int Wd) {
    const double sx = (double)W / Wd, sy = (double)H / Hd;
    const int isx = (int)std::lrint(sx), isy = (int)std::lrint(sy);
    return {std::fabs(sx - isx) < DBL_EPSILON && std::fabs(sy - isy) < DBL_EPSILON, isx, isy};
}

// the table cache's INTER_AREA tables of H x W -> Hd x Wd, as the kernels take them
int area_axes(avx_ctx* ctx, hipStream_t s, int H, int W, int Hd, int Wd, AxisArea* ax, AxisArea* ay) {
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    avx_area_tab tx{}, ty{};
    if (const int rc = avx_geom_area_tables(ctx, ws, s, H, W, Hd, Wd, &tx, &ty)) return rc;
    *ax = {const_cast<int*>(tx.start), const_cast<int*>(tx.cnt), const_cast<float*>(tx.alpha), tx.maxcnt};
    *ay = {const_cast<int*>(ty.start), const_cast<int*>(ty.cnt), const_cast<float*>(ty.alpha), ty.maxcnt};
    return AVX_OK;
}

// the 2 x 2 vector kernels' condition, PD destination pixels per thread: a 4:2:0 format at exactly 2 x 2, W a multiple of the 2 PD source columns' 16-byte runs, H even
bool half_vec(const Traits& t, const void* a, const void* b, int H, int W, int isx, int isy, int PD) {
    return t.sx == 1 && t.sy == 1 && isx == 2 && isy == 2 && W % (4 * PD) == 0 && H % 2 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

}  // namespace
