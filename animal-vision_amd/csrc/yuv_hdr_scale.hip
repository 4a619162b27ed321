// csrc/yuv_hdr_scale.hip -- HDR video in at a smaller size: 10-bit BT.2020 PQ / HLG payloads -> tone-mapped SDR RGB uint8 of
// Hd x Wd, in one launch per batch.
//
// The definition, byte for byte, is the chain it replaces: avx_yuv_hdr_to_rgb_u8 (yuv_hdr.hip, §4.10) into a full-size RGB frame,
// then avx_resize_hwc(uint8, INTER_AREA) of that frame (geom.hip, resize_common.h).  The kernels restate both steps per destination
// pixel and never write the full-size frame: the integer-ratio walk of yuv_walks.h, the one yuv_scale.hip runs for the SDR decode
// (§4.11), on HdrStage (yuv_hdr_px.h), the stage yuv_hdr.hip decodes with; the 2 x 2 vector kernel and the general-ratio kernel are
// this file's own, on hdr_px (§4.13 says why: the latter restates k_yuv_to_rgb_area_gen's area_sum order and is kept in step with it).
// The decode returns uint8 codes and the reductions work on codes.  No scratch; the quantiser's 3 KiB of tables are the only LDS.
// tests/test_hdr_scale_gpu.py holds them to the chain bit for bit.
#include "yuv_hdr_px.h"
#include "yuv_walks.h"

namespace {

// the chroma terms of R', G', B' of block r (row-major over the frame's chroma blocks) of frame `fr`
template <class F>
__device__ __forceinline__ void load_terms(const HdrC& c, const typename F::T* fr, size_t ysz, size_t csz, size_t r, float& dr, float& dg,
                                           float& db) {
    int u, v;
    if constexpr (F::IL) { u = (int)(fr[ysz + 2 * r] >> F::SH); v = (int)(fr[ysz + 2 * r + 1] >> F::SH); }
    else { u = (int)(fr[ysz + r] >> F::SH); v = (int)(fr[ysz + csz + r] >> F::SH); }
    const float cb = (float)(u - 512) * c.cs, cr = (float)(v - 512) * c.cs;
    dr = c.rv * cr; dg = c.gu * cb + c.gv * cr; db = c.bu * cb;
}

template <class F, int TR>
__global__ __launch_bounds__(kYT) void k_yuv_hdr_to_rgb_area_int(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                  int W, int Hd, int Wd, int isx, int isy, HdrC c, Quant q) {
    static_assert(!F::LUMA && sizeof(typename F::T) == 2, "10-bit formats with chroma only");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    walk_area_int<F>(yuv, rgb, units, H, W, Hd, Wd, isx, isy, HdrStage<TR>{c, thr, (const uint8_t*)coarse_w, q.lo_key});
}

#ifndef AVX_HDR_HALF_PD
#define AVX_HDR_HALF_PD 8
#endif
constexpr int kHalfPD = AVX_HDR_HALF_PD;  // 8 or 4 destination pixels per thread; DESIGN §4.13 has the figures of both

// ---- 2 x 2 of yuv420p10le and p010le, vector path: PD destination pixels of one row per thread ----------------------------------
// An output pixel is exactly one chroma block: its chroma terms are formed once and shared by its four hdr_px.  W % (4 PD) == 0,
// H even, both buffers 16-byte aligned (half_vec): every run is aligned to its access.  Same sums, same (sum + 2) >> 2 as
// walk_area_int: byte-identical output.  The layout, the chroma fetch and the stores are written out here, not taken from
// yuv_walks.h: the instances sit at 70-71 VGPRs, just below the step from 7 waves to 6 (above 72), and on Frame one of them
// crosses it.
template <class F, int TR, int PD>
__global__ __launch_bounds__(kYT) void k_yuv420_hdr_to_rgb_half_vec(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                     int W, HdrC c, Quant q) {
    using T = typename F::T;
    static_assert(F::SX == 1 && F::SY == 1 && !F::LUMA && sizeof(T) == 2, "10-bit 4:2:0 only");
    static_assert(PD == 8 || PD == 4, "8 or 4 destination pixels per thread");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    const uint8_t* coarse = (const uint8_t*)coarse_w;
    const int Hd = H >> 1, Wd = W >> 1, ux = Wd / PD;      // units per destination row
    const size_t ysz = (size_t)H * W, csz = ysz >> 2, fsz = (ysz + 2 * csz) * sizeof(T);
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / ((size_t)ux * Hd);
        const int r = (int)(t - f * ux * Hd);
        const int dy = r / ux, ui = r - dy * ux, x0 = ui * (2 * PD);  // x0: the first source column
        const uint8_t* fr = yuv + f * fsz;
        int u[PD], v[PD];
        if constexpr (F::IL) {
            int uv[2 * PD];
            load_samples<T, 2 * PD, F::SH>(fr + (ysz + (size_t)dy * W + x0) * sizeof(T), uv);
#pragma unroll
            for (int j = 0; j < PD; ++j) { u[j] = uv[2 * j]; v[j] = uv[2 * j + 1]; }
        } else {
            const size_t co = (size_t)dy * (W >> 1) + (x0 >> 1);
            load_samples<T, PD, F::SH>(fr + (ysz + co) * sizeof(T), u);
            load_samples<T, PD, F::SH>(fr + (ysz + csz + co) * sizeof(T), v);
        }
        int y0[2 * PD], y1[2 * PD];
        load_samples<T, 2 * PD, F::SH>(fr + ((size_t)(2 * dy) * W + x0) * sizeof(T), y0);
        load_samples<T, 2 * PD, F::SH>(fr + ((size_t)(2 * dy + 1) * W + x0) * sizeof(T), y1);
        uint32_t b[3 * PD];                                // PD RGB pixels = 3 PD bytes
#pragma unroll
        for (int i = 0; i < PD; ++i) {                     // destination pixel i: one chroma block, four source pixels
            const float cb = (float)(u[i] - 512) * c.cs, cr = (float)(v[i] - 512) * c.cs;
            const float dr = c.rv * cr, dg = c.gu * cb + c.gv * cr, db = c.bu * cb;
            const int ys[4] = {y0[2 * i], y0[2 * i + 1], y1[2 * i], y1[2 * i + 1]};
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t pr, pg, pb;
                hdr_px<TR>(c, thr, coarse, q.lo_key, (float)(ys[k] - c.yo) * c.ys, dr, dg, db, pr, pg, pb);
                sr += (int)pr; sg += (int)pg; sb += (int)pb;
            }
            b[3 * i] = (uint32_t)(sr + 2) >> 2; b[3 * i + 1] = (uint32_t)(sg + 2) >> 2; b[3 * i + 2] = (uint32_t)(sb + 2) >> 2;
            // this pixel is finished here: past HLG's branches every pixel's quantiser otherwise sinks to the stores (256 VGPRs)
            if constexpr (TR == AVX_TRANSFER_HLG) asm volatile("" : "+v"(b[3 * i]), "+v"(b[3 * i + 1]), "+v"(b[3 * i + 2]));
        }
        uint32_t o[3 * PD / 4];
#pragma unroll
        for (int w = 0; w < 3 * PD / 4; ++w) o[w] = b[4 * w] | b[4 * w + 1] << 8 | b[4 * w + 2] << 16 | b[4 * w + 3] << 24;
        uint8_t* d = rgb + ((f * Hd + dy) * (size_t)Wd + (x0 >> 1)) * 3;  // a row starts at a multiple of 24 bytes (Wd % 8 == 0)
        if constexpr (PD == 8) {                           // 24 bytes at a multiple of 24: three 8-byte stores
#pragma unroll
            for (int k = 0; k < 3; ++k) ((uint2*)d)[k] = make_uint2(o[2 * k], o[2 * k + 1]);
        } else if ((ui & 1) == 0) {                        // 12 bytes at a multiple of 12: the 8-byte store goes where it is aligned
            *(uint2*)d = make_uint2(o[0], o[1]);
            *(uint32_t*)(d + 8) = o[2];
        } else {
            *(uint32_t*)d = o[0];
            *(uint2*)(d + 4) = make_uint2(o[1], o[2]);
        }
    }
}

// ---- any other ratio: one thread per destination pixel, the table cache's INTER_AREA tables ---------------------------------------
// Neighbouring destination pixels share source pixels and each thread decodes its own: hdr_px is recomputed (§4.13 has the ratio).
template <class F, int TR>
__global__ __launch_bounds__(kYT) void k_yuv_hdr_to_rgb_area_gen(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ rgb, size_t units, int H,
                                                                  int W, int Hd, int Wd, AxisArea ax, AxisArea ay, HdrC c, Quant q) {
    using T = typename F::T;
    static_assert(!F::LUMA && sizeof(T) == 2, "10-bit formats with chroma only");
    __shared__ uint32_t coarse_w[kCoarseTableBytes / 4];
    __shared__ float thr[256];
    stage_tables(q, coarse_w, thr);
    const uint8_t* coarse = (const uint8_t*)coarse_w;
    constexpr int BW = 1 << F::SX, BH = 1 << F::SY;
    const int cw = (W + BW - 1) >> F::SX, ch = (H + BH - 1) >> F::SY;
    const size_t ysz = (size_t)H * W, csz = (size_t)ch * cw, fsz = (ysz + 2 * csz) * sizeof(T);
    const size_t dsz = (size_t)Hd * Wd;
    for (size_t t = (size_t)blockIdx.x * kYT + threadIdx.x; t < units; t += (size_t)gridDim.x * kYT) {
        const size_t f = t / dsz;
        const size_t r = t - f * dsz;
        const int dy = (int)(r / Wd), dx = (int)(r - (size_t)dy * Wd);
        const T* fr = (const T*)(yuv + f * fsz);
        const int x0 = ax.start[dx], nx = ax.cnt[dx], y0 = ay.start[dy], ny = ay.cnt[dy];  // area_sum's walk (resize_common.h)
        const float* al = ax.alpha + (size_t)dx * ax.maxcnt;
        const float* be = ay.alpha + (size_t)dy * ay.maxcnt;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, dr = 0.f, dg = 0.f, db = 0.f;
        int cbx = -1, cby = -1;
        for (int j = 0; j < ny; ++j) {
            const int y = y0 + j;
            const T* yrow = fr + (size_t)y * W;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = 0; k < nx; ++k) {
                const int x = x0 + k;
                const int bx = x >> F::SX, by = y >> F::SY;
                if (bx != cbx || by != cby) {
                    cbx = bx; cby = by;
                    load_terms<F>(c, fr, ysz, csz, (size_t)by * cw + bx, dr, dg, db);
                }
                uint32_t pr, pg, pb;
                hdr_px<TR>(c, thr, coarse, q.lo_key, (float)((int)(yrow[x] >> F::SH) - c.yo) * c.ys, dr, dg, db, pr, pg, pb);
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
constexpr const char* kFn = "avx_yuv_hdr_to_rgb_scaled_u8";

struct Job { avx_ctx* ctx; hipStream_t s; const uint8_t* yuv; uint8_t* rgb; int n, H, W, Hd, Wd; HdrC c; Quant q; };

template <class F, int TR>
void launch_int(const Job& j, bool vec, int isx, int isy) {
    if constexpr (F::SX == 1 && F::SY == 1) {
        if (vec) {
            const size_t units = (size_t)j.n * (j.H / 2) * (j.W / (2 * kHalfPD));
            hipLaunchKernelGGL((k_yuv420_hdr_to_rgb_half_vec<F, TR, kHalfPD>), dim3(raw_grid(j.ctx, units)), dim3(kYT), 0, j.s, j.yuv, j.rgb, units,
                               j.H, j.W, j.c, j.q);
            return;
        }
    }
    const size_t units = (size_t)j.n * j.Hd * j.Wd;
    hipLaunchKernelGGL((k_yuv_hdr_to_rgb_area_int<F, TR>), dim3(raw_grid(j.ctx, units)), dim3(kYT), 0, j.s, j.yuv, j.rgb, units, j.H, j.W, j.Hd,
                       j.Wd, isx, isy, j.c, j.q);
}

template <class F, int TR>
void launch_gen(const Job& j, const AxisArea& ax, const AxisArea& ay) {
    const size_t units = (size_t)j.n * j.Hd * j.Wd;
    hipLaunchKernelGGL((k_yuv_hdr_to_rgb_area_gen<F, TR>), dim3(raw_grid(j.ctx, units)), dim3(kYT), 0, j.s, j.yuv, j.rgb, units, j.H, j.W, j.Hd,
                       j.Wd, ax, ay, j.c, j.q);
}

}  // namespace

extern "C" int avx_yuv_hdr_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, int Wd,
                                            int full_range, int transfer, int tonemap, double peak_nits, double sdr_white, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    int rc = hdr_check(ctx, kFn, fmt, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, full_range, transfer, tonemap, peak_nits, sdr_white);
    if (rc) return rc;
    if (Hd == H && Wd == W)  // the 1 x 1 block is rintf(sum * 1.f): the plain decode, which has the wider kernels for it
        return avx_yuv_hdr_to_rgb_u8(ctx, fmt, yuv, rgb_hwc, n_frames, H, W, full_range, transfer, tonemap, peak_nits, sdr_white, stream);
    const AreaRoute a = area_route(H, W, Hd, Wd);
    AVX_REQUIRE(ctx, !a.integer || (size_t)a.isx * a.isy <= 65536, "%s: a %d x %d block is more than 65536 samples per output pixel", kFn, a.isx, a.isy);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const Job j = {ctx, s, yuv, rgb_hwc, n_frames, H, W, Hd, Wd, hdr_constants(full_range, transfer, tonemap, peak_nits, sdr_white),
                   {ctx->d_enc_thr_f32, ctx->d_coarse_f32, ctx->coarse_lo_key[0]}};
    const bool pq = transfer == AVX_TRANSFER_PQ;
    if (a.integer) {
        const bool vec = half_vec(kTraits[fmt], yuv, rgb_hwc, H, W, a.isx, a.isy, kHalfPD);
#define AVX_HDR_INT(F) (pq ? launch_int<F, AVX_TRANSFER_PQ>(j, vec, a.isx, a.isy) : launch_int<F, AVX_TRANSFER_HLG>(j, vec, a.isx, a.isy))
        AVX_FMT10_DISPATCH(fmt, AVX_HDR_INT)
#undef AVX_HDR_INT
    } else {
        AxisArea ax, ay;
        if ((rc = area_axes(ctx, s, H, W, Hd, Wd, &ax, &ay))) return rc;
#define AVX_HDR_GEN(F) (pq ? launch_gen<F, AVX_TRANSFER_PQ>(j, ax, ay) : launch_gen<F, AVX_TRANSFER_HLG>(j, ax, ay))
        AVX_FMT10_DISPATCH(fmt, AVX_HDR_GEN)
#undef AVX_HDR_GEN
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
