// csrc/cat_wide.hip -- Cat's two frames for the stream (animals/cat.py:74-109), batches of uint8 frames:
//   avx_cat_wide_u8     the wide view in ONE launch: binocular warp (two remaps + cos^2 blend) -> float32 sRGB decode ->
//                       L/M-merge colour tail (float64) -> separable Gaussian (float64) -> encode.  Defined as, and byte for
//                       byte equal to, avx_binocular_warp_u8 -> avx_dichromat_u8(in_f32 = 1) frame by frame: every sample goes
//                       through that chain's own statements (remap_common.h, dichromat_common.h) in its order; what is gone is
//                       the 12 B/px float32 frame in between, the host tables per call and the stream synchronisations.
//   avx_center_zoom_u8  the baseline: cv2.resize(frame[y0:y0+ch, x0:x0+cw], (W, H), INTER_LINEAR) on uint8 (AVX_LINEAR_U8 with
//                       avx_resize_hwc's cached tables), the crop read in place through the frame's row stride.
//
// k_cat_wide: one 256-thread workgroup per TW x TH output tile of one frame (DESIGN 4.14 for the tile).
//   phase 0  per tile: the 256 normalised byte values of this frame (get_normalized_image's rule, from flags[f]), and for
//            every column / row of the haloed tile the reflected output coordinate's rounded 1/32-px map value and weights
//            (xL, xR, wL, wR depend on the column only, ymap on the row only)
//   phase 1  every sample of the haloed tile from the uint8 source: warp, blend, decode, colour stage -> three float64 planes in LDS
//   per channel: row pass -> LDS, symmetric column pass + quantise -> the uint8 tile in LDS (the reference kernel's statements)
//   store    the uint8 tile -> HBM, dwords where the frame allows
#include <cstdlib>

#include "dichromat_common.h"
#include "remap_common.h"
#include "resize_common.h"

using namespace avxk;

// geom.hip: the INTER_LINEAR tables avx_resize_hwc runs an H x W -> Hd x Wd resize with, out of the workspace's cache
int avx_geom_linear_tables(avx_ctx* ctx, avx_ws* ws, hipStream_t s, int H, int W, int Hd, int Wd, avx_lin_tab* ax, avx_lin_tab* ay);

namespace {

constexpr int kCT = 256;

struct CatWideArgs {
    DichromatArgs d;  // in, out, n_frames, H, W, tiles, tile, r, M, Bk, alpha, one_minus_alpha, enc_thr, flags
    const float* xL; const float* xR; const float* ymap; const float* wL; const float* wR;  // device: W, W, H, W, W floats
};

struct CatWideLds {
    size_t off_A, off_B, off_nlut, off_colw, off_colq, off_rowq, off_out, bytes;
    __host__ __device__ CatWideLds(int TW, int TH, int r) {
        const size_t AW = TW + 2 * r, AH = TH + 2 * r;
        off_A = 256 * sizeof(double);                                   // thr: double[256] at 0
        off_B = off_A + 3 * AH * AW * sizeof(double);                   // A: three haloed planes
        off_nlut = off_B + (r > 0 ? AH * (size_t)TW * sizeof(double) : 0);  // B: one row-passed plane at a time
        off_colw = off_nlut + 256 * sizeof(float);
        off_colq = off_colw + 3 * AW * sizeof(float);                   // wl, wr, wsum per haloed column
        off_rowq = off_colq + 2 * AW * sizeof(int);                     // rounded xL, xR per haloed column
        off_out = off_rowq + AH * sizeof(int);                          // rounded ymap per haloed row
        bytes = (off_out + (size_t)TW * TH * 3 + 15) & ~(size_t)15;     // the uint8 tile
    }
};

// flags[f] = 1 when frame f holds a byte above 1 (get_normalized_image divides that frame by 255): all frames of the batch in
// one launch, 16 bytes per load where the frame's alignment allows.  flags are zero on entry.
__global__ __launch_bounds__(kCT) void k_any_gt1_frames(const uint8_t* __restrict__ in, size_t nbytes, int blocks_per_frame, uint32_t* flags) {
    const int f = blockIdx.x / blocks_per_frame, b = blockIdx.x - f * blocks_per_frame;
    const uint8_t* p = in + (size_t)f * nbytes;
    size_t head = (16 - ((uintptr_t)p & 15u)) & 15u;
    head = head < nbytes ? head : nbytes;
    const size_t nvec = (nbytes - head) / 16, tail = head + nvec * 16;
    const size_t t = (size_t)b * kCT + threadIdx.x, step = (size_t)blocks_per_frame * kCT;
    uint32_t seen = 0;
    for (size_t i = t; i < head; i += step) seen |= p[i] >> 1;
    const uint4* q = reinterpret_cast<const uint4*>(p + head);
    for (size_t i = t; i < nvec; i += step) {
        const uint4 v = q[i];
        seen |= (v.x | v.y | v.z | v.w) & 0xfefefefeu;
    }
    for (size_t i = tail + t; i < nbytes; i += step) seen |= p[i] >> 1;
    if (seen) flags[f] = 1u;  // benign race: every writer stores the same value
}

__global__ __launch_bounds__(kCT) void k_cat_wide(CatWideArgs w, Taps<double> taps) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const DichromatArgs& a = w.d;
    const int r = a.r, TW = a.TW, TH = a.TH;
    const int AW = TW + 2 * r, AH = TH + 2 * r;
    const CatWideLds L(TW, TH, r);
    double* thr = reinterpret_cast<double*>(smem_raw);
    double* A = reinterpret_cast<double*>(smem_raw + L.off_A);
    double* Bm = reinterpret_cast<double*>(smem_raw + L.off_B);
    float* nlut = reinterpret_cast<float*>(smem_raw + L.off_nlut);
    float* colw = reinterpret_cast<float*>(smem_raw + L.off_colw);
    int* colq = reinterpret_cast<int*>(smem_raw + L.off_colq);
    int* rowq = reinterpret_cast<int*>(smem_raw + L.off_rowq);
    uint8_t* OUT = smem_raw + L.off_out;
    const int tid = threadIdx.x;
    const int tiles_per_frame = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x;  // the host launches exactly tiles_per_frame * n_frames workgroups
    const int f = tile / tiles_per_frame;
    const int t2 = tile - f * tiles_per_frame;
    const int ty = t2 / a.tiles_x, tx = t2 - ty * a.tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;
    const uint8_t* fin = a.in + (size_t)f * a.H * a.W * 3;
    uint8_t* fout = a.out + (size_t)f * a.H * a.W * 3;
    // ---- phase 0: per-frame, per-column and per-row values of this tile -------------------------------------------------
    const float norm = a.flags[f] ? 255.f : 1.f;  // all bytes <= 1: get_normalized_image does not divide
    for (int i = tid; i < 256; i += kCT) {
        thr[i] = reinterpret_cast<const double*>(a.enc_thr)[i];
        nlut[i] = remap_norm((float)i, norm);
    }
    for (int lx = tid; lx < AW; lx += kCT) {
        const int gx = reflect101(x0 - r + lx, a.W);  // the halo is the reflected OUTPUT sample, as in the chain's second kernel
        const float wl = w.wL[gx], wr = w.wR[gx];
        colq[lx] = remap_round(w.xL[gx]);
        colq[AW + lx] = remap_round(w.xR[gx]);
        colw[lx] = wl;
        colw[AW + lx] = wr;
        colw[2 * AW + lx] = (wl + wr) + 1e-8f;
    }
    for (int ly = tid; ly < AH; ly += kCT) rowq[ly] = remap_round(w.ymap[reflect101(y0 - r + ly, a.H)]);
    __syncthreads();
    // ---- phase 1: warp + blend + decode + colour stage -> A planes --------------------------------------------------------
    auto nrm = [nlut](uint8_t b) { return nlut[b]; };
    for (int i = tid; i < AH * AW; i += kCT) {
        const int ly = i / AW, lx = i - ly * AW;
        const int fy = rowq[ly];
        const float wl = colw[lx], wr = colw[AW + lx], wsum = colw[2 * AW + lx];
        float l[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f};
        // a sample is finite and >= 0, so under a zero weight its product is +-0 whatever it is: not fetched
        if (wl != 0.f) remap_px_q(fin, a.H, a.W, colq[lx], fy, nrm, l);
        if (wr != 0.f) remap_px_q(fin, a.H, a.W, colq[AW + lx], fy, nrm, rr);
        const float c0 = srgb_eotf_f32(binocular_blend(l[0], rr[0], wl, wr, wsum));
        const float c1 = srgb_eotf_f32(binocular_blend(l[1], rr[1], wl, wr, wsum));
        const float c2 = srgb_eotf_f32(binocular_blend(l[2], rr[2], wl, wr, wsum));
        double o0, o1, o2;
        cat_merge_stage<double>(c0, c1, c2, a, o0, o1, o2);
        A[i] = o0;
        A[AH * AW + i] = o1;
        A[2 * AH * AW + i] = o2;
    }
    __syncthreads();
    // ---- per channel: row pass, column pass + quantise (the reference kernel's statements) --------------------------------
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        if (r > 0) {
            const int n = 2 * r + 1;
            for (int i = tid; i < AH * TW; i += kCT) {
                const int ly = i / TW, x = i - ly * TW;
                const double* row = A + (c * AH + ly) * AW + x;
                double s = row[0] * taps.k[0];
                for (int j = 1; j < n; ++j) s = fma_t(row[j], taps.k[j], s);
                Bm[i] = s;
            }
            __syncthreads();
        }
        for (int i = tid; i < TH * TW; i += kCT) {
            const int y = i / TW, x = i - y * TW;
            double s;
            if (r > 0) {
                const double* col = Bm + (y + r) * TW + x;
                s = col[0] * taps.k[r];
                for (int j = 1; j <= r; ++j) s = fma_t(col[j * TW] + col[-j * TW], taps.k[r + j], s);
            } else {
                s = A[(c * AH + y) * AW + x];
            }
            OUT[i * 3 + c] = (uint8_t)quantize<double>(s, thr);
        }
        __syncthreads();  // Bm is rewritten by the next channel; OUT is read below
    }
    // ---- store the uint8 tile ---------------------------------------------------------------------------------------------
    const int tw = a.W - x0 < TW ? a.W - x0 : TW;  // valid columns / rows of this tile
    const int th = a.H - y0 < TH ? a.H - y0 : TH;
    if (((a.W & 3) == 0) && (((uintptr_t)fout & 3u) == 0)) {  // TW % 4 == 0 (host): every row segment is whole dwords
        const int dpr = tw * 3 / 4;
        for (int i = tid; i < th * dpr; i += kCT) {
            const int y = i / dpr, d = i - y * dpr;
            reinterpret_cast<uint32_t*>(fout + ((size_t)(y0 + y) * a.W + x0) * 3)[d] = reinterpret_cast<const uint32_t*>(OUT + (size_t)y * TW * 3)[d];
        }
    } else {
        const int bpr = tw * 3;
        for (int i = tid; i < th * bpr; i += kCT) {
            const int y = i / bpr, b = i - y * bpr;
            fout[((size_t)(y0 + y) * a.W + x0) * 3 + b] = OUT[(size_t)y * TW * 3 + b];
        }
    }
}

// One thread per destination pixel of one frame; the source is the crop inside the full frame (row stride W pixels).
__global__ __launch_bounds__(kCT) void k_center_zoom_u8(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int x0, int y0, int ch,
                                                       int blocks_per_frame, avx_lin_tab ax, avx_lin_tab ay) {
    const int f = blockIdx.x / blocks_per_frame, b = blockIdx.x - f * blocks_per_frame;
    const size_t frame = (size_t)H * W * 3;
    const uint8_t* src = in + (size_t)f * frame + ((size_t)y0 * W + x0) * 3;
    uint8_t* dst = out + (size_t)f * frame;
    const unsigned npx = (unsigned)H * (unsigned)W;  // the host checks H * W < 2^31
    for (unsigned p = (unsigned)b * kCT + threadIdx.x; p < npx; p += (unsigned)blocks_per_frame * kCT) {
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
#pragma unroll
        for (int c = 0; c < 3; ++c) AVX_LINEAR_U8(dst[(size_t)p * 3 + c], src, ch, W, 3, c, x, y, ax, ay);  // resize_common.h
    }
}

int blocks_per_frame_for(avx_ctx* ctx, size_t items, int n_frames) {
    size_t want = (items + kCT - 1) / kCT, cap = ((size_t)ctx->num_cus * 16 + n_frames - 1) / n_frames;
    if (cap < 1) cap = 1;
    return (int)(want < cap ? (want ? want : 1) : cap);
}

}  // namespace

extern "C" int avx_cat_wide_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, const avx_dichromat_desc* d,
                               const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, d != nullptr && d->struct_size == sizeof(avx_dichromat_desc), "avx_cat_wide_u8: desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, in_hwc_u8 && out_hwc_u8, "avx_cat_wide_u8: NULL frame pointer");
    AVX_REQUIRE(ctx, d_xL && d_xR && d_ymap && d_wL && d_wR, "avx_cat_wide_u8: NULL warp table pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_cat_wide_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, d->color_mode == AVX_COLOR_CAT_MERGE, "avx_cat_wide_u8: color_mode %d is not AVX_COLOR_CAT_MERGE", d->color_mode);
    AVX_REQUIRE(ctx, d->post_mode == AVX_POST_GAUSS || d->post_mode == AVX_POST_NONE, "avx_cat_wide_u8: post_mode %d is neither AVX_POST_GAUSS nor AVX_POST_NONE",
                d->post_mode);
    AVX_REQUIRE(ctx, !d->chroma_enable, "avx_cat_wide_u8: chroma compression is not part of Cat's tail");
    CatWideArgs w{};
    DichromatArgs& a = w.d;
    a.r = 0;
    if (d->post_mode == AVX_POST_GAUSS) {
        AVX_REQUIRE(ctx, d->ksize >= 1 && d->ksize <= AVX_MAX_KSIZE && (d->ksize & 1), "avx_cat_wide_u8: ksize %d must be odd, 1..%d", d->ksize, AVX_MAX_KSIZE);
        AVX_REQUIRE(ctx, d->taps_host != nullptr, "avx_cat_wide_u8: taps_host is NULL");
        a.r = d->ksize / 2;
    }
    if (n_frames == 0) return AVX_OK;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    // the tile; AVX_CAT_TILE=WxH is for tuning only
    int TW = 32, TH = 16;
    if (const char* e = getenv("AVX_CAT_TILE")) {
        int tw = 0, th = 0;
        if (sscanf(e, "%dx%d", &tw, &th) == 2 && tw >= 4 && tw <= 256 && (tw & 3) == 0 && th >= 1 && th <= 256) { TW = tw; TH = th; }
    }
    while (CatWideLds(TW, TH, a.r).bytes > 160 * 1024 && TH > 4) TH /= 2;
    AVX_REQUIRE(ctx, CatWideLds(TW, TH, a.r).bytes <= 160 * 1024, "avx_cat_wide_u8: ksize %d too large for LDS", d->ksize);
    a.in = in_hwc_u8; a.out = out_hwc_u8; a.n_frames = n_frames; a.H = H; a.W = W;
    a.TW = TW; a.TH = TH;
    a.tiles_x = (W + TW - 1) / TW;
    a.tiles_y = (H + TH - 1) / TH;
    const long long total = (long long)a.tiles_x * a.tiles_y * n_frames;
    AVX_REQUIRE(ctx, total < (1LL << 31) && (size_t)H * W < ((size_t)1 << 31), "avx_cat_wide_u8: batch too large");
    static const float kRgbToLms[9] = {0.31399022f, 0.63951294f, 0.04649755f, 0.15537241f, 0.75789446f, 0.08670142f, 0.01775239f, 0.10944209f, 0.87256922f};
    static const double kLmsToRgb[9] = {5.472213, -4.6419606, 0.16963711, -1.125242, 2.2931712, -0.16789523, 0.02980164, -0.19318072, 1.1636479};
    for (int i = 0; i < 9; ++i) { a.M[i] = kRgbToLms[i]; a.Bk[i] = kLmsToRgb[i]; }  // animal_utils.py:56-63, :70-76 (as avx_dichromat_u8)
    a.alpha = d->cat_alpha;
    a.one_minus_alpha = d->cat_beta;
    a.enc_thr = ctx->d_enc_thr_f64;
    a.post_mode = d->post_mode;
    if ((size_t)n_frames > ws->flags_cap) {  // grown as avx_dichromat_u8 grows it
        if (ws->d_flags) { AVX_HIP(ctx, hipStreamSynchronize(s)); AVX_HIP(ctx, hipFree(ws->d_flags)); }
        ws->d_flags = nullptr;
        ws->flags_cap = 0;
        size_t cap = (size_t)n_frames < 64 ? 64 : (size_t)n_frames;
        AVX_HIP(ctx, hipMalloc((void**)&ws->d_flags, sizeof(uint32_t) * cap));
        ws->flags_cap = cap;
    }
    a.flags = ws->d_flags;
    w.xL = d_xL; w.xR = d_xR; w.ymap = d_ymap; w.wL = d_wL; w.wR = d_wR;
    Taps<double> taps;
    for (int i = 0; i < AVX_MAX_KSIZE; ++i) taps.k[i] = 0.0;
    if (a.r > 0)
        for (int i = 0; i < d->ksize; ++i) taps.k[i] = d->taps_host[i];
    const size_t lds = CatWideLds(TW, TH, a.r).bytes;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k_cat_wide, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AVX_HIP(ctx, hipMemsetAsync(a.flags, 0, sizeof(uint32_t) * n_frames, s));
    const size_t nbytes = (size_t)H * W * 3;
    const int bpf = blocks_per_frame_for(ctx, nbytes / 64 + 1, n_frames);  // ~4 16-byte loads per thread
    AVX_REQUIRE(ctx, (long long)bpf * n_frames < (1LL << 31), "avx_cat_wide_u8: batch too large");
    hipLaunchKernelGGL(k_any_gt1_frames, dim3((unsigned)(bpf * n_frames)), dim3(kCT), 0, s, in_hwc_u8, nbytes, bpf, a.flags);
    hipLaunchKernelGGL(k_cat_wide, dim3((unsigned)total), dim3(kCT), lds, s, w, taps);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_center_zoom_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, int x0, int y0, int cw, int ch,
                                  void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, in_hwc_u8 && out_hwc_u8 && in_hwc_u8 != out_hwc_u8, "avx_center_zoom_u8: NULL or aliased frame pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_center_zoom_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, cw >= 1 && ch >= 1 && x0 >= 0 && y0 >= 0 && x0 <= W - cw && y0 <= H - ch,
                "avx_center_zoom_u8: crop %dx%d at (%d, %d) is empty or leaves the %dx%d frame", cw, ch, x0, y0, W, H);
    AVX_REQUIRE(ctx, (size_t)H * W < ((size_t)1 << 31), "avx_center_zoom_u8: frame larger than 2^31 pixels");
    if (n_frames == 0) return AVX_OK;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    avx_lin_tab ax{}, ay{};
    const int rc = avx_geom_linear_tables(ctx, ws, s, ch, cw, H, W, &ax, &ay);  // what avx_resize_hwc builds for (ch, cw) -> (H, W)
    if (rc) return rc;
    const int bpf = blocks_per_frame_for(ctx, (size_t)H * W, n_frames);
    AVX_REQUIRE(ctx, (long long)bpf * n_frames < (1LL << 31), "avx_center_zoom_u8: batch too large");
    hipLaunchKernelGGL(k_center_zoom_u8, dim3((unsigned)(bpf * n_frames)), dim3(kCT), 0, s, in_hwc_u8, out_hwc_u8, H, W, x0, y0, ch, bpf, ax, ay);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
