// csrc/dichromat_wide.hip -- the wide view of any dichromat: binocular warp in front of the species' colour and post
// stages, batches of uint8 frames.  avx_dichromat_wide_u8 is defined, frame by frame, as
//     avx_binocular_warp_u8(frame, tables, Ho = H, Wo = W) -> float32 frame -> avx_dichromat_u8(desc with in_f32 = 1)
// for AVX_POST_NONE / _GAUSS / _ROWGAIN and is byte for byte equal to that chain: every sample goes through the chain's own
// statements (remap_common.h, dichromat_common.h) in its order.  AVX_POST_STREAK has no such chain; it is the night route's structure
// without the rod stage (planes -> avx_streak_planes_f32 -> chroma, encode) and is held to the oracle.  Two routes:
//
//   fused   k_wide_fused<T, COLOR, EPI>: k_cat_wide generalised over the compute type and the colour stage (float + matrix for the 19
//           species, double + L/M merge for Cat).  One 256-thread workgroup per TW x TH output tile of one frame:
//             phase 0  the 256 normalised byte values of this frame (from flags[f]); per column / row of the haloed tile the reflected
//                      output coordinate's rounded 1/32-px map value and weights
//             phase 1  every sample of the haloed tile from the uint8 source: warp, blend, decode, colour stage -> three planes in LDS
//             per channel: row pass -> LDS, symmetric column pass (the reference kernel's statements)
//             EPI      row gain and chroma compression need a pixel's three channels: the column pass leaves them in the dead A
//                      plane of its channel and an epilogue finishes the pixel; without either the column pass quantises at once
//             store    the uint8 tile -> HBM, dwords where the frame allows
//   planes  k_wide_front (warp, blend, decode, colour -> three float32 planes per frame in the stream workspace's scratch, the frame a
//           grid dimension) -> avx_planes_gaussian_blur_batch | avx_streak_planes_f32 per frame -> k_wide_back (row gain, chroma,
//           encode), a batch walked in groups whose planes fit 1 GiB.  float32 only: Cat's float64 tail always takes the fused route.
//
// k_any_gt1_frames finds each frame's "any byte > 1" flag (get_normalized_image) in front of either route.
#include <cstdlib>

#include "dichromat_common.h"
#include "remap_common.h"

using namespace avxk;

namespace {

constexpr int kWT = 256;
constexpr size_t kWideScratchCap = (size_t)1 << 30;

struct WideArgs {
    DichromatArgs d;  // in, out, n_frames, H, W, tiles, tile, r, M, Bk, alpha, one_minus_alpha, row gain, chroma, enc_thr, flags
    const float* xL; const float* xR; const float* ymap; const float* wL; const float* wR;  // device: W, W, H, W, W floats
    float* planes;        // planes route: what k_wide_front writes, 3 planes per frame
    const float* back;    // planes route: what k_wide_back reads (planes, or the post stage's output)
};

struct WideLds {
    size_t off_A, off_B, off_nlut, off_colw, off_colq, off_rowq, off_out, off_post, bytes;
    __host__ __device__ WideLds(int TW, int TH, int r, size_t ts) {
        const size_t AW = TW + 2 * r, AH = TH + 2 * r;
        off_A = 256 * ts;                                               // thr: T[256] at 0
        off_B = off_A + 3 * AH * AW * ts;                               // A: three haloed planes
        off_nlut = off_B + (r > 0 ? AH * (size_t)TW * ts : 0);          // B: one row-passed plane at a time
        off_colw = off_nlut + 256 * sizeof(float);
        off_colq = off_colw + 3 * AW * sizeof(float);                   // wl, wr, wsum per haloed column
        off_rowq = off_colq + 2 * AW * sizeof(int);                     // rounded xL, xR per haloed column
        off_out = off_rowq + AH * sizeof(int);                          // rounded ymap per haloed row
        off_post = (off_out + (size_t)TW * TH * 3 + 15) & ~(size_t)15;  // the uint8 tile
        bytes = off_post + 32;                                          // EPI: the epilogue's arguments (a WidePost)
    }
};

// flags[f] = 1 when frame f holds a byte above 1 (get_normalized_image divides that frame by 255): all frames of the batch in
// one launch, 16 bytes per load where the frame's alignment allows.  flags are zero on entry.
__global__ __launch_bounds__(kWT) void k_any_gt1_frames(const uint8_t* __restrict__ in, size_t nbytes, int blocks_per_frame, uint32_t* flags) {
    const int f = blockIdx.x / blocks_per_frame, b = blockIdx.x - f * blocks_per_frame;
    const uint8_t* p = in + (size_t)f * nbytes;
    size_t head = (16 - ((uintptr_t)p & 15u)) & 15u;
    head = head < nbytes ? head : nbytes;
    const size_t nvec = (nbytes - head) / 16, tail = head + nvec * 16;
    const size_t t = (size_t)b * kWT + threadIdx.x, step = (size_t)blocks_per_frame * kWT;
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

// the colour stage of one decoded sample in the compute type (the reference kernel's statements, dichromat.hip)
template <typename T, int COLOR>
__device__ __forceinline__ void wide_colour(float c0, float c1, float c2, const DichromatArgs& a, T& o0, T& o1, T& o2) {
    if constexpr (COLOR == AVX_COLOR_MATRIX) {
        o0 = fma_t(c2, a.M[2], fma_t(c1, a.M[1], c0 * a.M[0]));
        o1 = fma_t(c2, a.M[5], fma_t(c1, a.M[4], c0 * a.M[3]));
        o2 = fma_t(c2, a.M[8], fma_t(c1, a.M[7], c0 * a.M[6]));
    } else {
        cat_merge_stage<T>(c0, c1, c2, a, o0, o1, o2);
    }
}

// apply_s_cone_vertical_gain and apply_chroma_compression of one pixel (the reference kernel's statements)
struct WidePost {
    const float* row_gain;  // NULL: no row gain
    int row_gain_clamp, chroma_enable;
    float chroma_keep;
    __host__ __device__ explicit WidePost(const DichromatArgs& a)
        : row_gain(a.post_mode == AVX_POST_ROWGAIN ? a.row_gain : nullptr), row_gain_clamp(a.row_gain_clamp), chroma_enable(a.chroma_enable), chroma_keep(a.chroma_keep) {}
};

static_assert(sizeof(WidePost) <= 32, "WideLds keeps 32 bytes for it");

template <typename T>
__device__ __forceinline__ void wide_post_point(const WidePost& p, int gy, T (&v)[3]) {
    if (p.row_gain) {
        T b = v[2] * (T)p.row_gain[gy];
        if (p.row_gain_clamp) b = b < (T)0 ? (T)0 : (b > (T)1 ? (T)1 : b);
        v[2] = b;
    }
    if (p.chroma_enable) {
        const T gray = ((v[0] + v[1]) + v[2]) / (T)3;
        const T keep = (T)p.chroma_keep;
        v[0] = gray + (v[0] - gray) * keep;
        v[1] = gray + (v[1] - gray) * keep;
        v[2] = gray + (v[2] - gray) * keep;
    }
}

template <typename T, int COLOR, bool EPI>
__global__ __launch_bounds__(kWT) void k_wide_fused(WideArgs w, Taps<T> taps) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const DichromatArgs& a = w.d;
    const int r = a.r, TW = a.TW, TH = a.TH;
    const int AW = TW + 2 * r, AH = TH + 2 * r;
    const WideLds L(TW, TH, r, sizeof(T));
    T* thr = reinterpret_cast<T*>(smem_raw);
    T* A = reinterpret_cast<T*>(smem_raw + L.off_A);
    T* Bm = reinterpret_cast<T*>(smem_raw + L.off_B);
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
    for (int i = tid; i < 256; i += kWT) {
        thr[i] = reinterpret_cast<const T*>(a.enc_thr)[i];
        nlut[i] = remap_norm((float)i, norm);
    }
    for (int lx = tid; lx < AW; lx += kWT) {
        const int gx = reflect101(x0 - r + lx, a.W);  // the halo is the reflected OUTPUT sample, as in the chain's second kernel
        const float wl = w.wL[gx], wr = w.wR[gx];
        colq[lx] = remap_round(w.xL[gx]);
        colq[AW + lx] = remap_round(w.xR[gx]);
        colw[lx] = wl;
        colw[AW + lx] = wr;
        colw[2 * AW + lx] = (wl + wr) + 1e-8f;
    }
    for (int ly = tid; ly < AH; ly += kWT) rowq[ly] = remap_round(w.ymap[reflect101(y0 - r + ly, a.H)]);
    if constexpr (EPI) {  // the epilogue's arguments wait in LDS: held in scalar registers across the passes, next to 33 taps, they spill
        if (tid == 0) *reinterpret_cast<WidePost*>(smem_raw + L.off_post) = WidePost(a);
    }
    __syncthreads();
    // ---- phase 1: warp + blend + decode + colour stage -> A planes --------------------------------------------------------
    auto nrm = [nlut](uint8_t b) { return nlut[b]; };
    for (int i = tid; i < AH * AW; i += kWT) {
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
        T o0, o1, o2;
        wide_colour<T, COLOR>(c0, c1, c2, a, o0, o1, o2);
        A[i] = o0;
        A[AH * AW + i] = o1;
        A[2 * AH * AW + i] = o2;
    }
    __syncthreads();
    // ---- per channel: row pass, column pass (the reference kernel's statements) --------------------------------------------
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        if (r > 0) {
            const int n = 2 * r + 1;
            for (int i = tid; i < AH * TW; i += kWT) {
                const int ly = i / TW, x = i - ly * TW;
                const T* row = A + (c * AH + ly) * AW + x;
                T s = row[0] * taps.k[0];
                for (int j = 1; j < n; ++j) s = fma_t(row[j], taps.k[j], s);
                Bm[i] = s;
            }
            __syncthreads();
        }
        if (!EPI || r > 0) {  // (EPI with r == 0: the pixel's three values are where the epilogue reads them already)
            for (int i = tid; i < TH * TW; i += kWT) {
                const int y = i / TW, x = i - y * TW;
                T s;
                if (r > 0) {
                    const T* col = Bm + (y + r) * TW + x;
                    s = col[0] * taps.k[r];
                    for (int j = 1; j <= r; ++j) s = fma_t(col[j * TW] + col[-j * TW], taps.k[r + j], s);
                } else {
                    s = A[(c * AH + y) * AW + x];
                }
                if constexpr (EPI) A[c * AH * AW + i] = s;  // plane c is dead once its row pass has run: TH * TW <= AH * AW
                else OUT[i * 3 + c] = (uint8_t)quantize<T>(s, thr);
            }
            __syncthreads();  // Bm is rewritten by the next channel; A / OUT are read below
        }
    }
    if constexpr (EPI) {  // ---- row gain, chroma compression, quantise: one pixel per thread step -------------------------------
        const WidePost post = *reinterpret_cast<const WidePost*>(smem_raw + L.off_post);
        for (int i = tid; i < TH * TW; i += kWT) {
            const int y = i / TW, x = i - y * TW;
            const int gy = y0 + y;
            if (gy >= a.H || x0 + x >= a.W) continue;  // never stored; row_gain holds H entries
            T v[3] = {A[i], A[AH * AW + i], A[2 * AH * AW + i]};  // (r == 0: AW == TW, the colour stage's own planes)
            wide_post_point<T>(post, gy, v);
            OUT[i * 3] = (uint8_t)quantize<T>(v[0], thr);
            OUT[i * 3 + 1] = (uint8_t)quantize<T>(v[1], thr);
            OUT[i * 3 + 2] = (uint8_t)quantize<T>(v[2], thr);
        }
        __syncthreads();
    }
    // ---- store the uint8 tile ---------------------------------------------------------------------------------------------
    const int tw = a.W - x0 < TW ? a.W - x0 : TW;  // valid columns / rows of this tile
    const int th = a.H - y0 < TH ? a.H - y0 : TH;
    if (((a.W & 3) == 0) && (((uintptr_t)fout & 3u) == 0)) {  // TW % 4 == 0 (host): every row segment is whole dwords
        const int dpr = tw * 3 / 4;
        for (int i = tid; i < th * dpr; i += kWT) {
            const int y = i / dpr, d = i - y * dpr;
            reinterpret_cast<uint32_t*>(fout + ((size_t)(y0 + y) * a.W + x0) * 3)[d] = reinterpret_cast<const uint32_t*>(OUT + (size_t)y * TW * 3)[d];
        }
    } else {
        const int bpr = tw * 3;
        for (int i = tid; i < th * bpr; i += kWT) {
            const int y = i / bpr, b = i - y * bpr;
            fout[((size_t)(y0 + y) * a.W + x0) * 3 + b] = OUT[(size_t)y * TW * 3 + b];
        }
    }
}

// ---- planes route ---------------------------------------------------------------------------------------------------------------
// One output pixel per thread step, the frame is blockIdx.y: warp, blend, decode, matrix colour stage -> three float32 planes.
__global__ __launch_bounds__(kWT) void k_wide_front(WideArgs w) {
    __shared__ float nlut[256];
    const DichromatArgs& a = w.d;
    const int f = blockIdx.y;
    const float norm = a.flags[f] ? 255.f : 1.f;
    for (int i = threadIdx.x; i < 256; i += kWT) nlut[i] = remap_norm((float)i, norm);
    __syncthreads();
    auto nrm = [&](uint8_t b) { return nlut[b]; };
    const unsigned npx = (unsigned)a.H * (unsigned)a.W;  // the host checks H * W < 2^31
    const uint8_t* fin = a.in + (size_t)f * npx * 3;
    float* dst = w.planes + (size_t)f * npx * 3;
    for (unsigned p = blockIdx.x * kWT + threadIdx.x; p < npx; p += gridDim.x * kWT) {
        const int y = (int)(p / (unsigned)a.W), x = (int)(p - (unsigned)y * (unsigned)a.W);
        const float wl = w.wL[x], wr = w.wR[x];
        const float wsum = (wl + wr) + 1e-8f;
        const int fy = remap_round(w.ymap[y]);
        float l[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f};
        if (wl != 0.f) remap_px_q(fin, a.H, a.W, remap_round(w.xL[x]), fy, nrm, l);  // (a zero weight: as k_wide_fused)
        if (wr != 0.f) remap_px_q(fin, a.H, a.W, remap_round(w.xR[x]), fy, nrm, rr);
        const float c0 = srgb_eotf_f32(binocular_blend(l[0], rr[0], wl, wr, wsum));
        const float c1 = srgb_eotf_f32(binocular_blend(l[1], rr[1], wl, wr, wsum));
        const float c2 = srgb_eotf_f32(binocular_blend(l[2], rr[2], wl, wr, wsum));
        float o0, o1, o2;
        wide_colour<float, AVX_COLOR_MATRIX>(c0, c1, c2, a, o0, o1, o2);
        dst[p] = o0; dst[npx + p] = o1; dst[2 * (size_t)npx + p] = o2;
    }
}

// row gain, chroma compression and the float32 threshold encode of the post stage's planes -> uint8 HWC
__global__ __launch_bounds__(kWT) void k_wide_back(WideArgs w) {
    __shared__ float thr[256];
    const DichromatArgs& a = w.d;
    const int f = blockIdx.y;
    for (int i = threadIdx.x; i < 256; i += kWT) thr[i] = reinterpret_cast<const float*>(a.enc_thr)[i];
    __syncthreads();
    const unsigned npx = (unsigned)a.H * (unsigned)a.W;
    const float* src = w.back + (size_t)f * npx * 3;
    uint8_t* fout = a.out + (size_t)f * npx * 3;
    const WidePost post(a);
    for (unsigned p = blockIdx.x * kWT + threadIdx.x; p < npx; p += gridDim.x * kWT) {
        const int gy = (int)(p / (unsigned)a.W);
        float v[3] = {src[p], src[npx + p], src[2 * (size_t)npx + p]};
        wide_post_point<float>(post, gy, v);
        uint8_t* q = fout + (size_t)p * 3;
        q[0] = (uint8_t)quantize<float>(v[0], thr);
        q[1] = (uint8_t)quantize<float>(v[1], thr);
        q[2] = (uint8_t)quantize<float>(v[2], thr);
    }
}

bool parse_tile(const char* e, int& TW, int& TH) {
    int tw = 0, th = 0;
    if (!e || sscanf(e, "%dx%d", &tw, &th) != 2 || tw < 4 || tw > 256 || (tw & 3) || th < 1 || th > 256) return false;
    TW = tw; TH = th;
    return true;
}

template <typename T, int COLOR>
int launch_fused(avx_ctx* ctx, const char* who, WideArgs& w, const avx_dichromat_desc* d, const char* tile_env, hipStream_t s) {
    DichromatArgs& a = w.d;
    // the tile; the environment switches are for tuning and tests only
    int TW = 32, TH = 16;
    if (sizeof(T) == 4 && a.r <= 8) TH = 32;  // float32: measured at r = 0, 3, 8 and 14
    if (!parse_tile(getenv(tile_env), TW, TH) && strcmp(tile_env, "AVX_WIDE_TILE") != 0) parse_tile(getenv("AVX_WIDE_TILE"), TW, TH);
    while (WideLds(TW, TH, a.r, sizeof(T)).bytes > 160 * 1024 && TH > 4) TH /= 2;
    AVX_REQUIRE(ctx, WideLds(TW, TH, a.r, sizeof(T)).bytes <= 160 * 1024, "%s: ksize %d too large for LDS", who, d->ksize);
    a.TW = TW; a.TH = TH;
    a.tiles_x = (a.W + TW - 1) / TW;
    a.tiles_y = (a.H + TH - 1) / TH;
    const long long total = (long long)a.tiles_x * a.tiles_y * a.n_frames;
    AVX_REQUIRE(ctx, total < (1LL << 31), "%s: batch too large", who);
    Taps<T> taps;
    for (int i = 0; i < AVX_MAX_KSIZE; ++i) taps.k[i] = (T)0;
    if (a.r > 0)
        for (int i = 0; i < d->ksize; ++i) taps.k[i] = (T)d->taps_host[i];  // getGaussianKernel: double -> ktype
    const size_t lds = WideLds(TW, TH, a.r, sizeof(T)).bytes;
    const bool epi = a.post_mode == AVX_POST_ROWGAIN || a.chroma_enable;
    auto k = epi ? k_wide_fused<T, COLOR, true> : k_wide_fused<T, COLOR, false>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)total), dim3(kWT), lds, s, w, taps);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

int launch_planes(avx_ctx* ctx, avx_ws* ws, WideArgs& w, const avx_dichromat_desc* d, hipStream_t s, void* stream) {
    DichromatArgs& a = w.d;
    const bool planes_post = d->post_mode == AVX_POST_GAUSS || d->post_mode == AVX_POST_STREAK;
    const size_t npx = (size_t)a.H * a.W;
    const size_t frame_bytes = sizeof(float) * 3 * npx * (planes_post ? 2 : 1);
    const size_t fit = kWideScratchCap / frame_bytes;
    int group = (int)(fit < 1 ? 1 : fit > AVX_EW_MAX_FRAMES ? AVX_EW_MAX_FRAMES : fit);
    if (const char* e = getenv("AVX_WIDE_GROUP")) {  // tests: reach the walk at small sizes
        const int v = atoi(e);
        if (v >= 1) group = v < AVX_EW_MAX_FRAMES ? v : AVX_EW_MAX_FRAMES;
    }
    const int n_frames = a.n_frames;
    if (group > n_frames) group = n_frames;
    { const int rc = avx_ensure_scratch(ctx, ws, frame_bytes * (size_t)group); if (rc) return rc; }
    float* p0 = (float*)ws->d_scratch;
    float* p1 = p0 + (size_t)group * 3 * npx;
    w.planes = p0;
    w.back = planes_post ? p1 : p0;
    const uint8_t* in = a.in;
    uint8_t* out = a.out;
    uint32_t* flags = a.flags;
    const unsigned want = (unsigned)((npx + kWT - 1) / kWT), cap = (unsigned)ctx->num_cus * 16u;
    const unsigned gx = want < cap ? want : cap;
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int n = n_frames - f0 < group ? n_frames - f0 : group;
        a.in = in + (size_t)f0 * 3 * npx;
        a.out = out + (size_t)f0 * 3 * npx;
        a.flags = flags + f0;
        a.n_frames = n;
        hipLaunchKernelGGL(k_wide_front, dim3(gx, (unsigned)n), dim3(kWT), 0, s, w);
        AVX_HIP(ctx, hipGetLastError());
        if (d->post_mode == AVX_POST_GAUSS) {
            const int rc = avx_planes_gaussian_blur_batch(ctx, p0, 3 * npx, p1, 3 * npx, n, 3, a.H, a.W, d->ksize, d->taps_host, 0, stream);
            if (rc) return rc;
        } else if (d->post_mode == AVX_POST_STREAK) {
            for (int f = 0; f < n; ++f) {
                const int rc = avx_streak_planes_f32(ctx, p0 + (size_t)f * 3 * npx, p1 + (size_t)f * 3 * npx, a.H, a.W, d->streak_rows_host, d->streak_stride, stream);
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL(k_wide_back, dim3(gx, (unsigned)n), dim3(kWT), 0, s, w);
        AVX_HIP(ctx, hipGetLastError());
    }
    return AVX_OK;
}

// The route a float32 descriptor takes by default (measured): the fused kernel recomputes the warp and the powf of its
// halo, the planes route moves 24 B/px (48 with a blur) more and recomputes nothing.
bool planes_by_default(const avx_dichromat_desc* d, int r) {
    if (d->post_mode == AVX_POST_STREAK) return true;
    return d->post_mode == AVX_POST_GAUSS && r >= 1;
}

}  // namespace

int avx_blocks_per_frame(avx_ctx* ctx, size_t items, int n_frames) {
    size_t want = (items + kWT - 1) / kWT, cap = ((size_t)ctx->num_cus * 16 + n_frames - 1) / n_frames;
    if (cap < 1) cap = 1;
    return (int)(want < cap ? (want ? want : 1) : cap);
}

// What both entries run once their own checks have passed: the flags pass, then one of the routes.  `who` names the entry in errors.
int avx_wide_run(avx_ctx* ctx, const char* who, const char* tile_env, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W,
                 const avx_dichromat_desc* d, const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream) {
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    const bool cat = d->color_mode == AVX_COLOR_CAT_MERGE;
    WideArgs w{};
    DichromatArgs& a = w.d;
    a.r = d->post_mode == AVX_POST_GAUSS ? d->ksize / 2 : 0;
    a.in = in_hwc_u8; a.out = out_hwc_u8; a.n_frames = n_frames; a.H = H; a.W = W;
    AVX_REQUIRE(ctx, (size_t)H * W < ((size_t)1 << 31), "%s: batch too large", who);
    if (!cat) {
        for (int i = 0; i < 9; ++i) a.M[i] = d->matrix[i];
        a.enc_thr = ctx->d_enc_thr_f32;
    } else {
        static const float kRgbToLms[9] = {0.31399022f, 0.63951294f, 0.04649755f, 0.15537241f, 0.75789446f, 0.08670142f, 0.01775239f, 0.10944209f, 0.87256922f};
        static const double kLmsToRgb[9] = {5.472213, -4.6419606, 0.16963711, -1.125242, 2.2931712, -0.16789523, 0.02980164, -0.19318072, 1.1636479};
        for (int i = 0; i < 9; ++i) { a.M[i] = kRgbToLms[i]; a.Bk[i] = kLmsToRgb[i]; }  // animal_utils.py:56-63, :70-76 (as avx_dichromat_u8)
        a.alpha = d->cat_alpha;
        a.one_minus_alpha = d->cat_beta;
        a.enc_thr = ctx->d_enc_thr_f64;
    }
    a.post_mode = d->post_mode;
    a.chroma_enable = d->chroma_enable;
    a.chroma_keep = d->chroma_keep;
    if (d->post_mode == AVX_POST_ROWGAIN) {  // (uploaded when the bytes differ from the last table only)
        const int rcu = avx_upload_row_table(ctx, ws, d->row_gain_host, sizeof(float) * (size_t)H, s);
        if (rcu) return rcu;
        a.row_gain = ws->d_row_gain;
        a.row_gain_clamp = d->row_gain_clamp;
    }
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
    bool planes = !cat && planes_by_default(d, a.r);
    if (const char* e = getenv("AVX_WIDE_ROUTE")) {  // tuning and tests; the streak species have no fused form, Cat's float64 tail no planes
        if (!cat && d->post_mode != AVX_POST_STREAK && !strcmp(e, "fused")) planes = false;
        if (!cat && !strcmp(e, "planes")) planes = true;
    }
    AVX_HIP(ctx, hipMemsetAsync(a.flags, 0, sizeof(uint32_t) * n_frames, s));
    const size_t nbytes = (size_t)H * W * 3;
    const int bpf = avx_blocks_per_frame(ctx, nbytes / 64 + 1, n_frames);  // ~4 16-byte loads per thread
    AVX_REQUIRE(ctx, (long long)bpf * n_frames < (1LL << 31), "%s: batch too large", who);
    hipLaunchKernelGGL(k_any_gt1_frames, dim3((unsigned)(bpf * n_frames)), dim3(kWT), 0, s, in_hwc_u8, nbytes, bpf, a.flags);
    AVX_HIP(ctx, hipGetLastError());
    if (planes) return launch_planes(ctx, ws, w, d, s, stream);
    if (cat) return launch_fused<double, AVX_COLOR_CAT_MERGE>(ctx, who, w, d, tile_env, s);
    return launch_fused<float, AVX_COLOR_MATRIX>(ctx, who, w, d, tile_env, s);
}

extern "C" int avx_dichromat_wide_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, const avx_dichromat_desc* d,
                                     const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, d != nullptr && d->struct_size == sizeof(avx_dichromat_desc), "avx_dichromat_wide_u8: desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, in_hwc_u8 && out_hwc_u8 && in_hwc_u8 != out_hwc_u8, "avx_dichromat_wide_u8: NULL or aliased frame pointer");
    AVX_REQUIRE(ctx, d_xL && d_xR && d_ymap && d_wL && d_wR, "avx_dichromat_wide_u8: NULL warp table pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_dichromat_wide_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, d->color_mode == AVX_COLOR_MATRIX || d->color_mode == AVX_COLOR_CAT_MERGE, "avx_dichromat_wide_u8: unknown color_mode %d", d->color_mode);
    AVX_REQUIRE(ctx, d->post_mode >= AVX_POST_NONE && d->post_mode <= AVX_POST_STREAK, "avx_dichromat_wide_u8: unknown post_mode %d", d->post_mode);
    if (d->post_mode == AVX_POST_GAUSS) {
        AVX_REQUIRE(ctx, d->ksize >= 1 && d->ksize <= AVX_MAX_KSIZE && (d->ksize & 1), "avx_dichromat_wide_u8: ksize %d must be odd, 1..%d", d->ksize, AVX_MAX_KSIZE);
        AVX_REQUIRE(ctx, d->taps_host != nullptr, "avx_dichromat_wide_u8: taps_host is NULL");
    }
    if (d->post_mode == AVX_POST_ROWGAIN) AVX_REQUIRE(ctx, d->row_gain_host != nullptr, "avx_dichromat_wide_u8: row_gain_host is NULL");
    if (d->post_mode == AVX_POST_STREAK)
        AVX_REQUIRE(ctx, d->color_mode == AVX_COLOR_MATRIX && d->streak_rows_host != nullptr && d->streak_stride >= 48,
                    "avx_dichromat_wide_u8: AVX_POST_STREAK needs AVX_COLOR_MATRIX and its row tables");
    if (n_frames == 0) return AVX_OK;
    return avx_wide_run(ctx, "avx_dichromat_wide_u8", "AVX_WIDE_TILE", in_hwc_u8, out_hwc_u8, n_frames, H, W, d, d_xL, d_xR, d_ymap, d_wL, d_wR, stream);
}
