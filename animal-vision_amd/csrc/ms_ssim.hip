// csrc/ms_ssim.hip -- MS-SSIM over five scales (Wang, Simoncelli, Bovik 2003): per frame, channel and scale the mean
// of the contrast-structure term cs and of the full SSIM l * cs of two uint8 RGB batches.  The product over the scales is formed on
// the host (metrics.MsSsim).
//
// Scale 0 is metrics.hip's tile kernel in its WITH_CS instantiation (avx_metrics_scale0_launch): the record avx_frame_metrics_u8
// writes, and the cs sum beside it.
// k_ms_pyramid: one workgroup per (32 x 32 source tile, frame).  The tile of both frames goes into LDS once (6 B/px; as aligned words
// where W is a multiple of 4 and both batches are 4-byte aligned, byte by byte otherwise: frames of an odd byte size put every later
// frame of a batch on an odd address).  Scale j + 1 is the 2 x 2 mean of scale j with a trailing odd row or column dropped, that is
// the sum of an origin-aligned 2^j x 2^j block divided by 4^j: the workgroup emits the 16 x 16, 8 x 8, 4 x 4 and 2 x 2 block sums of
// its tile for the three channels of both frames, as exact integers (<= 255 * 256) in uint16 planes, without touching a neighbour.
// k_ms_levels: one workgroup per (32 x 32 tile of window positions of one of the scales 1..4, channel, frame), the tiles of the four
// scales numbered through in one grid, on ssim_window.h's scheme in float64, without a histogram: the 42 x 42 patch of both planes
// goes into LDS as the 16-bit sums.  A sample is its sum times 4^-j, centred by 128: up to 8 fractional bits, so samples and
// products are exact in float64 and the moments, the window sums and the quotients are float64.  A workgroup sums two terms (cs,
// l * cs); k_ms_final sums the tiles of a (scale, channel, frame).
#include "ssim_window.h"

namespace {

constexpr int kRawS = kP + 2;          // samples of a patch row in LDS (44: every row starts on an 8-byte boundary)
constexpr int kMinSide = 176;          // scale 4 is floor(H / 16) x floor(W / 16) and needs one window position
constexpr int kS = 32;                 // pyramid: source tile side
constexpr int kSrcRow = kS * 3 + 4;    // bytes of a source tile row in LDS (100: a multiple of 4, rows land one bank apart)

// scales 1..4 as index 0..3.  A plane of scale k is h x w uint16 without row padding; plane (frame f, side s, channel c) lies at
// off + ((f * 2 + s) * 3 + c) * h * w (in uint16 units).
struct Levels {
    int h[4], w[4];
    size_t off[4];
    unsigned ntx[4];    // tiles per row
    unsigned t0[5];     // first tile of scale k in the grid; t0[4]: tiles in all
    double inv[4];      // 4^-(k + 1)
    double count[4];    // window positions
    double taps[kK];    // the window, normalised in float64
};

__device__ __forceinline__ uint16_t* level_plane(uint16_t* pyr, const Levels& lv, int k, int f, int side, int c) {
    return pyr + lv.off[k] + (size_t)((f * 2 + side) * 3 + c) * ((size_t)lv.h[k] * lv.w[k]);
}

// ---------------------------------------------------------------------------------------------------------------- the pyramid
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_ms_pyramid(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, Levels lv,
                                                         uint16_t* __restrict__ pyr) {
    __shared__ __attribute__((aligned(16))) uint8_t src[2][kS * kSrcRow];
    __shared__ uint16_t s1[6][16][16];
    __shared__ uint16_t s2[6][8][8];
    __shared__ uint16_t s3[6][4][4];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * kS, y0 = blockIdx.y * kS;
    const size_t row_bytes = (size_t)W * 3, fo = (size_t)f * H * row_bytes;
    // ---- source tile -> LDS; what lies outside the frame is zero and never part of a sum that is written ----
    if (VEC) {
        for (int i = tid; i < 2 * kS * (kS * 3 / 4); i += kThreads) {
            const int side = i / (kS * 24), r = (i / 24) % kS, d = i % 24;
            const size_t col = (size_t)x0 * 3 + d * 4;
            uint32_t v = 0;
            if (y0 + r < H && col < row_bytes) v = *reinterpret_cast<const uint32_t*>((side ? b : a) + fo + (size_t)(y0 + r) * row_bytes + col);
            *reinterpret_cast<uint32_t*>(&src[side][r * kSrcRow + d * 4]) = v;
        }
    } else {
        for (int i = tid; i < 2 * kS * kS * 3; i += kThreads) {
            const int side = i / (kS * 96), r = (i / 96) % kS, d = i % 96;
            const size_t col = (size_t)x0 * 3 + d;
            uint8_t v = 0;
            if (y0 + r < H && col < row_bytes) v = (side ? b : a)[fo + (size_t)(y0 + r) * row_bytes + col];
            src[side][r * kSrcRow + d] = v;
        }
    }
    __syncthreads();
    // ---- scale 1: one 2 x 2 block per thread, three channels of both frames ----
    {
        const int ly = tid >> 4, lx = tid & 15;
        const int Y = (y0 >> 1) + ly, X = (x0 >> 1) + lx;
        const bool in = Y < lv.h[0] && X < lv.w[0];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint8_t* r0 = &src[side][(2 * ly) * kSrcRow + 6 * lx];
            const uint8_t* r1 = r0 + kSrcRow;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned s = (unsigned)r0[c] + r0[3 + c] + r1[c] + r1[3 + c];
                s1[side * 3 + c][ly][lx] = (uint16_t)s;
                if (in) level_plane(pyr, lv, 0, f, side, c)[(size_t)Y * lv.w[0] + X] = (uint16_t)s;
            }
        }
    }
    __syncthreads();
    // ---- scales 2, 3, 4: 2 x 2 sums of the scale before, out of LDS ----
    for (int i = tid; i < 6 * 64; i += kThreads) {
        const int p = i >> 6, y = (i >> 3) & 7, x = i & 7;
        const unsigned s = (unsigned)s1[p][2 * y][2 * x] + s1[p][2 * y][2 * x + 1] + s1[p][2 * y + 1][2 * x] + s1[p][2 * y + 1][2 * x + 1];
        s2[p][y][x] = (uint16_t)s;
        const int Y = (y0 >> 2) + y, X = (x0 >> 2) + x;
        if (Y < lv.h[1] && X < lv.w[1]) level_plane(pyr, lv, 1, f, p / 3, p % 3)[(size_t)Y * lv.w[1] + X] = (uint16_t)s;
    }
    __syncthreads();
    if (tid < 6 * 16) {
        const int p = tid >> 4, y = (tid >> 2) & 3, x = tid & 3;
        const unsigned s = (unsigned)s2[p][2 * y][2 * x] + s2[p][2 * y][2 * x + 1] + s2[p][2 * y + 1][2 * x] + s2[p][2 * y + 1][2 * x + 1];
        s3[p][y][x] = (uint16_t)s;
        const int Y = (y0 >> 3) + y, X = (x0 >> 3) + x;
        if (Y < lv.h[2] && X < lv.w[2]) level_plane(pyr, lv, 2, f, p / 3, p % 3)[(size_t)Y * lv.w[2] + X] = (uint16_t)s;
    }
    __syncthreads();
    if (tid < 6 * 4) {
        const int p = tid >> 2, y = (tid >> 1) & 1, x = tid & 1;
        const unsigned s = (unsigned)s3[p][2 * y][2 * x] + s3[p][2 * y][2 * x + 1] + s3[p][2 * y + 1][2 * x] + s3[p][2 * y + 1][2 * x + 1];
        const int Y = (y0 >> 4) + y, X = (x0 >> 4) + x;
        if (Y < lv.h[3] && X < lv.w[3]) level_plane(pyr, lv, 3, f, p / 3, p % 3)[(size_t)Y * lv.w[3] + X] = (uint16_t)s;
    }
}

// ------------------------------------------------------------------------------------------------------------ scales 1..4
// Row item of NOUT adjacent positions of patch row `row`, from column x on (x even): the NOUT + 10 samples of both planes as the
// aligned words that hold them, scaled, centred by 128
template <int NOUT>
__device__ __forceinline__ void row_item(const uint16_t* raw_a, const uint16_t* raw_b, double* hp, const Taps<double>& tp, double inv, int row, int x) {
    constexpr int NS = NOUT + kK - 1;  // 14 or 12 samples: 7 or 6 aligned words
    const uint32_t* wa = reinterpret_cast<const uint32_t*>(raw_a + row * kRawS + x);
    const uint32_t* wb = reinterpret_cast<const uint32_t*>(raw_b + row * kRawS + x);
    double a[NS], b[NS];
#pragma unroll
    for (int i = 0; i < NS / 2; ++i) {
        const uint32_t va = wa[i], vb = wb[i];
        a[2 * i] = (double)(va & 0xffffu) * inv - 128.0, a[2 * i + 1] = (double)(va >> 16) * inv - 128.0;
        b[2 * i] = (double)(vb & 0xffffu) * inv - 128.0, b[2 * i + 1] = (double)(vb >> 16) * inv - 128.0;
    }
    row_moments<double, NOUT>(a, b, tp, hp, row, x);
}

// the tile's sums of cs and of l * cs into out[0], out[1] (thread 0)
template <bool EDGE>
__device__ __forceinline__ void level_tile(const uint16_t* __restrict__ pa, const uint16_t* __restrict__ pb, int H, int W, int x0, int y0, double inv,
                                           const Taps<double>& tp, uint16_t* raw_a, uint16_t* raw_b, double* hp, double* red, double* out, size_t out_stride) {
    const int tid = threadIdx.x;
    // ---- patch -> LDS; outside the plane: the centre (128 * 4^j <= 32768), never part of a valid window ----
    const uint16_t centre = (uint16_t)(128.0 / inv);
    for (int p = tid; p < kP * kP; p += kThreads) {
        const int py = p / kP, px = p - py * kP;
        uint16_t a = centre, b = centre;
        if (!EDGE || (y0 + py < H && x0 + px < W)) {
            const size_t i = (size_t)(y0 + py) * W + (x0 + px);
            a = pa[i], b = pb[i];
        }
        raw_a[py * kRawS + px] = a;
        raw_b[py * kRawS + px] = b;
    }
    __syncthreads();
    row_pass([&](auto n, int row, int x) { row_item<decltype(n)::value>(raw_a, raw_b, hp, tp, inv, row, x); });
    __syncthreads();
    const int col = tid & (kT - 1), seg = tid >> 5;
    double acc[5][4];
    column_pass(hp, tp, col, seg, acc);
    // ---- cs and l * cs.  E[x^2] - mu^2 in float64: its error is 2^-53 of mu^2 <= 2^14 against C2 = 58.5 ----
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double sum[2] = {};  // cs, l * cs
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (EDGE && !(x0 + col < W - (kK - 1) && y0 + seg * 4 + o < H - (kK - 1))) continue;
        const double ma = acc[0][o], mb = acc[1][o];
        const double va = acc[2][o] - ma * ma, vb = acc[3][o] - mb * mb, cab = acc[4][o] - ma * mb;
        const double ua = ma + 128.0, ub = mb + 128.0;
        const double l = (2.0 * (ua * ub) + C1) / ((ua * ua + ub * ub) + C1);
        const double cs = (2.0 * cab + C2) / ((va + vb) + C2);
        sum[0] += cs;
        sum[1] += l * cs;
    }
    workgroup_sum(sum, red);
    if (tid == 0) {
        out[0] = sum[0];
        out[out_stride] = sum[1];
    }
}

// grid (tiles of the four scales, 3 channels, frames); partials: [frame][channel][cs, l * cs][tile]
__global__ __launch_bounds__(kThreads) void k_ms_levels(const uint16_t* __restrict__ pyr, Levels lv, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) uint16_t raw_a[kP * kRawS];
    __shared__ __attribute__((aligned(16))) uint16_t raw_b[kP * kRawS];
    __shared__ __attribute__((aligned(16))) double hp[5 * kP * kT];
    __shared__ double red[2 * (kThreads / 64)];
    const unsigned t = blockIdx.x;
    const int c = blockIdx.y, f = blockIdx.z;
    int k = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (t >= lv.t0[i]) k = i;
    const unsigned tile = t - lv.t0[k], ntx = lv.ntx[k], ty = tile / ntx, tx = tile - ty * ntx;
    const int H = lv.h[k], W = lv.w[k];
    const int x0 = (int)tx * kT, y0 = (int)ty * kT;
    const size_t plane = (size_t)H * W;
    const uint16_t* pa = pyr + lv.off[k] + (size_t)((f * 2 + 0) * 3 + c) * plane;
    const uint16_t* pb = pyr + lv.off[k] + (size_t)((f * 2 + 1) * 3 + c) * plane;
    Taps<double> taps;
#pragma unroll
    for (int i = 0; i < kK; ++i) taps.w[i] = lv.taps[i];
    const size_t nt = lv.t0[4];
    double* out = partials + ((size_t)(f * 3 + c) * 2) * nt + t;
    if (x0 + kP <= W && y0 + kP <= H)  // the whole patch lies in the plane: no bounds tests
        level_tile<false>(pa, pb, H, W, x0, y0, lv.inv[k], taps, raw_a, raw_b, hp, red, out, nt);
    else
        level_tile<true>(pa, pb, H, W, x0, y0, lv.inv[k], taps, raw_a, raw_b, hp, red, out, nt);
}

// grid (4 scales, 3 channels, frames): the sums of a scale's tile partials, cs and l * cs
__global__ __launch_bounds__(kThreads) void k_ms_final(const double* __restrict__ partials, Levels lv, avx_ms_ssim_rec* __restrict__ ms) {
    __shared__ double red[2][kThreads];
    const int tid = threadIdx.x, k = blockIdx.x, c = blockIdx.y, f = blockIdx.z;
    const size_t nt = lv.t0[4], n = lv.t0[k + 1] - lv.t0[k];
    const double* pc = partials + ((size_t)(f * 3 + c) * 2) * nt + lv.t0[k];
    const double s_cs = tile_partials_sum(pc, n, red[0]), s_ss = tile_partials_sum(pc + nt, n, red[1]);
    if (tid == 0) {
        ms[f].cs[c][k + 1] = s_cs / lv.count[k];
        ms[f].ssim[c][k + 1] = s_ss / lv.count[k];
    }
}

}  // namespace

extern "C" int avx_frame_metrics_ms_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W,
                                       avx_frame_metrics* out_dev, avx_ms_ssim_rec* ms_out_dev, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a_hwc && b_hwc && out_dev && ms_out_dev, "avx_frame_metrics_ms_u8: NULL buffer (a %p, b %p, out %p, ms_out %p)",
                (const void*)a_hwc, (const void*)b_hwc, (void*)out_dev, (void*)ms_out_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "avx_frame_metrics_ms_u8: n_frames must be 1..16 (got %d)", n_frames);
    AVX_REQUIRE(ctx, H >= kMinSide && W >= kMinSide,
                "avx_frame_metrics_ms_u8: frame size %d x %d: five scales need at least %d each way (scale 4 is floor(H/16) x floor(W/16))", H, W,
                kMinSide);
    AVX_REQUIRE(ctx, (uint64_t)H * (uint64_t)W < (1ull << 32) && H <= 65535 * kT,
                "avx_frame_metrics_ms_u8: bad frame size %d x %d (H * W must be below 2^32, H at most %d)", H, W, 65535 * kT);
    AVX_REQUIRE(ctx, (((uintptr_t)out_dev | (uintptr_t)ms_out_dev) & 7) == 0, "avx_frame_metrics_ms_u8: out_dev and ms_out_dev must be 8-byte aligned");

    Levels lv{};
    ssim_window_taps(lv.taps);
    size_t pyr_elems = 0;
    for (int k = 0; k < 4; ++k) {
        lv.h[k] = H >> (k + 1), lv.w[k] = W >> (k + 1);
        lv.off[k] = pyr_elems;
        pyr_elems += (size_t)n_frames * 6 * (size_t)lv.h[k] * lv.w[k];
        lv.ntx[k] = ssim_tiles(lv.w[k]);
        lv.t0[k + 1] = lv.t0[k] + lv.ntx[k] * ssim_tiles(lv.h[k]);
        lv.inv[k] = 1.0 / (double)(1 << (2 * (k + 1)));
        lv.count[k] = (double)(lv.h[k] - (kK - 1)) * (double)(lv.w[k] - (kK - 1));
    }

    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    // the arena: scale 0's partials, the partials of scales 1..4, the pyramid
    const size_t part0 = 6 * avx_metrics_scale0_tiles(H, W) * (size_t)n_frames, part_l = (size_t)n_frames * 3 * 2 * lv.t0[4];
    int rc = avx_ensure_scratch(ctx, ws, sizeof(double) * (part0 + part_l) + sizeof(uint16_t) * pyr_elems);
    if (rc) return rc;
    double* d_part0 = (double*)ws->d_scratch;
    double* d_part_l = d_part0 + part0;
    uint16_t* d_pyr = (uint16_t*)(d_part_l + part_l);

    const dim3 pgrid((unsigned)((W + kS - 1) / kS), (unsigned)((H + kS - 1) / kS), (unsigned)n_frames);
    if (W % 4 == 0 && (((uintptr_t)a_hwc | (uintptr_t)b_hwc) & 3) == 0)  // then every row of every frame starts on a word
        hipLaunchKernelGGL(k_ms_pyramid<true>, pgrid, dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, lv, d_pyr);
    else
        hipLaunchKernelGGL(k_ms_pyramid<false>, pgrid, dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, lv, d_pyr);
    AVX_HIP(ctx, hipGetLastError());
    rc = avx_metrics_scale0_launch(ctx, a_hwc, b_hwc, n_frames, H, W, d_part0, out_dev, ms_out_dev, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ms_levels, dim3(lv.t0[4], 3, (unsigned)n_frames), dim3(kThreads), 0, s, (const uint16_t*)d_pyr, lv, d_part_l);
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ms_final, dim3(4, 3, (unsigned)n_frames), dim3(kThreads), 0, s, (const double*)d_part_l, lv, ms_out_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
