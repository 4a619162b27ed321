// csrc/receptor_acuity.hip -- the receptor-noise-limited colour distance behind the observer's acuity blur (AcuityView, Caves & Johnsen
// 2018, followed by the distance of Vorobyev & Osorio 1998; the definition is include/avx.h's): both frames are blurred
// in linear light by the species' own Gaussian -- cv::getGaussianKernel(cvRound(8 sigma + 1) | 1, sigma), rows then columns,
// BORDER_REFLECT_101 -- and the distance of receptor.hip is taken per pixel on the blurred values.  The value arithmetic is
// receptor_common.h's Rnl<K>; the record's share, the map's quantiser and colours, a pixel's panels and the host side's checks and
// launch frame are delta_e_common.h's: one copy of each.
//
// k_receptor_acuity<K>: grid (tiles, frames); a workgroup of 256 threads owns a kTileW x kTileH = 64 x 32 tile of one frame pair and
// needs no scratch planes: plane by plane, for the three channels of A and then of B,
//   load: the (64 + 2R) x (32 + 2R) region around the tile -- R the radius of this call, not the largest -- is decoded (delta_e.hip's
//         table, in LDS) into the LDS tile, the reflection applied to the coordinates (tiles whose region lies inside the frame skip
//         the folding); a wave takes a row, its lanes adjacent pixels;
//   rows: a thread forms four adjacent row sums of one region row from 16-byte LDS reads, four rows a wave, with the lanes dealt to the
//         rows as ds_read_b128 groups them (16 lanes of one group read 64 consecutive words), into the 64 x (32 + 2R) row-pass result;
//   columns: thread (column tid & 63, segment tid >> 6) slides a window down its column for eight adjacent rows -- lanes read
//         consecutive words, four loads for 32 multiply-adds -- and keeps the eight sums in registers.
// After six planes a thread holds the 48 blurred values of its eight pixels and goes on to the distance, the record and the map.
// The taps travel as kernel arguments with three zeros in front and zeros behind, so that both passes run whole groups of four taps:
// fma(0, x, s) = s exactly for the finite x of a tile, and fma(t_0, x_0, +0) is the one rounding of t_0 x_0, so every sum is the
// definition's, in index order.  Both sides go through the same operations in the same order: equal neighbourhoods give equal blurred
// values and a distance of exactly 0.  Nothing depends on the batch: the tiles and the order of the float64 partials are functions of H
// and W alone.
#include <cmath>

#include "delta_e_common.h"
#include "receptor_common.h"

namespace {

constexpr int kTileW = 64, kTileH = 32, kPer = 8;  // a thread: column tid & 63, rows (tid >> 6) * 8 ...
constexpr int kMaxRad = (AVX_MAX_KSIZE - 1) / 2;   // 16
constexpr int kTapFront = 3;                       // zero taps in front of t_0
constexpr int kTapSlots = 40;                      // 3 + 33 taps, and the zeros the last group of four reads
constexpr int kPadRows = 4;                        // zero rows below the row-pass result, for the last group of the column pass
static_assert(kTileW * kTileH == kThreads * kPer && kTileW == 64 && kThreads == 256, "tile geometry");
static_assert(4 * ((2 * kMaxRad + 3) / 4) + 6 < kTapSlots &&kTapFront + 4 * ((2 * kMaxRad + 4) / 4) - 1 < kTapSlots, "tap slots");

struct AcArgs {
    const uint8_t* a;
    const uint8_t* b;
    int R;
    unsigned tiles_x;
    float tp[kTapSlots];  // tp[kTapFront + k] = t_k, zero elsewhere
    DeOut o;              // partials: [frame][tile]
};

// BORDER_REFLECT_101, folded as often as needed: n = 1 gives 0
__device__ __forceinline__ long long fold101(long long i, long long n) {
    if (n == 1) return 0;
    const long long p = 2 * (n - 1);
    long long m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - m;
}

// six waves a SIMD: at most 80 registers, which the small radii need (their LDS admits seven workgroups a compute unit)
template <int K>
__global__ __launch_bounds__(kThreads, 6) void k_receptor_acuity(AcArgs p, RnlArgs c) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ float lut[256];
    __shared__ DeRecLds lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = p.R, H = p.o.H, W = p.o.W;
    const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int f = blockIdx.y;
    const long long x0 = (long long)tile_x * kTileW, y0 = (long long)tile_y * kTileH;
    const size_t npx = (size_t)H * W;
    const int rows = kTileH + 2 * R;              // rows of the region
    const int span = (kTileW + 2 * R + 3) & ~3;   // its columns, rounded up to whole 16-byte reads: the extra ones are pixels too
    float* tile = dyn;                            // [rows][span]
    float* rowres = dyn + rows * span;            // [rows + kPadRows][kTileW]
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    lds.hist[tid] = 0;
    rowres[rows * kTileW + tid] = 0.0f;           // kPadRows * kTileW == kThreads
    static_assert(kPadRows * kTileW == kThreads, "one pad word a thread");

    // a region that lies inside the frame needs no folding
    const bool edge = x0 - R < 0 || y0 - R < 0 || x0 - R + span > (long long)W || y0 - R + rows > (long long)H;
    // load: the lane's two columns of the region, as byte offsets into a frame row
    const int q1 = lane + 64;
    const bool has1 = q1 < span;
    const size_t xo0 = 3 * (size_t)(edge ? fold101(x0 - R + lane, W) : x0 - R + lane);
    const size_t xo1 = 3 * (size_t)(edge ? fold101(x0 - R + q1, W) : x0 - R + q1);
    // rows: ds_read_b128 serves the lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same of the upper half as four groups of 16;
    // a group takes one region row, its 16 lanes the row's 16 runs of four outputs
    const int l5 = lane & 31;
    const int grp = (l5 < 4 || (l5 >= 12 && l5 < 16) || (l5 >= 20 && l5 < 28)) ? 0 : 1;
    const int run = l5 < 4 ? l5 : l5 < 12 ? l5 - 4 : l5 < 20 ? l5 - 8 : l5 < 28 ? l5 - 12 : l5 - 16;
    const int rsub = (lane >> 5) * 2 + grp;
    const int groups_r = (2 * R + 3) / 4 + 1, groups_c = (2 * R + 4) / 4;  // groups of four taps of the row and of the column pass
    const int col = lane, seg = wave;

    float filt[2][3][kPer];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint8_t* src = (side ? p.b : p.a) + (size_t)f * npx * 3 + ch;
            __syncthreads();  // the table and the pad rows; the column pass of the plane before
#pragma unroll 4
            for (int r = wave; r < rows; r += kThreads / 64) {
                const long long ys = y0 - R + r;
                const uint8_t* line = src + (size_t)(edge ? fold101(ys, H) : ys) * W * 3;
                tile[r * span + lane] = lut[line[xo0]];
                if (has1) tile[r * span + q1] = lut[line[xo1]];
            }
            __syncthreads();
            for (int rb = wave * 4; rb < rows; rb += kThreads / 16) {
                const int r = rb + rsub;
                if (r < rows) {
                    const float4* in = reinterpret_cast<const float4*>(tile + r * span) + run;
                    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                    for (int m = 0; m < groups_r; ++m) {
                        const float4 v4 = in[m];
                        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                        float t[7];  // taps 4 m - 3 .. 4 m + 3
#pragma unroll
                        for (int j = 0; j < 7; ++j) t[j] = p.tp[4 * m + j];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int o = 0; o < 4; ++o) acc[o] = __builtin_fmaf(t[j - o + kTapFront], v[j], acc[o]);  // output o, tap 4 m + j - o
                    }
                    *reinterpret_cast<float4*>(rowres + r * kTileW + 4 * run) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                }
            }
            __syncthreads();
            {
                const float* in = rowres + (seg * kPer) * kTileW + col;
                float v[kPer + 4], acc[kPer];
#pragma unroll
                for (int o = 0; o < kPer; ++o) v[o] = in[o * kTileW], acc[o] = 0.0f;
#pragma unroll 1
                for (int m = 0; m < groups_c; ++m) {
                    float t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[kPer + j] = in[(kPer + 4 * m + j) * kTileW], t[j] = p.tp[kTapFront + 4 * m + j];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int o = 0; o < kPer; ++o) acc[o] = __builtin_fmaf(t[j], v[o + j], acc[o]);  // output o, tap 4 m + j
#pragma unroll
                    for (int o = 0; o < kPer; ++o) v[o] = v[o + 4];
                }
#pragma unroll
                for (int o = 0; o < kPer; ++o) filt[side][ch][o] = acc[o];
            }
        }
    }

    // ---- the thread's eight pixels: the distance, the record, the panels (a wave's 64 pixels are 192 adjacent bytes of each) ----
    const Rnl<K> rnl{c};
    const uint8_t* fa = p.a + (size_t)f * npx * 3;
    const uint8_t* fb = p.b + (size_t)f * npx * 3;
    DeTally tally;
    float* de_out = p.o.de ? p.o.de + (size_t)f * npx : nullptr;
    uint8_t* fo = p.o.out ? p.o.out + (size_t)f * npx * 3 * (p.o.side ? 3 : 1) : nullptr;
    const size_t x = (size_t)x0 + col;
#pragma unroll
    for (int o = 0; o < kPer; ++o) {
        const size_t y = (size_t)y0 + seg * kPer + o;
        if (y >= (size_t)H || x >= (size_t)W) continue;
        const float de = rnl.value(filt[0][0][o], filt[0][1][o], filt[0][2][o], filt[1][0][o], filt[1][1][o], filt[1][2][o]);
        const size_t at = y * W + x;
        tally.add(de, (uint32_t)at, p.o.threshold, lds.hist);
        if (de_out) de_out[at] = de;
        if (fo) de_px_panels(p.o, fo, fa, fb, y, x, de);  // the dim grey and the side panels are the unfiltered frames'
    }

    // ---- the record ----
    de_record_share(tally, lds, p.o.partials + ((size_t)f * gridDim.x + blockIdx.x), p.o.rec + f);
}

}  // namespace

extern "C" int avx_receptor_acuity_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                      double sigma, int mode, float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev,
                                      float* ds_out, void* stream) {
    static const char fn[] = "avx_receptor_acuity_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, layout, rec_dev, ds_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, a_hwc, b_hwc, n_frames, H, W, layout, map_out)) return rc;
    RnlArgs c;
    int K;
    if (const int rc = rnl_constants(ctx, fn, obs, c, K)) return rc;
    AVX_REQUIRE(ctx, std::isfinite(sigma) && sigma >= 0.2 && sigma <= 4.0, "%s: sigma must be a finite number from 0.2 to 4 (got %g)", fn, sigma);
    const int ksize = (int)lrint(sigma * 8.0 + 1.0) | 1;  // cvRound: half to even
    AVX_REQUIRE(ctx, ksize >= 3 && ksize <= AVX_MAX_KSIZE, "%s: sigma %g needs %d taps, 3 .. %d are supported", fn, sigma, ksize, AVX_MAX_KSIZE);

    // ---- the taps: cv::getGaussianKernel(ksize, sigma) in double, summed left to right, rounded once ----
    AcArgs p = {};
    {
        const double scale2x = -0.5 / (sigma * sigma), mid = (ksize - 1) * 0.5;
        double t[AVX_MAX_KSIZE], sum = 0.0;
        for (int i = 0; i < ksize; ++i) sum += t[i] = exp(scale2x * (i - mid) * (i - mid));
        const double scale = 1.0 / sum;
        for (int i = 0; i < ksize; ++i) p.tp[kTapFront + i] = (float)(t[i] * scale);
    }
    const int R = (ksize - 1) / 2;
    const size_t tiles_x = ((size_t)W + kTileW - 1) / kTileW, tiles = tiles_x * (((size_t)H + kTileH - 1) / kTileH);  // below 2^31
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, sizeof(double) * tiles * (size_t)n_frames, rec_dev, n_frames, &s, &ws)) return rc;
    p.a = a_hwc, p.b = b_hwc, p.R = R, p.tiles_x = (unsigned)tiles_x;
    p.o = {map_out, ds_out, (double*)ws->d_scratch, rec_dev, H, W, mode, layout == AVX_DELTA_E_SIDE, gain, threshold};
    const int rows = kTileH + 2 * R, span = (kTileW + 2 * R + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)rows * span + (size_t)(rows + kPadRows) * kTileW);  // at most 41984 bytes
    const dim3 grid((unsigned)tiles, n_frames);
    if (K == 2) hipLaunchKernelGGL((k_receptor_acuity<2>), grid, dim3(kThreads), lds, s, p, c);
    else if (K == 3) hipLaunchKernelGGL((k_receptor_acuity<3>), grid, dim3(kThreads), lds, s, p, c);
    else hipLaunchKernelGGL((k_receptor_acuity<4>), grid, dim3(kThreads), lds, s, p, c);
    return de_finish(ctx, s, p.o.partials, tiles, W, rec_dev, n_frames);
}
