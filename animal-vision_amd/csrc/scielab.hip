// csrc/scielab.hip -- S-CIELAB colour difference maps on the device (Zhang & Wandell 1996; the definition is
// include/avx.h's): both frames are filtered in an opponent colour space by the eye's contrast sensitivity at `ppd` pixels per degree,
// and the dE00 of delta_e.hip is taken per pixel on the filtered frames.  The values, the map and the record are those of
// avx_delta_e_u8 in every other respect, and the Lab transfer function, CIEDE2000, the record, the map's quantiser and colours, a
// pixel's panels and the host side's checks and launch frame are delta_e_common.h's one copy; the 3 x 3 inverse is yuv_hdr_px.h's.
//
// Seven separable Gaussian terms (three of the luminance channel, two of each chroma channel) with R = ceil(ppd / 2) taps to either
// side, borders clamped.  The taps are formed on the host in float64, each normalised over its support, rounded once to float32 and
// kept in a constant slot of the workspace (uploaded again only when ppd changes); the kernels read them through the scalar cache.
//
// k_scielab_rows: grid (tiles, 2 * frames of the group); a workgroup owns kRowW x kRowH pixels of one side of one frame.  The codes of
// the tile and R columns to either side are decoded (delta_e.hip's table, in LDS) and taken to the opponent space on their way into
// LDS; a thread then forms the seven row sums of four adjacent pixels from a window it slides through LDS -- three loads for 28 fused
// multiply-adds -- and stores them into seven float32 planes of the workspace scratch.  The LDS image of a row is split by position
// modulo 4 so that the 64 lanes of a row read consecutive words.
// k_scielab_cols: grid (tiles, frames of the group); a workgroup owns kColW x kColH pixels of a frame pair.  Plane by plane the tile
// and R rows above and below go into LDS, a thread slides a window down its column for eight adjacent rows -- one load for eight
// multiply-adds -- and adds the term to its channel with the term's weight.  The six filtered channels of the tile then go through
// LDS to the pixel loop, where thread t takes pixels t, t + 256, ...: XYZ over white, Lab, dE00, the record, the map.
// Every pixel of either side goes through the same operations in the same order (every tap, in index order, whether or not the index
// was clamped), so equal neighbourhoods give equal Lab and a dE of exactly 0; nothing depends on the batch: the tiles and the order of
// the float64 partials are functions of H and W alone, and the batch is walked in groups, sized by H and W alone, whose planes fit
// kScratchCap.
#include <cmath>

#include "delta_e_common.h"
#include "yuv_hdr_px.h"

namespace {

constexpr int kTerms = 7, kTapStride = 8;  // taps[k][term], the eighth column is padding
constexpr int kMaxR = 64;
constexpr int kConstSlot = 11;
constexpr size_t kScratchCap = (size_t)1 << 30;

constexpr int kRowW = 256, kRowH = 4;               // a wave per row, four adjacent pixels per thread
constexpr int kRowPhase = (kRowW + 2 * kMaxR) / 4 + 8;  // words of a position class: 104, so that the four classes start 8 banks apart
constexpr int kColW = 64, kColH = 32, kColPer = 8;  // a thread: column tid & 63, rows (tid >> 6) * 8 ...
constexpr int kColRows = kColH + 2 * kMaxR;         // 160 rows of 64 floats: 40 KiB
constexpr int kColPx = kColW * kColH;
constexpr int kColLds = 6 * kColPx;                 // the six filtered channels of a tile: 48 KiB, above the plane tile's 40 KiB + a row
static_assert(kColLds >= (kColRows + 1) * kColW && kColPx == kThreads * kColPer && kRowW == 64 * 4 && kThreads == 64 * kRowH, "tile geometry");

// the channel a term belongs to: three terms of the luminance, two of each chroma channel
__host__ __device__ constexpr int term_channel(int i) { return i < 3 ? 0 : i < 5 ? 1 : 2; }

struct SlArgs {
    const uint8_t* a;    // the group's first frame
    const uint8_t* b;
    const float* taps;   // [2R + 1][kTapStride]
    float* planes;       // [frame of the group][side][term][H][W]
    int R;
    unsigned tiles_x;
    float q[3][3];       // P M: decoded sRGB -> opponent
    float pinv[3][3];    // opponent -> XYZ
    float white[3];      // 1 / the white point
    float weight[kTerms];
    DeOut o;             // the group's first frame; partials: [frame of the group][tile]
};

__global__ __launch_bounds__(kThreads) void k_scielab_rows(SlArgs p) {
    __shared__ float so[kRowH][3][4 * kRowPhase];
    __shared__ float lut[256];
    const int tid = threadIdx.x, R = p.R, H = p.o.H, W = p.o.W;
    const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int f = blockIdx.y >> 1, side = blockIdx.y & 1;
    const size_t x0 = (size_t)tile_x * kRowW, y0 = (size_t)tile_y * kRowH, npx = (size_t)H * W;
    const uint8_t* src = (side ? p.b : p.a) + (size_t)f * npx * 3;
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    __syncthreads();
    // positions 0 .. kRowW + 2R - 1 of a row are the pixels x0 - R ..., clamped into the frame; rows below the frame repeat the last
    const int span = kRowW + 2 * R;
    for (int j = tid; j < span * kRowH; j += kThreads) {
        const int r = j / span, q = j - r * span;
        const long long xs = (long long)x0 - R + q;
        const size_t x = xs < 0 ? 0 : xs > (long long)W - 1 ? (size_t)W - 1 : (size_t)xs;
        const size_t y = min(y0 + r, (size_t)H - 1);
        const uint8_t* px = src + (y * W + x) * 3;
        const float cr = lut[px[0]], cg = lut[px[1]], cb = lut[px[2]];
        const int at = (q & 3) * kRowPhase + (q >> 2);
#pragma unroll
        for (int c = 0; c < 3; ++c) so[r][c][at] = __builtin_fmaf(p.q[c][2], cb, __builtin_fmaf(p.q[c][1], cg, p.q[c][0] * cr));
    }
    __syncthreads();

    const int r = tid >> 6, t = tid & 63;
    float w[3][4], acc[kTerms][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int o = 0; o < 4; ++o) w[c][o] = so[r][c][o * kRowPhase + t];  // positions 4 t + o
#pragma unroll
    for (int i = 0; i < kTerms; ++i)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[i][o] = 0.0f;
    const float* taps = p.taps;
#pragma unroll 4
    for (int k = 0; k <= 2 * R; ++k) {
        float g[kTerms];
#pragma unroll
        for (int i = 0; i < kTerms; ++i) g[i] = taps[k * kTapStride + i];
#pragma unroll
        for (int i = 0; i < kTerms; ++i)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[i][o] = __builtin_fmaf(g[i], w[term_channel(i)][o], acc[i][o]);
        const int q = k + 4;  // the window moves on to positions 4 t + k + 1 ... + 4; the last load of the loop is not used
        const int at = (q & 3) * kRowPhase + (q >> 2) + t;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            w[c][0] = w[c][1], w[c][1] = w[c][2], w[c][2] = w[c][3];
            w[c][3] = so[r][c][at];
        }
    }
    const size_t y = y0 + r, x = x0 + 4 * (size_t)t;
    if (y >= (size_t)H || x >= (size_t)W) return;
    float* dst = p.planes + ((size_t)(f * 2 + side) * kTerms) * npx + y * W + x;
    if ((W & 3) == 0) {  // the planes start at multiples of 16 bytes then, and so does every run of four
#pragma unroll
        for (int i = 0; i < kTerms; ++i) *reinterpret_cast<float4*>(dst + i * npx) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    } else {
#pragma unroll
        for (int i = 0; i < kTerms; ++i)
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (x + o < (size_t)W) dst[i * npx + o] = acc[i][o];
    }
}

__global__ __launch_bounds__(kThreads) void k_scielab_cols(SlArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[kColLds];
    __shared__ DeRecLds lds;
    const int tid = threadIdx.x, R = p.R, H = p.o.H, W = p.o.W;
    const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
    const int f = blockIdx.y;
    const size_t x0 = (size_t)tile_x * kColW, y0 = (size_t)tile_y * kColH, npx = (size_t)H * W;
    const int col = tid & 63, seg = tid >> 6;
    const size_t xc = min(x0 + col, (size_t)W - 1);  // columns right of the frame repeat the last; they are not kept
    const float* taps = p.taps;
    lds.hist[tid] = 0;

    float filt[2][3][kColPer];
    const int rows = kColH + 2 * R;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int i = 0; i < kTerms; ++i) {
            const float* plane = p.planes + ((size_t)(f * 2 + side) * kTerms + i) * npx;
            __syncthreads();
            for (int rr = seg; rr < rows; rr += kThreads / 64) {
                const long long ys = (long long)y0 - R + rr;
                const size_t y = ys < 0 ? 0 : ys > (long long)H - 1 ? (size_t)H - 1 : (size_t)ys;
                buf[rr * kColW + col] = plane[y * W + xc];
            }
            __syncthreads();
            float w[kColPer], acc[kColPer];
#pragma unroll
            for (int o = 0; o < kColPer; ++o) w[o] = buf[(seg * kColPer + o) * kColW + col], acc[o] = 0.0f;
#pragma unroll 8
            for (int k = 0; k <= 2 * R; ++k) {
                const float g = taps[k * kTapStride + i];
#pragma unroll
                for (int o = 0; o < kColPer; ++o) acc[o] = __builtin_fmaf(g, w[o], acc[o]);
#pragma unroll
                for (int o = 0; o + 1 < kColPer; ++o) w[o] = w[o + 1];
                w[kColPer - 1] = buf[(seg * kColPer + k + kColPer) * kColW + col];  // the last load of the loop is not used: row <= kColRows
            }
            const int c = term_channel(i);
            const bool first = i == 0 || i == 3 || i == 5;
#pragma unroll
            for (int o = 0; o < kColPer; ++o) filt[side][c][o] = first ? p.weight[i] * acc[o] : __builtin_fmaf(p.weight[i], acc[o], filt[side][c][o]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int o = 0; o < kColPer; ++o) buf[(side * 3 + c) * kColPx + (seg * kColPer + o) * kColW + col] = filt[side][c][o];
    __syncthreads();

    // ---- the pixels of the tile: Lab of both sides, dE00, the record, the panels (a wave's 64 pixels are 192 adjacent bytes of each) ----
    const uint8_t* fa = p.a + (size_t)f * npx * 3;
    const uint8_t* fb = p.b + (size_t)f * npx * 3;
    DeTally tally;
    float* de_out = p.o.de ? p.o.de + (size_t)f * npx : nullptr;
    uint8_t* fo = p.o.out ? p.o.out + (size_t)f * npx * 3 * (p.o.side ? 3 : 1) : nullptr;
#pragma unroll 1
    for (int i = tid; i < kColPx; i += kThreads) {
        const size_t y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y >= (size_t)H || x >= (size_t)W) continue;
        float lab[2][3];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float o0 = buf[(side * 3) * kColPx + i], o1 = buf[(side * 3 + 1) * kColPx + i], o2 = buf[(side * 3 + 2) * kColPx + i];
            float fx[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                fx[j] = lab_f(p.white[j] * __builtin_fmaf(p.pinv[j][2], o2, __builtin_fmaf(p.pinv[j][1], o1, p.pinv[j][0] * o0)));
            lab[side][0] = 116.0f * fx[1] - 16.0f;
            lab[side][1] = 500.0f * (fx[0] - fx[1]);
            lab[side][2] = 200.0f * (fx[1] - fx[2]);
        }
        const float de = ciede2000(lab[0][0], lab[0][1], lab[0][2], lab[1][0], lab[1][1], lab[1][2]);
        const size_t at = y * W + x;
        tally.add(de, (uint32_t)at, p.o.threshold, lds.hist);
        if (de_out) de_out[at] = de;
        if (fo) de_px_panels(p.o, fo, fa, fb, y, x, de);  // the dim grey and the side panels are the unfiltered frames'
    }

    // ---- the record ----
    de_record_share(tally, lds, p.o.partials + ((size_t)f * gridDim.x + blockIdx.x), p.o.rec + f);
}

// Zhang & Wandell 1996: XYZ -> opponent (luminance, red-green, blue-yellow), and the (weight, spread in degrees) of the filter terms
constexpr double kOpp[3][3] = {{0.279, 0.72, -0.107}, {-0.449, 0.29, -0.077}, {0.086, -0.59, 0.501}};
constexpr double kTermWeight[kTerms] = {0.921, 0.105, -0.108, 0.531, 0.330, 0.488, 0.371};
constexpr double kTermSpread[kTerms] = {0.0283, 0.133, 4.336, 0.0392, 0.494, 0.0536, 0.386};

}  // namespace

extern "C" int avx_scielab_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, double ppd, int mode, float gain,
                              float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream) {
    static const char fn[] = "avx_scielab_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, layout, rec_dev, de_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, a_hwc, b_hwc, n_frames, H, W, layout, map_out)) return rc;
    AVX_REQUIRE(ctx, std::isfinite(ppd) && ppd >= 2.0 && ppd <= 128.0, "%s: ppd must be a finite number from 2 to 128 (got %g)", fn, ppd);

    // ---- the constants: float64 on the host, rounded once ----
    SlArgs p;
    const int R = (int)ceil(ppd / 2.0);  // 1 .. kMaxR
    float taps[(2 * kMaxR + 1) * kTapStride] = {};
    for (int i = 0; i < kTerms; ++i) {
        const double sd = kTermSpread[i] * ppd;
        double g[2 * kMaxR + 1], sum = 0.0;
        for (int k = 0; k <= 2 * R; ++k) sum += g[k] = exp(-(double)((k - R) * (k - R)) / (sd * sd));
        for (int k = 0; k <= 2 * R; ++k) taps[k * kTapStride + i] = (float)(g[k] / sum);
        double wsum = 0.0;
        for (int j = 0; j < kTerms; ++j) wsum += term_channel(j) == term_channel(i) ? kTermWeight[j] : 0.0;
        p.weight[i] = (float)(kTermWeight[i] / wsum);
    }
    double pinv[3][3];
    inv3(kOpp, pinv);
    const double white[3] = {kSX, kSY, kSZ};
    for (int i = 0; i < 3; ++i) {
        p.white[i] = (float)(1.0 / white[i]);
        for (int j = 0; j < 3; ++j) {
            p.q[i][j] = (float)(kOpp[i][0] * kM[0][j] + kOpp[i][1] * kM[1][j] + kOpp[i][2] * kM[2][j]);
            p.pinv[i][j] = (float)pinv[i][j];
        }
    }

    // ---- the scratch: the partials of all 16 frames a batch may hold, then the planes of one group ----
    const size_t npx = (size_t)H * W;
    const size_t row_tiles_x = (W + kRowW - 1) / kRowW, row_tiles = row_tiles_x * (((size_t)H + kRowH - 1) / kRowH);
    const size_t col_tiles_x = (W + kColW - 1) / kColW, col_tiles = col_tiles_x * (((size_t)H + kColH - 1) / kColH);  // both below 2^31
    const size_t part_bytes = (sizeof(double) * col_tiles * 16 + 255) & ~(size_t)255;
    const size_t pair_bytes = npx * 2 * kTerms * sizeof(float);
    const size_t fit = kScratchCap > part_bytes ? (kScratchCap - part_bytes) / pair_bytes : 0;
    const int group = (int)(fit < 1 ? 1 : fit > 16 ? 16 : fit);  // a pair above 19 Mpixel is walked alone and takes its 56 bytes a pixel
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, part_bytes + pair_bytes * (size_t)(group < n_frames ? group : n_frames), rec_dev, n_frames, &s, &ws)) return rc;
    void* d_taps = nullptr;
    if (const int rc = avx_const_upload(ctx, ws, kConstSlot, taps, sizeof(float) * (size_t)(2 * R + 1) * kTapStride, s, &d_taps)) return rc;
    p.taps = (const float*)d_taps;
    p.planes = (float*)((char*)ws->d_scratch + part_bytes);
    p.R = R;
    p.o.H = H, p.o.W = W, p.o.mode = mode, p.o.side = layout == AVX_DELTA_E_SIDE, p.o.gain = gain, p.o.threshold = threshold;
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int n = n_frames - f0 < group ? n_frames - f0 : group;
        p.a = a_hwc + (size_t)f0 * npx * 3, p.b = b_hwc + (size_t)f0 * npx * 3;
        p.o.out = map_out ? map_out + (size_t)f0 * npx * 3 * (p.o.side ? 3 : 1) : nullptr;
        p.o.de = de_out ? de_out + (size_t)f0 * npx : nullptr;
        p.o.partials = (double*)ws->d_scratch + (size_t)f0 * col_tiles;
        p.o.rec = rec_dev + f0;
        p.tiles_x = (unsigned)row_tiles_x;
        hipLaunchKernelGGL(k_scielab_rows, dim3((unsigned)row_tiles, 2 * n), dim3(kThreads), 0, s, p);
        AVX_HIP(ctx, hipGetLastError());
        p.tiles_x = (unsigned)col_tiles_x;
        hipLaunchKernelGGL(k_scielab_cols, dim3((unsigned)col_tiles, n), dim3(kThreads), 0, s, p);
        AVX_HIP(ctx, hipGetLastError());
    }
    return de_finish(ctx, s, (const double*)ws->d_scratch, col_tiles, W, rec_dev, n_frames);
}
