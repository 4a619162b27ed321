// csrc/receptor_edges.hip -- receptor contrast within one frame (Local Edge Intensity Analysis, van den Berg et al. 2020: the third
// stage of QCPA; the definition is include/avx.h's): per pixel the largest receptor-noise-limited contrast between the
// pixel and its up to eight neighbours at distance D, chromatic (receptor.hip's dS), achromatic (the Weber contrast of a luminance
// channel) or the larger of the two, behind the observer's acuity blur (receptor_acuity.hip's).  The quadratic form and the catch are
// receptor_common.h's; the record's share, the map's quantiser and colours and the host side's checks and launch frame are
// delta_e_common.h's; the block geometry, the reflection and the host's checks of the channel, sigma and step are
// receptor_edges_common.h's, shared with receptor_smooth.hip: one copy of each.  The blur passes are a second copy of
// receptor_acuity.hip's, statement for statement: moved to a shared header they compile k_receptor_acuity to other instructions
// (registers and schedule), and that kernel is pinned.
//
// k_receptor_edges<K, CHROMA, LUMA>: grid (blocks, frames); a workgroup of 256 threads blurs a kBlockW x kBlockH = 64 x 32 block of
// one frame and owns the block's interior, (64 - 2D) x (32 - 2D) pixels: blocks are pitched by the owned size, block (i, j) starts at
// pixel (i (64 - 2D) - D, j (32 - 2D) - D), so every neighbour of an owned pixel lies in the block.  Pixels of the block outside the
// frame blur the reflected frame and are never read as neighbours.  No scratch planes: plane by plane, for the three channels,
//   load: the (64 + 2R) x (32 + 2R) region around the block -- R the radius of this call -- is decoded (delta_e.hip's table, in LDS)
//         into the LDS tile, the reflection applied to the coordinates (blocks whose region lies inside the frame skip the folding);
//   rows: a thread forms four adjacent row sums of one region row from 16-byte LDS reads, the lanes dealt to the rows as ds_read_b128
//         groups them, into the 64 x (32 + 2R) row-pass result;
//   columns: thread (column tid & 63, segment tid >> 6) slides a window down its column for eight adjacent rows and keeps the eight
//         sums in registers.
// The taps travel as kernel arguments with three zeros in front and zeros behind; fma(0, x, s) = s and fma(t_0, x_0, +0) is the one
// rounding of t_0 x_0, so every sum is the definition's, in index order.  sigma = 0 is one tap of 1.0: fma(1, x, +0) = x.
// After three planes a thread holds the blurred (r, g, b) of its eight pixels, takes the logarithm of every catch once and writes it to
// LDS, which the blur no longer needs: plane j of the K (+ 1) log-catches is [32][64] floats, so that for each of the eight offsets a
// wave's 64 lanes -- adjacent columns of one row -- read 64 consecutive words, one per bank.  Then a thread walks its owned pixels from
// the top down: the eight neighbours' log-catches from LDS, the value, the tally, the value plane and the map.
// Nothing depends on the batch: the blocks and the order of the float64 partials are functions of H, W and D alone.
#include <cmath>

#include "delta_e_common.h"
#include "receptor_common.h"
#include "receptor_edges_common.h"

namespace {

struct EdArgs {
    const uint8_t* in;
    int R, D;
    unsigned blocks_x;
    float tp[kTapSlots];  // tp[kTapFront + k] = t_k, zero elsewhere
    LumArgs l;
    DeOut o;              // partials: [frame][block]
};

// six waves a SIMD: at most 80 registers (the kernels take 63), so that the small radii run as many workgroups as their LDS admits
template <int K, bool CHROMA, bool LUMA>
__global__ __launch_bounds__(kThreads, 6) void k_receptor_edges(EdArgs p, RnlArgs c) {
    constexpr int kPlanes = (CHROMA ? K : 0) + (LUMA ? 1 : 0);
    static_assert(kPlanes >= 1, "a channel");
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ float lut[256];
    __shared__ DeRecLds lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = p.R, D = p.D, H = p.o.H, W = p.o.W;
    const unsigned block_y = blockIdx.x / p.blocks_x, block_x = blockIdx.x - block_y * p.blocks_x;
    const int f = blockIdx.y;
    const long long x0 = (long long)block_x * (kBlockW - 2 * D) - D, y0 = (long long)block_y * (kBlockH - 2 * D) - D;  // the block's first pixel
    const size_t npx = (size_t)H * W;
    const int rows = kBlockH + 2 * R;              // rows of the region
    const int span = (kBlockW + 2 * R + 3) & ~3;   // its columns, rounded up to whole 16-byte reads: the extra ones are pixels too
    float* tile = dyn;                             // [rows][span]
    float* rowres = dyn + rows * span;             // [rows + kPadRows][kBlockW]
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    lds.hist[tid] = 0;
    rowres[rows * kBlockW + tid] = 0.0f;           // kPadRows * kBlockW == kThreads

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

    float filt[3][kPer];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint8_t* src = p.in + (size_t)f * npx * 3 + ch;
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
                *reinterpret_cast<float4*>(rowres + r * kBlockW + 4 * run) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        }
        __syncthreads();
        {
            const float* in = rowres + (seg * kPer) * kBlockW + col;
            float v[kPer + 4], acc[kPer];
#pragma unroll
            for (int o = 0; o < kPer; ++o) v[o] = in[o * kBlockW], acc[o] = 0.0f;
#pragma unroll 1
            for (int m = 0; m < groups_c; ++m) {
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[kPer + j] = in[(kPer + 4 * m + j) * kBlockW], t[j] = p.tp[kTapFront + 4 * m + j];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int o = 0; o < kPer; ++o) acc[o] = __builtin_fmaf(t[j], v[o + j], acc[o]);  // output o, tap 4 m + j
#pragma unroll
                for (int o = 0; o < kPer; ++o) v[o] = v[o + 4];
            }
#pragma unroll
            for (int o = 0; o < kPer; ++o) filt[ch][o] = acc[o];
        }
    }

    // ---- the log-catches of the thread's eight pixels, once per pixel, into the planes [plane][row][column] over the blur's LDS ----
    const Rnl<K> rnl{c};
    float* planes = dyn;
    __syncthreads();  // the last column pass has read the row-pass result
#pragma unroll
    for (int o = 0; o < kPer; ++o) {
        const float g = filt[1][o], dr = filt[0][o] - g, db = filt[2][o] - g;
        float* at = planes + (seg * kPer + o) * kBlockW + col;
        if (CHROMA) {
#pragma unroll
            for (int i = 0; i < K; ++i) at[i * kPlane] = logf(rnl_catch(c.r0[i], c.r2[i], g, dr, db) + c.eps);
        }
        if (LUMA) at[(kPlanes - 1) * kPlane] = logf(rnl_catch(p.l.r0, p.l.r2, g, dr, db) + c.eps);
    }
    __syncthreads();

    // ---- the thread's owned pixels from the top down: the value, the record, the map (a wave's pixels are adjacent bytes of each) ----
    const uint8_t* fi = p.in + (size_t)f * npx * 3;
    DeTally tally;
    float* de_out = p.o.de ? p.o.de + (size_t)f * npx : nullptr;
    uint8_t* fo = p.o.out ? p.o.out + (size_t)f * npx * 3 : nullptr;
    const long long x = x0 + col;
    const bool own_x = col >= D && col < kBlockW - D && x < (long long)W;  // x >= 0 follows: block 0 starts at -D
    for (int o = 0; o < kPer; ++o) {
        const int row = seg * kPer + o;
        const long long y = y0 + row;
        if (!own_x || row < D || row >= kBlockH - D || y >= (long long)H) continue;
        const float* at = planes + row * kBlockW + col;
        float own[kPlanes];
#pragma unroll
        for (int j = 0; j < kPlanes; ++j) own[j] = at[j * kPlane];
        float value = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const long long ny = y + dy * D, nx = x + dx * D;
                if (ny < 0 || ny >= (long long)H || nx < 0 || nx >= (long long)W) continue;  // outside the frame: skipped, not reflected
                const float* n = at + (dy * D) * kBlockW + dx * D;
                float v = 0.0f;
                if (CHROMA) {
                    float df[K];
#pragma unroll
                    for (int i = 0; i < K; ++i) df[i] = own[i] - n[i * kPlane];
                    v = rnl.from_contrasts(df);
                }
                if (LUMA) {
                    const float dl = fabsf(own[kPlanes - 1] - n[(kPlanes - 1) * kPlane]) * p.l.rcp;
                    v = CHROMA ? fmaxf(v, dl) : dl;
                }
                value = fmaxf(value, v);
            }
        }
        const size_t px = (size_t)y * W + (size_t)x;
        tally.add(value, (uint32_t)px, p.o.threshold, lds.hist);
        if (de_out) de_out[px] = value;
        if (fo) de_px_panels(p.o, fo, fi, fi, (size_t)y, (size_t)x, value);  // the map alone: the dim grey is the unfiltered frame's
    }

    // ---- the record ----
    de_record_share(tally, lds, p.o.partials + ((size_t)f * gridDim.x + blockIdx.x), p.o.rec + f);
}

template <int K>
void launch_edges(int channel, dim3 grid, size_t lds, hipStream_t s, const EdArgs& p, const RnlArgs& c) {
    if (channel == AVX_EDGES_CHROMATIC) hipLaunchKernelGGL((k_receptor_edges<K, true, false>), grid, dim3(kThreads), lds, s, p, c);
    else hipLaunchKernelGGL((k_receptor_edges<K, true, true>), grid, dim3(kThreads), lds, s, p, c);
}

}  // namespace

extern "C" int avx_receptor_edges_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                     const avx_luminance_desc* lum, int channel, double sigma, int step, int mode, float gain, float threshold,
                                     uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out, void* stream) {
    static const char fn[] = "avx_receptor_edges_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, AVX_DELTA_E_MAP, rec_dev, ds_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, hwc, hwc, n_frames, H, W, AVX_DELTA_E_MAP, map_out)) return rc;
    RnlArgs c;
    int K;
    if (const int rc = rnl_constants(ctx, fn, obs, c, K)) return rc;
    EdArgs p = {};
    int R;
    if (const int rc = edges_check(ctx, fn, lum, channel, sigma, step, p.l, p.tp, R)) return rc;
    const int D = step;
    const size_t own_w = kBlockW - 2 * D, own_h = kBlockH - 2 * D;
    const size_t blocks_x = ((size_t)W + own_w - 1) / own_w, blocks = blocks_x * (((size_t)H + own_h - 1) / own_h);  // below 2^31
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, sizeof(double) * blocks * (size_t)n_frames, rec_dev, n_frames, &s, &ws)) return rc;
    p.in = hwc, p.R = R, p.D = D, p.blocks_x = (unsigned)blocks_x;
    p.o = {map_out, ds_out, (double*)ws->d_scratch, rec_dev, H, W, mode, 0, gain, threshold};
    const int n_planes = (channel == AVX_EDGES_ACHROMATIC ? 0 : K) + (channel == AVX_EDGES_CHROMATIC ? 0 : 1);
    const size_t floats = blur_floats(R) > (size_t)n_planes * kPlane ? blur_floats(R) : (size_t)n_planes * kPlane;
    const size_t lds = sizeof(float) * floats;  // at most 41984 bytes
    const dim3 grid((unsigned)blocks, n_frames);
    if (channel == AVX_EDGES_ACHROMATIC) hipLaunchKernelGGL((k_receptor_edges<2, false, true>), grid, dim3(kThreads), lds, s, p, c);  // K plays no part
    else if (K == 2) launch_edges<2>(channel, grid, lds, s, p, c);
    else if (K == 3) launch_edges<3>(channel, grid, lds, s, p, c);
    else launch_edges<4>(channel, grid, lds, s, p, c);
    return de_finish(ctx, s, p.o.partials, blocks, W, rec_dev, n_frames);
}
