// csrc/metrics.hip -- frame comparison on the device: per frame and channel the exact histogram of absolute code
// differences of two uint8 RGB batches, and the mean SSIM (ssim_window.h: the tile scheme, its passes and its sums).
//
// k_metrics_tile: one workgroup per (32 x 32 tile of window positions, frame).  The 42 x 42 patch of both frames goes into LDS once,
// as bytes and for the three channels together (a patch row is 126 contiguous bytes of the interleaved frame); the histogram of the
// samples the tile owns is counted on the way.  The passes then run per channel, in float32: the samples are centred by 128 before
// they are squared, so the moments keep their digits where variance and covariance need them, and the SSIM of a position is formed
// in float32 with the products' rounding errors recovered with fma.  k_metrics_final sums the tiles of a (frame, channel).
// k_metrics_hist is the histogram alone (with_ssim == 0, or a frame with no window position).
// WITH_CS (avx_metrics_scale0_launch with a record of ms_ssim.hip) is the same tile code that also sums the contrast-
// structure term cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2) of every position: scale 0 of MS-SSIM.  The SSIM sums are formed by the
// same operations in the same order in both instantiations (nothing is contracted: -ffp-contract=off), so they are bit-identical.
#include "ssim_window.h"

namespace {

constexpr int kBins = 3 * 256;

// one sample pair into the workgroup's histogram; zeros, by far the commonest difference of two renderings of one clip, are
// counted in a register
__device__ __forceinline__ void hist_add(unsigned* hist, int c, int a, int b, unsigned& zeros) {
    const int d = a > b ? a - b : b - a;
    if (d == 0) ++zeros;
    else atomicAdd(&hist[c * 256 + d], 1u);
}

// One channel of a tile: row pass into hp, column pass in registers, the SSIM of the thread's 4 positions, the workgroup's sum.
template <bool EDGE, int C, bool WITH_CS>
__device__ __forceinline__ void channel_pass(int H, int W, int x0, int y0, const Taps<float>& tp, const uint8_t* raw_a, const uint8_t* raw_b, float* hp,
                                             double* red, double* part, size_t cs_offset) {
    const int tid = threadIdx.x;
    row_pass([&](auto n, int row, int x) { rgb_row_item<decltype(n)::value, C>(raw_a, raw_b, hp, tp, row, x); });
    __syncthreads();
    const int col = tid & (kT - 1), seg = tid >> 5;
    float acc[5][4];
    column_pass(hp, tp, col, seg, acc);
    // ---- SSIM of the thread's positions: ssim_window.h's float32 arithmetic of one position ----
    double sum[WITH_CS ? 2 : 1] = {};  // SSIM and, WITH_CS, cs
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (EDGE && !(x0 + col < W - (kK - 1) && y0 + seg * 4 + o < H - (kK - 1))) continue;
        float cs = 0.0f;
        sum[0] += (double)ssim_position_f32<WITH_CS>(acc[0][o], acc[1][o], acc[2][o], acc[3][o], acc[4][o], &cs);
        if constexpr (WITH_CS) sum[1] += (double)cs;
    }
    workgroup_sum(sum, red);  // its barrier: every column pass has read hp before the next channel's row pass writes it
    if (tid == 0) {
        *part = sum[0];
        if constexpr (WITH_CS) part[cs_offset] = sum[1];
    }
}

template <bool EDGE, bool WITH_CS>
__device__ __forceinline__ void tile_body(const uint8_t* __restrict__ fa, const uint8_t* __restrict__ fb, int H, int W, int x0, int y0,
                                          int own_w, int own_h, const Taps<float>& tp, uint8_t* raw_a, uint8_t* raw_b, float* hp, unsigned* hist,
                                          double* red, double* part, size_t part_stride) {
    const int tid = threadIdx.x;
    // ---- patch -> LDS (bytes, three channels), histogram of the owned samples ----
    unsigned z0 = 0, z1 = 0, z2 = 0;
    for (int p = tid; p < kP * kP; p += kThreads) {
        const int py = p / kP, px = p - py * kP;
        int a0 = 128, a1 = 128, a2 = 128, b0 = 128, b1 = 128, b2 = 128;  // outside the frame: centred zero, never part of a valid window
        if (!EDGE || (y0 + py < H && x0 + px < W)) {
            const size_t off = ((size_t)(y0 + py) * W + (x0 + px)) * 3;
            a0 = fa[off], a1 = fa[off + 1], a2 = fa[off + 2];
            b0 = fb[off], b1 = fb[off + 1], b2 = fb[off + 2];
            if (px < own_w && py < own_h) {
                hist_add(hist, 0, a0, b0, z0);
                hist_add(hist, 1, a1, b1, z1);
                hist_add(hist, 2, a2, b2, z2);
            }
        }
        uint8_t* wa = raw_a + py * kRaw + px * 3;
        uint8_t* wb = raw_b + py * kRaw + px * 3;
        wa[0] = (uint8_t)a0, wa[1] = (uint8_t)a1, wa[2] = (uint8_t)a2;
        wb[0] = (uint8_t)b0, wb[1] = (uint8_t)b1, wb[2] = (uint8_t)b2;
    }
    z0 = wave_sum_u32(z0), z1 = wave_sum_u32(z1), z2 = wave_sum_u32(z2);
    if ((tid & 63) == 0) {
        if (z0) atomicAdd(&hist[0], z0);
        if (z1) atomicAdd(&hist[256], z1);
        if (z2) atomicAdd(&hist[512], z2);
    }
    __syncthreads();

    // WITH_CS: the cs sum of channel c lies three rows of partials behind its SSIM sum
    channel_pass<EDGE, 0, WITH_CS>(H, W, x0, y0, tp, raw_a, raw_b, hp, red, part, 3 * part_stride);
    channel_pass<EDGE, 1, WITH_CS>(H, W, x0, y0, tp, raw_a, raw_b, hp, red, part + part_stride, 3 * part_stride);
    channel_pass<EDGE, 2, WITH_CS>(H, W, x0, y0, tp, raw_a, raw_b, hp, red, part + 2 * part_stride, 3 * part_stride);
}

// partials: [frame][row][tile] doubles, rows 0..2 the SSIM sums of the channels and, WITH_CS, rows 3..5 their cs sums
template <bool WITH_CS>
__global__ __launch_bounds__(kThreads) void k_metrics_tile(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, Taps<float> tp,
                                                           double* __restrict__ partials, avx_frame_metrics* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t raw_a[kP * kRaw];
    __shared__ __attribute__((aligned(16))) uint8_t raw_b[kP * kRaw];
    __shared__ __attribute__((aligned(16))) float hp[5 * kP * kT];
    __shared__ unsigned hist[kBins];
    __shared__ double red[(WITH_CS ? 2 : 1) * (kThreads / 64)];
    const int tid = threadIdx.x, f = blockIdx.z;
    for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
    __syncthreads();
    const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
    // the samples this tile counts: its kT x kT corner of the patch, and the rest of the frame for the last tile of a row / column
    const int own_w = blockIdx.x == gridDim.x - 1 ? W - x0 : kT, own_h = blockIdx.y == gridDim.y - 1 ? H - y0 : kT;
    const size_t fo = (size_t)f * H * W * 3;
    const size_t ntiles = (size_t)gridDim.x * gridDim.y;
    double* part = partials + (size_t)f * (WITH_CS ? 6 : 3) * ntiles + ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    if (x0 + kP <= W && y0 + kP <= H)  // the whole patch lies in the frame: no bounds tests
        tile_body<false, WITH_CS>(a + fo, b + fo, H, W, x0, y0, own_w, own_h, tp, raw_a, raw_b, hp, hist, red, part, ntiles);
    else
        tile_body<true, WITH_CS>(a + fo, b + fo, H, W, x0, y0, own_w, own_h, tp, raw_a, raw_b, hp, hist, red, part, ntiles);
    hist_flush(hist, kBins, &out[f].abs_hist[0][0]);  // the last barrier of tile_body is behind every histogram update
}

// sum of the tile partials of one (row of partials, frame).
// grid (3, frames): the SSIM of the channels; grid (6, frames) with ms: rows 3..5 are the cs sums, and scale 0 of ms[f] is filled.
__global__ __launch_bounds__(kThreads) void k_metrics_final(const double* __restrict__ partials, size_t ntiles, double count,
                                                            avx_frame_metrics* __restrict__ out, avx_ms_ssim_rec* __restrict__ ms) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, f = blockIdx.y;
    const int c = blockIdx.x % 3;
    const double s = tile_partials_sum(partials + ((size_t)f * gridDim.x + blockIdx.x) * ntiles, ntiles, red);
    if (tid == 0) {
        const double v = s / count;
        if (blockIdx.x < 3) {
            out[f].ssim[c] = v;
            if (ms) ms[f].ssim[c][0] = v;
        } else {
            ms[f].cs[c][0] = v;
        }
    }
}

// histogram alone: grid (blocks, frames); VEC: 16 bytes of both frames per thread and step
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_metrics_hist(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t frame_bytes,
                                                           avx_frame_metrics* __restrict__ out) {
    __shared__ unsigned hist[kBins];
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
    __syncthreads();
    const uint8_t* fa = a + (size_t)f * frame_bytes;
    const uint8_t* fb = b + (size_t)f * frame_bytes;
    unsigned z0 = 0, z1 = 0, z2 = 0;  // zeros per channel, in registers
    const size_t step = (size_t)gridDim.x * kThreads;
    if (VEC) {
        const size_t n = frame_bytes / 16;
        for (size_t i = (size_t)blockIdx.x * kThreads + tid; i < n; i += step) {
            const uint4 va = reinterpret_cast<const uint4*>(fa)[i], vb = reinterpret_cast<const uint4*>(fb)[i];
            const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
            const int c0 = (int)((i * 16) % 3);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int c = (c0 + k) % 3;
                const int x = (wa[k >> 2] >> (8 * (k & 3))) & 255, y = (wb[k >> 2] >> (8 * (k & 3))) & 255;
                const int d = x > y ? x - y : y - x;
                if (d == 0) z0 += c == 0, z1 += c == 1, z2 += c == 2;
                else atomicAdd(&hist[c * 256 + d], 1u);
            }
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * kThreads + tid; i < frame_bytes; i += step) {
            const int c = (int)(i % 3), x = fa[i], y = fb[i];
            const int d = x > y ? x - y : y - x;
            if (d == 0) z0 += c == 0, z1 += c == 1, z2 += c == 2;
            else atomicAdd(&hist[c * 256 + d], 1u);
        }
    }
    z0 = wave_sum_u32(z0), z1 = wave_sum_u32(z1), z2 = wave_sum_u32(z2);
    if ((tid & 63) == 0) {
        if (z0) atomicAdd(&hist[0], z0);
        if (z1) atomicAdd(&hist[256], z1);
        if (z2) atomicAdd(&hist[512], z2);
    }
    __syncthreads();
    hist_flush(hist, kBins, &out[f].abs_hist[0][0]);
    if (blockIdx.x == 0 && tid < 3) out[f].ssim[tid] = __longlong_as_double(0x7ff8000000000000LL);
}

}  // namespace

// avx_internal.h: the record memset, k_metrics_tile and k_metrics_final of n_frames frames with window positions, arguments checked
// by the caller; partials: (ms ? 6 : 3) * tiles * n_frames doubles
int avx_metrics_scale0_launch(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, double* partials,
                              avx_frame_metrics* out_dev, avx_ms_ssim_rec* ms, hipStream_t s) {
    const unsigned ntx = ssim_tiles(W), nty = ssim_tiles(H);
    const size_t ntiles = (size_t)ntx * nty;
    AVX_HIP(ctx, hipMemsetAsync(out_dev, 0, sizeof(avx_frame_metrics) * (size_t)n_frames, s));
    double w[kK];
    ssim_window_taps(w);
    Taps<float> tp;
    for (int k = 0; k < kK; ++k) tp.w[k] = (float)w[k];
    if (ms)
        hipLaunchKernelGGL(k_metrics_tile<true>, dim3(ntx, nty, n_frames), dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, tp, partials, out_dev);
    else
        hipLaunchKernelGGL(k_metrics_tile<false>, dim3(ntx, nty, n_frames), dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, tp, partials, out_dev);
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_metrics_final, dim3(ms ? 6 : 3, n_frames), dim3(kThreads), 0, s, (const double*)partials, ntiles,
                       (double)(H - (kK - 1)) * (double)(W - (kK - 1)), out_dev, ms);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

// tiles of a frame with window positions: what a row of partials holds
size_t avx_metrics_scale0_tiles(int H, int W) {
    return (size_t)ssim_tiles(W) * ssim_tiles(H);
}

extern "C" int avx_frame_metrics_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int with_ssim,
                                    avx_frame_metrics* out_dev, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a_hwc && b_hwc && out_dev, "avx_frame_metrics_u8: NULL buffer (a %p, b %p, out %p)", (const void*)a_hwc, (const void*)b_hwc,
                (void*)out_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "avx_frame_metrics_u8: n_frames must be 1..16 (got %d)", n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 32), "avx_frame_metrics_u8: bad frame size %d x %d (H * W must be below 2^32)",
                H, W);
    AVX_REQUIRE(ctx, ((uintptr_t)out_dev & 7) == 0, "avx_frame_metrics_u8: out_dev must be 8-byte aligned");
    const bool ssim = with_ssim != 0 && H >= kK && W >= kK;
    const unsigned ntx = ssim ? ssim_tiles(W) : 0, nty = ssim ? ssim_tiles(H) : 0;
    AVX_REQUIRE(ctx, nty <= 65535u, "avx_frame_metrics_u8: %d rows are more than the SSIM kernel's grid takes (%d)", H, 65535 * kT + kK - 1);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (ssim) {
        avx_ws* ws = avx_workspace(ctx, s);
        if (!ws) return AVX_ERR_NOMEM;
        const int rc = avx_ensure_scratch(ctx, ws, sizeof(double) * 3 * (size_t)ntx * nty * (size_t)n_frames);
        if (rc) return rc;
        return avx_metrics_scale0_launch(ctx, a_hwc, b_hwc, n_frames, H, W, (double*)ws->d_scratch, out_dev, nullptr, s);
    }
    AVX_HIP(ctx, hipMemsetAsync(out_dev, 0, sizeof(avx_frame_metrics) * (size_t)n_frames, s));
    const size_t fbytes = (size_t)H * W * 3;
    const bool vec = fbytes % 16 == 0 && (((uintptr_t)a_hwc | (uintptr_t)b_hwc) & 15) == 0;
    const size_t units = vec ? fbytes / 16 : fbytes;
    size_t blocks = (units + kThreads - 1) / kThreads;
    const size_t cap = (size_t)ctx->num_cus * 8;
    if (blocks > cap) blocks = cap;
    if (vec)
        hipLaunchKernelGGL(k_metrics_hist<true>, dim3((unsigned)blocks, n_frames), dim3(kThreads), 0, s, a_hwc, b_hwc, fbytes, out_dev);
    else
        hipLaunchKernelGGL(k_metrics_hist<false>, dim3((unsigned)blocks, n_frames), dim3(kThreads), 0, s, a_hwc, b_hwc, fbytes, out_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
