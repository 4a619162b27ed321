// csrc/diff_map.hip -- difference maps on the device: where two uint8 RGB batches differ, as one picture per frame
// (include/avx.h: AVX_DIFF_ABS, AVX_DIFF_HEAT, AVX_DIFF_SSIM; the map alone or A | B | map side by side), and per frame the record
// of the largest pixel difference, the first pixel that attains it and the number of pixels beyond the threshold.
//
// k_diff_stream (ABS, HEAT): a streaming kernel, grid (blocks, frames), a grid-stride loop over the units of a frame.  No pixel goes
// through LDS and nothing spills.  VEC (W a multiple of 16, every buffer 16-byte aligned): a thread owns 16 pixels -- three 16-byte
// loads per input, three 16-byte stores per panel; a run never leaves its row, and the panels of the side layout start at multiples
// of 48 bytes in rows of 9 W bytes, so their stores stay aligned.  Otherwise one pixel per thread and step, any size, byte accesses.
// k_diff_ssim_tile (SSIM): ssim_window.h's tile scheme as metrics.hip runs it -- the 42 x 42 patch of both frames into LDS once, row
// and column pass per channel -- with no histogram; a thread keeps the SSIM of its 4 positions for the three channels in registers
// across the channel passes, forms v of each and leaves it in LDS; the workgroup then writes the pixels its positions own (pixel
// (y, x) belongs to position (clamp(y - 5), clamp(x - 5)): tiles on the frame's border also write the replicated margin, every pixel
// is written exactly once), with the bytes of the side panels and the record's d taken from the patch in LDS.
// The record: a thread keeps the 64-bit key (d << 32) | (0xFFFFFFFF - pixel index) of its largest d, so that the larger key is the
// larger d and, among equals, the earlier pixel; a workgroup reduces keys (max) and counts (sum) by wave shuffles and four LDS words,
// then thread 0 applies one 64-bit atomicMax and one atomicAdd to the frame's record, whose first 8 bytes hold the key until
// k_diff_final turns it into (max_d, max_x, max_y).  Integer max and sum: the order of the atomics does not matter.
#include "map_common.h"
#include "ssim_window.h"

namespace {

__device__ __forceinline__ int iabs_diff(int a, int b) { return a > b ? a - b : b - a; }

// one pixel of the ABS / HEAT maps; d = max_c |a_c - b_c|
template <int MODE>
__device__ __forceinline__ int diff_px(int ar, int ag, int ab, int br, int bg, int bb, int G, int K, uint32_t& r, uint32_t& g, uint32_t& b) {
    const int dr = iabs_diff(ar, br), dg = iabs_diff(ag, bg), db = iabs_diff(ab, bb);
    const int d = max(dr, max(dg, db));
    if (MODE == AVX_DIFF_ABS) {
        r = (uint32_t)min(255, G * dr), g = (uint32_t)min(255, G * dg), b = (uint32_t)min(255, G * db);
    } else {
        pal(min(255, G * (d - K)), r, g, b);
        if (d <= K) r = g = b = dim_grey(ar, ag, ab);
    }
    return d;
}

// A thread's share of a frame's record.  see(): pixels in any order (the key decides among equal d).
struct RecAcc {
    unsigned long long key = 0;
    unsigned beyond = 0;
    __device__ __forceinline__ void see(int d, uint32_t index, int K) {
        const unsigned long long k = ((unsigned long long)(uint32_t)d << 32) | (unsigned long long)(0xFFFFFFFFu - index);
        key = k > key ? k : key;
        beyond += d > K ? 1u : 0u;
    }
    // every thread of the workgroup; wred: kThreads / 64 keys, bred: as many counts
    __device__ __forceinline__ void flush(unsigned long long* wred, unsigned* bred, avx_diff_rec* rec) {
        const int tid = threadIdx.x;
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long k = __shfl_down(key, o);
            key = k > key ? k : key;
            beyond += __shfl_down(beyond, o);
        }
        if ((tid & 63) == 0) wred[tid >> 6] = key, bred[tid >> 6] = beyond;
        __syncthreads();
        if (tid == 0) {
            unsigned long long k = wred[0];
            unsigned n = bred[0];
            for (int w = 1; w < kThreads / 64; ++w) k = wred[w] > k ? wred[w] : k, n += bred[w];
            if (k >> 32) atomicMax(reinterpret_cast<unsigned long long*>(rec), k);  // d == 0 leaves the zeroed record: (0, 0)
            if (n) atomicAdd(&rec->beyond, n);
        }
    }
};

template <int MODE, bool SIDE, bool VEC>
__global__ __launch_bounds__(kThreads) void k_diff_stream(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, int G, int K,
                                                          uint8_t* __restrict__ out, avx_diff_rec* __restrict__ rec) {
    __shared__ unsigned long long wred[kThreads / 64];
    __shared__ unsigned bred[kThreads / 64];
    const int tid = threadIdx.x, f = blockIdx.y;
    const size_t npx = (size_t)H * W;  // below 2^32
    const uint8_t* fa = a + (size_t)f * npx * 3;
    const uint8_t* fb = b + (size_t)f * npx * 3;
    uint8_t* fo = out + (size_t)f * npx * 3 * (SIDE ? 3 : 1);
    const size_t pitch = (size_t)W * 3 * (SIDE ? 3 : 1), panel = (size_t)W * 3;
    const size_t step = (size_t)gridDim.x * kThreads;
    RecAcc acc;
    if (VEC) {
        for (size_t u = (size_t)blockIdx.x * kThreads + tid; u < npx / 16; u += step) {
            const uint4* pa = reinterpret_cast<const uint4*>(fa + u * 48);
            const uint4* pb = reinterpret_cast<const uint4*>(fb + u * 48);
            const uint4 a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
            const uint32_t wa[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
            const uint32_t wb[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
            uint32_t o[12] = {};
            const uint32_t p0 = (uint32_t)(u * 16);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                int pa_[3], pb_[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int byte = 3 * i + c;
                    pa_[c] = (int)((wa[byte >> 2] >> (8 * (byte & 3))) & 255u);
                    pb_[c] = (int)((wb[byte >> 2] >> (8 * (byte & 3))) & 255u);
                }
                uint32_t q[3];
                acc.see(diff_px<MODE>(pa_[0], pa_[1], pa_[2], pb_[0], pb_[1], pb_[2], G, K, q[0], q[1], q[2]), p0 + i, K);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[(3 * i + c) >> 2] |= q[c] << (8 * ((3 * i + c) & 3));
            }
            uint8_t* dst = fo + u * 48;
            if (SIDE) {
                const uint32_t y = p0 / (uint32_t)W, x = p0 - y * (uint32_t)W;
                dst = fo + (size_t)y * pitch + (size_t)x * 3;
                uint4* da = reinterpret_cast<uint4*>(dst);
                uint4* db = reinterpret_cast<uint4*>(dst + panel);
                da[0] = a0, da[1] = a1, da[2] = a2;
                db[0] = b0, db[1] = b1, db[2] = b2;
                dst += 2 * panel;
            }
            uint4* dm = reinterpret_cast<uint4*>(dst);
            dm[0] = make_uint4(o[0], o[1], o[2], o[3]);
            dm[1] = make_uint4(o[4], o[5], o[6], o[7]);
            dm[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
    } else {
        for (size_t p = (size_t)blockIdx.x * kThreads + tid; p < npx; p += step) {
            const uint8_t* qa = fa + p * 3;
            const uint8_t* qb = fb + p * 3;
            const int ar = qa[0], ag = qa[1], ab = qa[2], br = qb[0], bg = qb[1], bb = qb[2];
            uint32_t r, g, bl;
            acc.see(diff_px<MODE>(ar, ag, ab, br, bg, bb, G, K, r, g, bl), (uint32_t)p, K);
            uint8_t* dst = fo + p * 3;
            if (SIDE) {
                const uint32_t y = (uint32_t)p / (uint32_t)W, x = (uint32_t)p - y * (uint32_t)W;
                dst = fo + (size_t)y * pitch + (size_t)x * 3;
                dst[0] = (uint8_t)ar, dst[1] = (uint8_t)ag, dst[2] = (uint8_t)ab;
                dst += panel;
                dst[0] = (uint8_t)br, dst[1] = (uint8_t)bg, dst[2] = (uint8_t)bb;
                dst += panel;
            }
            dst[0] = (uint8_t)r, dst[1] = (uint8_t)g, dst[2] = (uint8_t)bl;
        }
    }
    acc.flush(wred, bred, rec + f);
}

// ---- SSIM mode ------------------------------------------------------------------------------------------------------------------
// One channel of a tile: row pass into hp, column pass in registers, the SSIM of the thread's 4 positions into s.  Positions past the
// frame's last are computed on the patch's padding (centred zeros: a finite value) and never used.
template <int C>
__device__ __forceinline__ void map_channel(const Taps<float>& tp, const uint8_t* raw_a, const uint8_t* raw_b, float* hp, float (&s)[4]) {
    const int tid = threadIdx.x;
    row_pass([&](auto n, int row, int x) { rgb_row_item<decltype(n)::value, C>(raw_a, raw_b, hp, tp, row, x); });
    __syncthreads();
    float acc[5][4];
    column_pass(hp, tp, tid & (kT - 1), tid >> 5, acc);
#pragma unroll
    for (int o = 0; o < 4; ++o) s[o] = ssim_position_f32<false>(acc[0][o], acc[1][o], acc[2][o], acc[3][o], acc[4][o], nullptr);
    __syncthreads();  // every column pass has read hp before the next channel's row pass writes it
}

template <bool EDGE>
__device__ __forceinline__ void load_patch(const uint8_t* __restrict__ fa, const uint8_t* __restrict__ fb, int H, int W, int x0, int y0,
                                           uint8_t* raw_a, uint8_t* raw_b) {
    for (int p = threadIdx.x; p < kP * kP; p += kThreads) {
        const int py = p / kP, px = p - py * kP;
        int a0 = 128, a1 = 128, a2 = 128, b0 = 128, b1 = 128, b2 = 128;  // outside the frame: centred zero, never part of a valid window
        if (!EDGE || (y0 + py < H && x0 + px < W)) {
            const size_t off = ((size_t)(y0 + py) * W + (x0 + px)) * 3;
            a0 = fa[off], a1 = fa[off + 1], a2 = fa[off + 2];
            b0 = fb[off], b1 = fb[off + 1], b2 = fb[off + 2];
        }
        uint8_t* wa = raw_a + py * kRaw + px * 3;
        uint8_t* wb = raw_b + py * kRaw + px * 3;
        wa[0] = (uint8_t)a0, wa[1] = (uint8_t)a1, wa[2] = (uint8_t)a2;
        wb[0] = (uint8_t)b0, wb[1] = (uint8_t)b1, wb[2] = (uint8_t)b2;
    }
}

// grid (tiles along x, tiles along y, frames).  smap: NULL, or float32 [frame][H - 10][W - 10][3]
template <bool SIDE>
__global__ __launch_bounds__(kThreads) void k_diff_ssim_tile(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int H, int W, Taps<float> tp,
                                                             float scale, int K, uint8_t* __restrict__ out, avx_diff_rec* __restrict__ rec,
                                                             float* __restrict__ smap) {
    __shared__ __attribute__((aligned(16))) uint8_t raw_a[kP * kRaw];
    __shared__ __attribute__((aligned(16))) uint8_t raw_b[kP * kRaw];
    __shared__ __attribute__((aligned(16))) float hp[5 * kP * kT];
    __shared__ uint8_t vmap[kT * kT];
    __shared__ unsigned long long wred[kThreads / 64];
    __shared__ unsigned bred[kThreads / 64];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
    const size_t fo = (size_t)f * H * W * 3;
    if (x0 + kP <= W && y0 + kP <= H) load_patch<false>(a + fo, b + fo, H, W, x0, y0, raw_a, raw_b);
    else load_patch<true>(a + fo, b + fo, H, W, x0, y0, raw_a, raw_b);
    __syncthreads();

    float s[3][4];
    map_channel<0>(tp, raw_a, raw_b, hp, s[0]);
    map_channel<1>(tp, raw_a, raw_b, hp, s[1]);
    map_channel<2>(tp, raw_a, raw_b, hp, s[2]);
    const int col = tid & (kT - 1), seg = tid >> 5;
    const int PW = W - (kK - 1), PH = H - (kK - 1);  // window positions of the frame
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float sbar = ((s[0][o] + s[1][o]) + s[2][o]) / 3.0f;
        const float v = floorf(scale * (1.0f - sbar) + 0.5f);
        vmap[(seg * 4 + o) * kT + col] = (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);
        const int px = x0 + col, py = y0 + seg * 4 + o;
        if (smap && px < PW && py < PH) {
            float* dst = smap + (((size_t)f * PH + py) * PW + px) * 3;
            dst[0] = s[0][o], dst[1] = s[1][o], dst[2] = s[2][o];
        }
    }
    __syncthreads();

    // ---- the pixels this tile's positions own: position + 5, and on the frame's border the 5-pixel margin as well ----
    const int rx0 = blockIdx.x == 0 ? 0 : x0 + 5, rx1 = blockIdx.x == gridDim.x - 1 ? W : x0 + kT + 5;
    const int ry0 = blockIdx.y == 0 ? 0 : y0 + 5, ry1 = blockIdx.y == gridDim.y - 1 ? H : y0 + kT + 5;
    const int rw = rx1 - rx0, n = rw * (ry1 - ry0);  // at most kP x kP, all inside the patch
    uint8_t* fout = out + fo * (SIDE ? 3 : 1);
    const size_t pitch = (size_t)W * 3 * (SIDE ? 3 : 1), panel = (size_t)W * 3;
    RecAcc acc;
    for (int p = tid; p < n; p += kThreads) {
        const int r = ry0 + p / rw, c = rx0 + p % rw;
        const int py = min(max(r - 5, 0), PH - 1) - y0, px = min(max(c - 5, 0), PW - 1) - x0;
        uint32_t q0, q1, q2;
        pal((int)vmap[py * kT + px], q0, q1, q2);
        const uint8_t* qa = raw_a + (r - y0) * kRaw + (c - x0) * 3;
        const uint8_t* qb = raw_b + (r - y0) * kRaw + (c - x0) * 3;
        const int ar = qa[0], ag = qa[1], ab = qa[2], br = qb[0], bg = qb[1], bb = qb[2];
        acc.see(max(iabs_diff(ar, br), max(iabs_diff(ag, bg), iabs_diff(ab, bb))), (uint32_t)((size_t)r * W + c), K);
        uint8_t* dst = fout + (size_t)r * pitch + (size_t)c * 3;
        if (SIDE) {
            dst[0] = (uint8_t)ar, dst[1] = (uint8_t)ag, dst[2] = (uint8_t)ab;
            dst += panel;
            dst[0] = (uint8_t)br, dst[1] = (uint8_t)bg, dst[2] = (uint8_t)bb;
            dst += panel;
        }
        dst[0] = (uint8_t)q0, dst[1] = (uint8_t)q1, dst[2] = (uint8_t)q2;
    }
    acc.flush(wred, bred, rec + f);
}

// the key in a record's first 8 bytes -> (max_d, max_x, max_y); one thread per frame
__global__ void k_diff_final(avx_diff_rec* __restrict__ rec, int n_frames, int W) {
    const int f = threadIdx.x;
    if (f >= n_frames) return;
    const unsigned long long key = *reinterpret_cast<const unsigned long long*>(rec + f);
    const uint32_t d = (uint32_t)(key >> 32), index = 0xFFFFFFFFu - (uint32_t)key;
    rec[f].max_d = d;
    rec[f].max_x = d ? index % (uint32_t)W : 0u;
    rec[f].max_y = d ? index / (uint32_t)W : 0u;
}

template <int MODE, bool SIDE>
void launch_stream(bool vec, dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, int H, int W, int G, int K, uint8_t* out, avx_diff_rec* rec) {
    if (vec) hipLaunchKernelGGL((k_diff_stream<MODE, SIDE, true>), grid, dim3(kThreads), 0, s, a, b, H, W, G, K, out, rec);
    else hipLaunchKernelGGL((k_diff_stream<MODE, SIDE, false>), grid, dim3(kThreads), 0, s, a, b, H, W, G, K, out, rec);
}

}  // namespace

extern "C" int avx_diff_map_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, int threshold,
                               int layout, uint8_t* out_hwc, avx_diff_rec* rec_dev, float* ssim_map_dev, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a_hwc && b_hwc && out_hwc && rec_dev, "avx_diff_map_u8: NULL buffer (a %p, b %p, out %p, rec %p)", (const void*)a_hwc,
                (const void*)b_hwc, (void*)out_hwc, (void*)rec_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "avx_diff_map_u8: n_frames must be 1..16 (got %d)", n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 32), "avx_diff_map_u8: bad frame size %d x %d (H * W must be below 2^32)", H,
                W);
    AVX_REQUIRE(ctx, mode == AVX_DIFF_ABS || mode == AVX_DIFF_HEAT || mode == AVX_DIFF_SSIM, "avx_diff_map_u8: bad mode %d", mode);
    AVX_REQUIRE(ctx, layout == AVX_DIFF_MAP || layout == AVX_DIFF_SIDE, "avx_diff_map_u8: bad layout %d", layout);
    AVX_REQUIRE(ctx, threshold >= 0 && threshold <= 254, "avx_diff_map_u8: threshold must be 0..254 (got %d)", threshold);
    if (mode == AVX_DIFF_SSIM) {
        AVX_REQUIRE(ctx, gain > 0.0f && gain <= 16.0f, "avx_diff_map_u8: the gain of the SSIM mode must be above 0 and at most 16 (got %g)", (double)gain);
        AVX_REQUIRE(ctx, H >= kK && W >= kK, "avx_diff_map_u8: the SSIM mode needs frames of at least %d x %d (got %d x %d)", kK, kK, H, W);
        AVX_REQUIRE(ctx, ((uintptr_t)ssim_map_dev & 3) == 0, "avx_diff_map_u8: ssim_map_dev must be 4-byte aligned");
    } else {
        AVX_REQUIRE(ctx, gain >= 1.0f && gain <= 255.0f && gain == floorf(gain),
                    "avx_diff_map_u8: the gain of the ABS and HEAT modes must be an integer 1..255 (got %g)", (double)gain);
        AVX_REQUIRE(ctx, !ssim_map_dev, "avx_diff_map_u8: ssim_map_dev goes with the SSIM mode only (mode %d)", mode);
    }
    AVX_REQUIRE(ctx, ((uintptr_t)rec_dev & 7) == 0, "avx_diff_map_u8: rec_dev must be 8-byte aligned");
    const size_t in_bytes = (size_t)n_frames * H * W * 3, out_bytes = in_bytes * (layout == AVX_DIFF_SIDE ? 3 : 1);
    AVX_REQUIRE(ctx, !overlaps(out_hwc, out_bytes, a_hwc, in_bytes) && !overlaps(out_hwc, out_bytes, b_hwc, in_bytes),
                "avx_diff_map_u8: out_hwc overlaps an input (a %p, b %p, out %p)", (const void*)a_hwc, (const void*)b_hwc, (void*)out_hwc);
    const unsigned ntx = mode == AVX_DIFF_SSIM ? ssim_tiles(W) : 0, nty = mode == AVX_DIFF_SSIM ? ssim_tiles(H) : 0;
    AVX_REQUIRE(ctx, nty <= 65535u, "avx_diff_map_u8: %d rows are more than the SSIM kernel's grid takes (%d)", H, 65535 * kT + kK - 1);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    AVX_HIP(ctx, hipMemsetAsync(rec_dev, 0, sizeof(avx_diff_rec) * (size_t)n_frames, s));
    const bool side = layout == AVX_DIFF_SIDE;
    if (mode == AVX_DIFF_SSIM) {
        double w[kK];
        ssim_window_taps(w);
        Taps<float> tp;
        for (int k = 0; k < kK; ++k) tp.w[k] = (float)w[k];
        const float scale = 255.0f * gain;
        const dim3 grid(ntx, nty, n_frames);
        if (side) hipLaunchKernelGGL(k_diff_ssim_tile<true>, grid, dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, tp, scale, threshold, out_hwc, rec_dev, ssim_map_dev);
        else hipLaunchKernelGGL(k_diff_ssim_tile<false>, grid, dim3(kThreads), 0, s, a_hwc, b_hwc, H, W, tp, scale, threshold, out_hwc, rec_dev, ssim_map_dev);
    } else {
        const bool vec = W % 16 == 0 && (((uintptr_t)a_hwc | (uintptr_t)b_hwc | (uintptr_t)out_hwc) & 15) == 0;
        const size_t units = vec ? (size_t)H * W / 16 : (size_t)H * W;
        size_t blocks = (units + kThreads - 1) / kThreads;
        const size_t cap = ((size_t)ctx->num_cus * 8 + n_frames - 1) / n_frames;  // about 8 workgroups per CU over the batch
        if (blocks > cap) blocks = cap;
        const dim3 grid((unsigned)blocks, n_frames);
        const int G = (int)gain;
        if (mode == AVX_DIFF_ABS) {
            if (side) launch_stream<AVX_DIFF_ABS, true>(vec, grid, s, a_hwc, b_hwc, H, W, G, threshold, out_hwc, rec_dev);
            else launch_stream<AVX_DIFF_ABS, false>(vec, grid, s, a_hwc, b_hwc, H, W, G, threshold, out_hwc, rec_dev);
        } else {
            if (side) launch_stream<AVX_DIFF_HEAT, true>(vec, grid, s, a_hwc, b_hwc, H, W, G, threshold, out_hwc, rec_dev);
            else launch_stream<AVX_DIFF_HEAT, false>(vec, grid, s, a_hwc, b_hwc, H, W, G, threshold, out_hwc, rec_dev);
        }
    }
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_diff_final, dim3(1), dim3(64), 0, s, rec_dev, n_frames, W);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
