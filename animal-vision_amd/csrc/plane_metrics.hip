// csrc/plane_metrics.hip -- video compared in its own YUV planes: per frame and plane (Y, U, V) the exact histogram of
// absolute code differences of two payloads in any of the nine avx_pix_fmt layouts, at 8 or 10 bits, and the mean SSIM of the plane
// (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions, dynamic range 2^d - 1).  Nothing is converted: the samples
// are read as the decoders read them (yuv_formats.h), every plane at its own size.
//
// k_plane_tile<T, SHA, SHB>: one workgroup per (32 x 32 tile of window positions, plane, frame), on ssim_window.h's scheme: the
// 42 x 42 patch of both planes goes into LDS once as 16-bit samples, the histogram of the samples the tile owns is counted on the
// way (zeros in a register).  The moment type M is float at 8 bits (samples centred by 128, the products' rounding errors recovered
// with fma: the arithmetic of metrics.hip) and double at 10 bits: a fixed centre does not keep float32 within the bound there (flat
// 1023 against flat 1022 is 3.3e-5 off), and samples and products below 2^20 are exact in double.  k_plane_final sums the tiles of
// a (frame, plane).
// k_plane_hist<T, SHA, SHB>: the histogram alone (with_ssim == 0, or a plane with no window position): a plane is a flat run of
// samples; 16-byte loads where both sides are contiguous and aligned.
#include "ssim_window.h"
#include "yuv_formats.h"

namespace {

constexpr int kRawS = kP + 2;          // samples of a patch row in LDS (44: every row starts on an 8-byte boundary)

// where plane p of one side lies in its frame: sample i of row y is at byte off + (y * w + i) * step * sizeof(T)
struct Side { size_t frame_bytes; size_t off[3]; int step[3]; };
struct TilePlanes {
    Side a, b;
    int h[3], w[3];        // plane sizes; h == 0: absent
    unsigned ntx[3], nt[3];  // tiles per row, tiles in all; nt == 0: no window position (or no SSIM asked for)
    unsigned nt_max;       // stride of the partials of a (frame, plane)
    double taps[kK];       // the window, normalised in float64
};
// the histogram kernel's view: up to three flat runs of samples; a run of two rows is the interleaved UV plane of both sides
struct Run { size_t off_a, off_b, n; int step_a, step_b, row0, rows, vec; };
struct HistRuns { size_t frame_bytes_a, frame_bytes_b; Run r[3]; };
struct FinalPlanes { unsigned nt[3], nt_max; double count[3]; };

template <typename T, int SH>
__device__ __forceinline__ int load_sample(const uint8_t* p) {
    if constexpr (sizeof(T) == 1) return (int)*p;
    else return (int)(*reinterpret_cast<const uint16_t*>(p) >> SH);
}

// |a - b| as a bin: a planar 10-bit sample above 1023 is invalid input, its difference lands in the last bin
template <int BINS>
__device__ __forceinline__ int diff_bin(int a, int b) {
    const int d = a > b ? a - b : b - a;
    return d < BINS ? d : BINS - 1;
}

// Row item of NOUT adjacent positions of patch row `row`, from column x on (x even): the NOUT + 10 samples of both planes as the
// aligned words that hold them, centred
template <typename M, int CENTRE, int NOUT>
__device__ __forceinline__ void row_item(const uint16_t* raw_a, const uint16_t* raw_b, M* hp, const Taps<M>& tp, int row, int x) {
    constexpr int NS = NOUT + kK - 1;  // 14 or 12 samples: 7 or 6 aligned words
    const uint32_t* wa = reinterpret_cast<const uint32_t*>(raw_a + row * kRawS + x);
    const uint32_t* wb = reinterpret_cast<const uint32_t*>(raw_b + row * kRawS + x);
    M a[NS], b[NS];
#pragma unroll
    for (int i = 0; i < NS / 2; ++i) {
        const uint32_t va = wa[i], vb = wb[i];
        a[2 * i] = (M)((int)(va & 0xffffu) - CENTRE), a[2 * i + 1] = (M)((int)(va >> 16) - CENTRE);
        b[2 * i] = (M)((int)(vb & 0xffffu) - CENTRE), b[2 * i + 1] = (M)((int)(vb >> 16) - CENTRE);
    }
    row_moments<M, NOUT>(a, b, tp, hp, row, x);
}

// The SSIM of one position from its five window means (of centred samples).  float: E[x^2] - mu^2 loses nothing, the rounding error
// of the product is recovered with an fma and taken off the difference (metrics.hip); double: the direct form, its error is 2^-53 of
// mu^2 <= 2^18 against C2 >= 58.
template <typename M, int CENTRE, int PEAK>
__device__ __forceinline__ double ssim_at(M ma, M mb, M eaa, M ebb, M eab) {
    const M C1 = (M)((0.01 * PEAK) * (0.01 * PEAK)), C2 = (M)((0.03 * PEAK) * (0.03 * PEAK));
    const M paa = ma * ma, pbb = mb * mb, pab = ma * mb;
    M va = eaa - paa, vb = ebb - pbb, cab = eab - pab;
    if constexpr (sizeof(M) == 4) {
        va -= fma_m(ma, ma, -paa);
        vb -= fma_m(mb, mb, -pbb);
        cab -= fma_m(ma, mb, -pab);
    }
    const M ua = ma + (M)CENTRE, ub = mb + (M)CENTRE;
    const M num = ((M)2 * (ua * ub) + C1) * ((M)2 * cab + C2);
    const M den = ((ua * ua + ub * ub) + C1) * ((va + vb) + C2);
    return (double)(num / den);
}

template <typename T, int SHA, int SHB, bool EDGE>
__device__ __forceinline__ double tile_body(const uint8_t* __restrict__ pa, const uint8_t* __restrict__ pb, int step_a, int step_b, int H, int W,
                                            int x0, int y0, int own_w, int own_h, const Taps<typename std::conditional<sizeof(T) == 2, double, float>::type>& tp,
                                            uint16_t* raw_a, uint16_t* raw_b, void* hp_raw, unsigned* hist, double* red) {
    constexpr bool WIDE = sizeof(T) == 2;
    using M = typename std::conditional<WIDE, double, float>::type;
    constexpr int BINS = WIDE ? 1024 : 256, CENTRE = WIDE ? 512 : 128, PEAK = WIDE ? 1023 : 255;
    M* hp = reinterpret_cast<M*>(hp_raw);
    const int tid = threadIdx.x;
    // ---- patch -> LDS, histogram of the owned samples ----
    unsigned zeros = 0;
    for (int p = tid; p < kP * kP; p += kThreads) {
        const int py = p / kP, px = p - py * kP;
        int a = CENTRE, b = CENTRE;  // outside the plane: centred zero, never part of a valid window
        if (!EDGE || (y0 + py < H && x0 + px < W)) {
            const size_t i = (size_t)(y0 + py) * W + (x0 + px);
            a = load_sample<T, SHA>(pa + i * step_a * sizeof(T));
            b = load_sample<T, SHB>(pb + i * step_b * sizeof(T));
            if (px < own_w && py < own_h) {
                const int d = diff_bin<BINS>(a, b);
                if (d == 0) ++zeros;
                else atomicAdd(&hist[d], 1u);
            }
        }
        raw_a[py * kRawS + px] = (uint16_t)a;
        raw_b[py * kRawS + px] = (uint16_t)b;
    }
    zeros = wave_sum_u32(zeros);
    if ((tid & 63) == 0 && zeros) atomicAdd(&hist[0], zeros);
    __syncthreads();

    row_pass([&](auto n, int row, int x) { row_item<M, CENTRE, decltype(n)::value>(raw_a, raw_b, hp, tp, row, x); });
    __syncthreads();
    const int col = tid & (kT - 1), seg = tid >> 5;
    M acc[5][4];
    column_pass(hp, tp, col, seg, acc);
    double sum[1] = {};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (EDGE && !(x0 + col < W - (kK - 1) && y0 + seg * 4 + o < H - (kK - 1))) continue;
        sum[0] += ssim_at<M, CENTRE, PEAK>(acc[0][o], acc[1][o], acc[2][o], acc[3][o], acc[4][o]);
    }
    workgroup_sum(sum, red);
    return sum[0];
}

// grid (tiles of the largest plane, 3 planes, frames): a workgroup beyond its plane's tiles has nothing to do
template <typename T, int SHA, int SHB>
__global__ __launch_bounds__(kThreads) void k_plane_tile(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, TilePlanes tp,
                                                         double* __restrict__ partials, avx_plane_metrics_rec* __restrict__ out) {
    constexpr bool WIDE = sizeof(T) == 2;
    constexpr int BINS = WIDE ? 1024 : 256;
    using M = typename std::conditional<WIDE, double, float>::type;
    __shared__ __attribute__((aligned(16))) uint16_t raw_a[kP * kRawS];
    __shared__ __attribute__((aligned(16))) uint16_t raw_b[kP * kRawS];
    __shared__ __attribute__((aligned(16))) M hp[5 * kP * kT];
    __shared__ unsigned hist[BINS];
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x, p = blockIdx.y, f = blockIdx.z;
    const unsigned tile = blockIdx.x;
    if (tile >= tp.nt[p]) return;
    for (int i = tid; i < BINS; i += kThreads) hist[i] = 0;
    __syncthreads();
    const unsigned ntx = tp.ntx[p], ty = tile / ntx, tx = tile - ty * ntx, nty = tp.nt[p] / ntx;
    const int H = tp.h[p], W = tp.w[p];
    const int x0 = (int)tx * kT, y0 = (int)ty * kT;
    // the samples this tile counts: its kT x kT corner of the patch, and the rest of the plane for the last tile of a row / column
    const int own_w = tx == ntx - 1 ? W - x0 : kT, own_h = ty == nty - 1 ? H - y0 : kT;
    const uint8_t* pa = a + (size_t)f * tp.a.frame_bytes + tp.a.off[p];
    const uint8_t* pb = b + (size_t)f * tp.b.frame_bytes + tp.b.off[p];
    Taps<M> taps;
#pragma unroll
    for (int k = 0; k < kK; ++k) taps.w[k] = (M)tp.taps[k];
    double s;
    if (x0 + kP <= W && y0 + kP <= H)  // the whole patch lies in the plane: no bounds tests
        s = tile_body<T, SHA, SHB, false>(pa, pb, tp.a.step[p], tp.b.step[p], H, W, x0, y0, own_w, own_h, taps, raw_a, raw_b, hp, hist, red);
    else
        s = tile_body<T, SHA, SHB, true>(pa, pb, tp.a.step[p], tp.b.step[p], H, W, x0, y0, own_w, own_h, taps, raw_a, raw_b, hp, hist, red);
    if (tid == 0) partials[((size_t)f * 3 + p) * tp.nt_max + tile] = s;
    hist_flush(hist, BINS, &out[f].abs_hist[p][0]);  // the last barrier of tile_body is behind every histogram update
}

// sum of the tile partials of one (plane, frame); NaN for a plane without window positions
__global__ __launch_bounds__(kThreads) void k_plane_final(const double* __restrict__ partials, FinalPlanes fp, avx_plane_metrics_rec* __restrict__ out) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, p = blockIdx.x, f = blockIdx.y;
    const unsigned nt = fp.nt[p];
    if (nt == 0) {
        if (tid == 0) out[f].ssim[p] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double s = tile_partials_sum(partials + ((size_t)f * 3 + p) * fp.nt_max, nt, red);
    if (tid == 0) out[f].ssim[p] = s / fp.count[p];
}

// histogram alone: grid (blocks, runs, frames)
template <typename T, int SHA, int SHB>
__global__ __launch_bounds__(kThreads) void k_plane_hist(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, HistRuns hr,
                                                         avx_plane_metrics_rec* __restrict__ out) {
    constexpr int BINS = sizeof(T) == 2 ? 1024 : 256, N = 16 / (int)sizeof(T);
    __shared__ unsigned hist[2 * BINS];
    const Run r = hr.r[blockIdx.y];
    if (r.n == 0) return;
    const int tid = threadIdx.x, f = blockIdx.z;
    for (int i = tid; i < 2 * BINS; i += kThreads) hist[i] = 0;
    __syncthreads();
    const uint8_t* fa = a + (size_t)f * hr.frame_bytes_a + r.off_a;
    const uint8_t* fb = b + (size_t)f * hr.frame_bytes_b + r.off_b;
    unsigned z0 = 0, z1 = 0;  // zeros of the run's first and second row, in registers
    const size_t step = (size_t)gridDim.x * kThreads, first = (size_t)blockIdx.x * kThreads + tid;
    const int odd = r.rows - 1;  // 1: samples alternate between the two rows
    size_t done = 0;
    if (r.vec) {  // both sides contiguous and 16-byte aligned: N samples of each per step (N is even: k & 1 is the row)
        const size_t nv = r.n / N;
        for (size_t i = first; i < nv; i += step) {
            int x[N], y[N];
            load_samples<T, N, SHA>(fa + i * 16, x);
            load_samples<T, N, SHB>(fb + i * 16, y);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const int d = diff_bin<BINS>(x[k], y[k]), row = k & odd;
                if (d == 0) z0 += row == 0, z1 += row;
                else atomicAdd(&hist[row * BINS + d], 1u);
            }
        }
        done = nv * N;
    }
    for (size_t i = done + first; i < r.n; i += step) {
        const int x = load_sample<T, SHA>(fa + i * r.step_a * sizeof(T)), y = load_sample<T, SHB>(fb + i * r.step_b * sizeof(T));
        const int d = diff_bin<BINS>(x, y), row = (int)(i & 1) & odd;
        if (d == 0) z0 += row == 0, z1 += row;
        else atomicAdd(&hist[row * BINS + d], 1u);
    }
    z0 = wave_sum_u32(z0), z1 = wave_sum_u32(z1);
    if ((tid & 63) == 0) {
        if (z0) atomicAdd(&hist[0], z0);
        if (z1) atomicAdd(&hist[BINS], z1);
    }
    __syncthreads();
    for (int i = tid; i < r.rows * BINS; i += kThreads) {
        const unsigned v = hist[i];
        if (v) atomicAdd(&out[f].abs_hist[r.row0 + i / BINS][i % BINS], v);
    }
}

Side side_of(const Traits& t, int H, int W) {
    Side s{};
    const size_t ny = (size_t)H * W, nc = t.luma ? 0 : chroma_blocks(t, H, W);
    s.frame_bytes = frame_size(t, H, W);
    s.off[0] = 0, s.step[0] = 1;
    s.off[1] = ny * t.bps, s.step[1] = s.step[2] = t.il ? 2 : 1;
    s.off[2] = (t.il ? ny + 1 : ny + nc) * t.bps;
    return s;
}

template <typename T, int SHA, int SHB>
void launch_tile(dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, const TilePlanes& tp, double* partials, avx_plane_metrics_rec* out) {
    hipLaunchKernelGGL((k_plane_tile<T, SHA, SHB>), grid, dim3(kThreads), 0, s, a, b, tp, partials, out);
}
template <typename T, int SHA, int SHB>
void launch_hist(dim3 grid, hipStream_t s, const uint8_t* a, const uint8_t* b, const HistRuns& hr, avx_plane_metrics_rec* out) {
    hipLaunchKernelGGL((k_plane_hist<T, SHA, SHB>), grid, dim3(kThreads), 0, s, a, b, hr, out);
}

// the instantiation of (sample size, p010 shift of a, of b)
#define PLANE_DISPATCH(FN, wide, sha, shb, ...)                          \
    do {                                                                 \
        if (!(wide)) FN<uint8_t, 0, 0>(__VA_ARGS__);                     \
        else if (!(sha) && !(shb)) FN<uint16_t, 0, 0>(__VA_ARGS__);      \
        else if ((sha) && !(shb)) FN<uint16_t, 6, 0>(__VA_ARGS__);       \
        else if (!(sha) && (shb)) FN<uint16_t, 0, 6>(__VA_ARGS__);       \
        else FN<uint16_t, 6, 6>(__VA_ARGS__);                            \
    } while (0)

}  // namespace

extern "C" int avx_plane_metrics(avx_ctx* ctx, int fmt_a, const uint8_t* a, int fmt_b, const uint8_t* b, int n_frames, int H, int W,
                                 int with_ssim, avx_plane_metrics_rec* out_dev, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a && b && out_dev, "avx_plane_metrics: NULL buffer (a %p, b %p, out %p)", (const void*)a, (const void*)b, (void*)out_dev);
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "avx_plane_metrics: n_frames must be 1..16 (got %d)", n_frames);
    AVX_REQUIRE(ctx, fmt_ok(fmt_a) && fmt_ok(fmt_b), "avx_plane_metrics: pixel formats %d, %d (0 .. %d, enum avx_pix_fmt)", fmt_a, fmt_b,
                AVX_PIX_FMT_COUNT - 1);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && H <= (1 << 15) && W <= (1 << 15) && (uint64_t)H * (uint64_t)W < (1ull << 32),
                "avx_plane_metrics: bad frame size %d x %d (1 .. 32768 each way, a plane below 2^32 samples)", H, W);
    const Traits &ta = kTraits[fmt_a], &tb = kTraits[fmt_b];
    AVX_REQUIRE(ctx, ta.depth == tb.depth && ta.sx == tb.sx && ta.sy == tb.sy && ta.luma == tb.luma,
                "avx_plane_metrics: formats %d and %d disagree in sample depth or chroma subsampling", fmt_a, fmt_b);
    AVX_REQUIRE(ctx, ((uintptr_t)a & (ta.bps - 1)) == 0 && ((uintptr_t)b & (tb.bps - 1)) == 0,
                "avx_plane_metrics: 16-bit samples need a 2-byte aligned payload");
    AVX_REQUIRE(ctx, ((uintptr_t)out_dev & 7) == 0, "avx_plane_metrics: out_dev must be 8-byte aligned");

    const int planes = ta.luma ? 1 : 3;
    const int cw = (W + (1 << ta.sx) - 1) >> ta.sx, ch = (H + (1 << ta.sy) - 1) >> ta.sy;
    TilePlanes tp{};
    tp.a = side_of(ta, H, W), tp.b = side_of(tb, H, W);
    ssim_window_taps(tp.taps);
    FinalPlanes fp{};
    bool any_tile = false, any_hist = false;
    for (int p = 0; p < planes; ++p) {
        tp.h[p] = p ? ch : H, tp.w[p] = p ? cw : W;
        if (with_ssim != 0 && tp.h[p] >= kK && tp.w[p] >= kK) {
            tp.ntx[p] = ssim_tiles(tp.w[p]);
            tp.nt[p] = tp.ntx[p] * ssim_tiles(tp.h[p]);
            fp.count[p] = (double)(tp.h[p] - (kK - 1)) * (double)(tp.w[p] - (kK - 1));
            any_tile = true;
        } else {
            any_hist = true;
        }
        fp.nt[p] = tp.nt[p];
        if (tp.nt[p] > tp.nt_max) tp.nt_max = tp.nt[p];
    }
    fp.nt_max = tp.nt_max;

    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    double* partials = nullptr;
    if (any_tile) {
        avx_ws* ws = avx_workspace(ctx, s);
        if (!ws) return AVX_ERR_NOMEM;
        const int rc = avx_ensure_scratch(ctx, ws, sizeof(double) * 3 * (size_t)tp.nt_max * (size_t)n_frames);
        if (rc) return rc;
        partials = (double*)ws->d_scratch;
    }
    AVX_HIP(ctx, hipMemsetAsync(out_dev, 0, sizeof(avx_plane_metrics_rec) * (size_t)n_frames, s));
    const bool wide = ta.bps == 2, sha = fmt_a == AVX_PIX_P010LE, shb = fmt_b == AVX_PIX_P010LE;
    if (any_tile) {
        PLANE_DISPATCH(launch_tile, wide, sha, shb, dim3(tp.nt_max, 3, n_frames), s, a, b, tp, partials, out_dev);
        AVX_HIP(ctx, hipGetLastError());
    }
    if (any_hist) {
        // the planes the tile kernel did not take, as flat runs; the interleaved UV plane of both sides is one run of two rows
        HistRuns hr{};
        hr.frame_bytes_a = tp.a.frame_bytes, hr.frame_bytes_b = tp.b.frame_bytes;
        size_t longest = 0;
        int nr = 0;
        for (int p = 0; p < planes; ++p) {
            if (tp.nt[p]) continue;
            Run& r = hr.r[nr++];
            r.off_a = tp.a.off[p], r.off_b = tp.b.off[p], r.step_a = tp.a.step[p], r.step_b = tp.b.step[p];
            r.n = (size_t)tp.h[p] * tp.w[p], r.row0 = p, r.rows = 1;
            if (p == 1 && ta.il && tb.il && tp.nt[2] == 0) {
                r.n *= 2, r.step_a = r.step_b = 1, r.rows = 2;
                ++p;
            }
            r.vec = r.step_a == 1 && r.step_b == 1 && hr.frame_bytes_a % 16 == 0 && hr.frame_bytes_b % 16 == 0 && r.off_a % 16 == 0 &&
                    r.off_b % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
            const size_t units = r.vec ? r.n / (16 / ta.bps) + 1 : r.n;
            if (units > longest) longest = units;
        }
        size_t blocks = (longest + kThreads - 1) / kThreads;
        const size_t cap = (size_t)ctx->num_cus * 8;
        if (blocks > cap) blocks = cap;
        PLANE_DISPATCH(launch_hist, wide, sha, shb, dim3((unsigned)blocks, nr, n_frames), s, a, b, hr, out_dev);
        AVX_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_plane_final, dim3(3, n_frames), dim3(kThreads), 0, s, (const double*)partials, fp, out_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
