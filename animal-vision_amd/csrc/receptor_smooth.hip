// csrc/receptor_smooth.hip -- edge-preserving smoothing in receptor space in front of the edges (the project's stated
// stand-in for QCPA's RNL ranked filter, van den Berg et al. 2020; the definition is include/avx.h's, above
// avx_receptor_edges_smooth_u8).  The fused k_receptor_edges has no place for a frame-wide iteration, so this is a planes route: the
// P = K, 1 or K + 1 planes of log-catches of a group of frames lie in the workspace's scratch, twice, and three kinds of launch walk them.
//
// k_smooth_front<K, CHROMA, LUMA>: grid (blocks, frames); decode, blur and log-catches of a 64 x 32 block into the planes.  The blur
//   passes are a third copy of receptor_acuity.hip's, statement for statement from receptor_edges.hip (which says why they are copied
//   and not shared), at that kernel's D = 0 geometry: a block owns its whole tile, so every pixel is blurred once.  The sums are in
//   index order whatever the block, so a pixel's log-catches are k_receptor_edges's to the bit.
// k_receptor_smooth<K, CHROMA, LUMA>: grid (blocks, frames), one launch per iteration, from one set of planes into the other.  A
//   workgroup stages its 64 x 32 tile with a halo of R -- (64 + 2R) x (32 + 2R) x P floats, at most 62160 bytes -- in LDS, plane by
//   plane with the row pitch 64 + 2R, so a wave's 64 lanes (adjacent columns of one row) read 64 consecutive words at every offset.
//   Thread (column tid & 63, segment tid >> 6) takes its eight pixels from the top down.  A pixel walks its window three times,
//   recomputing v(p, n) from LDS each time and storing nothing: once for the count of exact zeros and the largest value; then, unless
//   the zeros already reach the rank (flat areas, and every pixel beside a straight seam: t = 0) or the rank is the window (t = the
//   largest), the bisection over the bits of t -- non-negative floats order as their bit patterns, so counting v <= candidate settles
//   one bit a round, from the largest value's top bit down, at most 31 rounds; last for the weights and the sums.  The selection is
//   exact: t is one of the values.  Templated on what changes the inner loop (K and the channel's planes), not on R.
// k_smooth_back<K, CHROMA, LUMA>: grid (blocks, frames); a block loads its 64 x 32 pixels of the planes into LDS and walks the
//   neighbours as k_receptor_edges does, at that kernel's owned-block pitch of (64 - 2D) x (32 - 2D), so the float64 partials keep
//   its order.
// Nothing depends on the batch, the group or a frame's place in either: every block works on one frame, and a group only says which
// frames share the scratch.
#include <cmath>
#include <type_traits>

#include "receptor_edges_common.h"

namespace {

constexpr int kMaxSmoothRad = 5, kMaxSmoothIter = 8;
constexpr int kMaxWindow = (2 * kMaxSmoothRad + 1) * (2 * kMaxSmoothRad + 1);  // 121
constexpr int kMaxPlanes = kMaxK + 1;
constexpr size_t kScratchCap = (size_t)1 << 30;  // the scratch of a call: the partials and the planes of a group of frames
static_assert((size_t)(kBlockW + 2 * kMaxSmoothRad) * (kBlockH + 2 * kMaxSmoothRad) * kMaxPlanes * sizeof(float) <= 65536, "the staged tile fits the LDS of a workgroup");

struct FrArgs {
    const uint8_t* in;
    float* planes;  // [frame][plane][H][W]
    int R, H, W;
    unsigned blocks_x;
    float tp[kTapSlots];  // tp[kTapFront + k] = t_k, zero elsewhere
    LumArgs l;
};

struct SmArgs {
    const float* src;  // [frame][plane][H][W]
    float* dst;
    int R, H, W;
    unsigned blocks_x;
    float lrcp;                      // 1 / e_L
    uint8_t rank[kMaxWindow + 3];    // rank[N] = ceil(KEEP N), formed by the host in float64: the contract's table
};

struct BkArgs {
    const uint8_t* in;
    const float* planes;
    int D;
    unsigned blocks_x;
    float lrcp;
    DeOut o;  // partials: [frame][block]
};

// v(p, n) exactly as k_receptor_edges takes it: own are the pixel's log-catches, n points at the neighbour's first plane, the planes
// are `stride` floats apart
template <int K, bool CHROMA, bool LUMA>
__device__ __forceinline__ float pair_value(const Rnl<K>& rnl, float lrcp, const float (&own)[(CHROMA ? K : 0) + (LUMA ? 1 : 0)], const float* n, int stride) {
    constexpr int kPlanes = (CHROMA ? K : 0) + (LUMA ? 1 : 0);
    float v = 0.0f;
    if (CHROMA) {
        float df[K];
#pragma unroll
        for (int i = 0; i < K; ++i) df[i] = own[i] - n[i * stride];
        v = rnl.from_contrasts(df);
    }
    if (LUMA) {
        const float dl = fabsf(own[kPlanes - 1] - n[(kPlanes - 1) * stride]) * lrcp;
        v = CHROMA ? fmaxf(v, dl) : dl;
    }
    return v;
}

// ---- front: decode, blur, log-catches -> planes ------------------------------------------------------------------------------------
template <int K, bool CHROMA, bool LUMA>
__global__ __launch_bounds__(kThreads, 6) void k_smooth_front(FrArgs p, RnlArgs c) {
    constexpr int kPlanes = (CHROMA ? K : 0) + (LUMA ? 1 : 0);
    static_assert(kPlanes >= 1, "a channel");
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ float lut[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = p.R, H = p.H, W = p.W;
    const unsigned block_y = blockIdx.x / p.blocks_x, block_x = blockIdx.x - block_y * p.blocks_x;
    const int f = blockIdx.y;
    const long long x0 = (long long)block_x * kBlockW, y0 = (long long)block_y * kBlockH;  // the block's first pixel
    const size_t npx = (size_t)H * W;
    const int rows = kBlockH + 2 * R;              // rows of the region
    const int span = (kBlockW + 2 * R + 3) & ~3;   // its columns, rounded up to whole 16-byte reads: the extra ones are pixels too
    float* tile = dyn;                             // [rows][span]
    float* rowres = dyn + rows * span;             // [rows + kPadRows][kBlockW]
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
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

    // ---- the log-catches of the thread's eight pixels, once per pixel, into the frame's planes (a wave's pixels are adjacent floats) ----
    const long long x = x0 + col;
    if (x >= (long long)W) return;  // no barrier follows
    float* dst = p.planes + (size_t)f * kPlanes * npx + (size_t)x;
#pragma unroll
    for (int o = 0; o < kPer; ++o) {
        const long long y = y0 + seg * kPer + o;
        if (y >= (long long)H) break;
        const float g = filt[1][o], dr = filt[0][o] - g, db = filt[2][o] - g;
        float* at = dst + (size_t)y * W;
        if (CHROMA) {
#pragma unroll
            for (int i = 0; i < K; ++i) at[i * npx] = logf(rnl_catch(c.r0[i], c.r2[i], g, dr, db) + c.eps);
        }
        if (LUMA) at[(kPlanes - 1) * npx] = logf(rnl_catch(p.l.r0, p.l.r2, g, dr, db) + c.eps);
    }
}

// ---- smooth: one iteration ---------------------------------------------------------------------------------------------------------
template <int K, bool CHROMA, bool LUMA>
__global__ __launch_bounds__(kThreads) void k_receptor_smooth(SmArgs p, RnlArgs c) {
    constexpr int kPlanes = (CHROMA ? K : 0) + (LUMA ? 1 : 0);
    static_assert(kPlanes >= 1, "a channel");
    extern __shared__ __attribute__((aligned(16))) float dyn[];  // [plane][rows][pitch]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = p.R, H = p.H, W = p.W;
    const unsigned block_y = blockIdx.x / p.blocks_x, block_x = blockIdx.x - block_y * p.blocks_x;
    const int f = blockIdx.y;
    const long long x0 = (long long)block_x * kBlockW, y0 = (long long)block_y * kBlockH;
    const size_t npx = (size_t)H * W;
    const int pitch = kBlockW + 2 * R, rows = kBlockH + 2 * R, plane = pitch * rows;
    const float* src = p.src + (size_t)f * kPlanes * npx;

    // stage: the tile and its halo; a pixel outside the frame holds 0 and is never read (the windows below stop at the frame)
    for (int r = wave; r < rows; r += kThreads / 64) {
        const long long y = y0 - R + r;
        const bool in_y = y >= 0 && y < (long long)H;
        for (int q = lane; q < pitch; q += 64) {
            const long long x = x0 - R + q;
            const bool in = in_y && x >= 0 && x < (long long)W;
            const float* at = src + (in ? (size_t)y * W + (size_t)x : 0);
#pragma unroll
            for (int j = 0; j < kPlanes; ++j) dyn[j * plane + r * pitch + q] = in ? at[j * npx] : 0.0f;
        }
    }
    __syncthreads();

    const Rnl<K> rnl{c};
    const long long x = x0 + lane;
    if (x >= (long long)W) return;  // no barrier follows
    const int dx0 = (int)(x < R ? -x : -R), dx1 = (int)(W - 1 - x < R ? W - 1 - x : R);
    float* dst = p.dst + (size_t)f * kPlanes * npx + (size_t)x;
#pragma unroll 1
    for (int o = 0; o < kPer; ++o) {
        const int row = wave * kPer + o;
        const long long y = y0 + row;
        if (y >= (long long)H) break;
        const int dy0 = (int)(y < R ? -y : -R), dy1 = (int)(H - 1 - y < R ? H - 1 - y : R);
        const unsigned N = (unsigned)((dy1 - dy0 + 1) * (dx1 - dx0 + 1)), m = p.rank[N];
        const float* at = dyn + (row + R) * pitch + lane + R;
        float own[kPlanes];
#pragma unroll
        for (int j = 0; j < kPlanes; ++j) own[j] = at[j * plane];

        // the exact zeros (the pixel's own is one) and the largest value
        unsigned zeros = 0, hi = 0;
        for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx) {
                const unsigned k = __float_as_uint(pair_value<K, CHROMA, LUMA>(rnl, p.lrcp, own, at + dy * pitch + dx, plane));
                zeros += k == 0u ? 1u : 0u;
                hi = k > hi ? k : hi;
            }
        // t: the m-th smallest value, by its bits
        unsigned tb = 0;
        if (zeros < m) {  // so hi > 0
            if (m == N) {
                tb = hi;
            } else {
                for (int b = 31 - __clz(hi); b >= 0; --b) {
                    const unsigned cand = tb | ((1u << b) - 1u);  // the largest pattern with this bit clear
                    unsigned count = 0;
                    for (int dy = dy0; dy <= dy1; ++dy)
                        for (int dx = dx0; dx <= dx1; ++dx)
                            count += __float_as_uint(pair_value<K, CHROMA, LUMA>(rnl, p.lrcp, own, at + dy * pitch + dx, plane)) <= cand ? 1u : 0u;
                    if (count < m) tb |= 1u << b;
                }
            }
        }
        // the weights and the update, the window in raster order
        const float t = __uint_as_float(tb), h = t + t;
        const float rh = h == 0.0f ? 0.0f : 1.0f / h;
        float sw = 0.0f, acc[kPlanes];
#pragma unroll
        for (int j = 0; j < kPlanes; ++j) acc[j] = 0.0f;
        for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx) {
                const float* n = at + dy * pitch + dx;
                const float v = pair_value<K, CHROMA, LUMA>(rnl, p.lrcp, own, n, plane);
                float w;
                if (h == 0.0f) {
                    w = v == 0.0f ? 1.0f : 0.0f;
                } else {
                    const float u = v * rh, a = 1.0f - u * u;
                    w = u < 1.0f ? a * a : 0.0f;
                }
                sw = sw + w;
#pragma unroll
                for (int j = 0; j < kPlanes; ++j) acc[j] = acc[j] + w * (n[j * plane] - own[j]);
            }
        float* out = dst + (size_t)y * W;
#pragma unroll
        for (int j = 0; j < kPlanes; ++j) out[j * npx] = own[j] + acc[j] / sw;
    }
}

// ---- back: the neighbour walk from the planes ---------------------------------------------------------------------------------------
template <int K, bool CHROMA, bool LUMA>
__global__ __launch_bounds__(kThreads) void k_smooth_back(BkArgs p, RnlArgs c) {
    constexpr int kPlanes = (CHROMA ? K : 0) + (LUMA ? 1 : 0);
    static_assert(kPlanes >= 1, "a channel");
    extern __shared__ __attribute__((aligned(16))) float dyn[];  // [plane][32][64]
    __shared__ DeRecLds lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = p.D, H = p.o.H, W = p.o.W;
    const unsigned block_y = blockIdx.x / p.blocks_x, block_x = blockIdx.x - block_y * p.blocks_x;
    const int f = blockIdx.y;
    const long long x0 = (long long)block_x * (kBlockW - 2 * D) - D, y0 = (long long)block_y * (kBlockH - 2 * D) - D;  // the block's first pixel
    const size_t npx = (size_t)H * W;
    const int col = lane, seg = wave;
    lds.hist[tid] = 0;
    float* planes = dyn;
    {
        const float* src = p.planes + (size_t)f * kPlanes * npx;
        const long long x = x0 + col;
        const bool in_x = x >= 0 && x < (long long)W;
#pragma unroll
        for (int o = 0; o < kPer; ++o) {
            const int row = seg * kPer + o;
            const long long y = y0 + row;
            const bool in = in_x && y >= 0 && y < (long long)H;  // a pixel outside the frame holds 0 and is never read as a neighbour
            const float* at = src + (in ? (size_t)y * W + (size_t)x : 0);
#pragma unroll
            for (int j = 0; j < kPlanes; ++j) planes[j * kPlane + row * kBlockW + col] = in ? at[j * npx] : 0.0f;
        }
    }
    __syncthreads();

    // ---- the thread's owned pixels from the top down: the value, the record, the map (a wave's pixels are adjacent bytes of each) ----
    const Rnl<K> rnl{c};
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
                value = fmaxf(value, pair_value<K, CHROMA, LUMA>(rnl, p.lrcp, own, at + (dy * D) * kBlockW + dx * D, kPlane));
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

// f(K, CHROMA, LUMA as integral constants) for the kernels of a channel: achromatic is one plane whatever K
template <class F>
void by_channel(int K, int channel, F&& f) {
    using T = std::true_type;
    using N = std::false_type;
    if (channel == AVX_EDGES_ACHROMATIC) return f(std::integral_constant<int, 2>{}, N{}, T{});
    const bool luma = channel == AVX_EDGES_EITHER;
    if (K == 2) return luma ? f(std::integral_constant<int, 2>{}, T{}, T{}) : f(std::integral_constant<int, 2>{}, T{}, N{});
    if (K == 3) return luma ? f(std::integral_constant<int, 3>{}, T{}, T{}) : f(std::integral_constant<int, 3>{}, T{}, N{});
    return luma ? f(std::integral_constant<int, 4>{}, T{}, T{}) : f(std::integral_constant<int, 4>{}, T{}, N{});
}

}  // namespace

extern "C" int avx_receptor_edges_smooth_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                            const avx_luminance_desc* lum, int channel, double sigma, int step, const avx_smooth_desc* smooth,
                                            int mode, float gain, float threshold, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out,
                                            float* planes_out, void* stream) {
    static const char fn[] = "avx_receptor_edges_smooth_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, AVX_DELTA_E_MAP, rec_dev, ds_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, hwc, hwc, n_frames, H, W, AVX_DELTA_E_MAP, map_out)) return rc;
    RnlArgs c;
    int K, R;
    if (const int rc = rnl_constants(ctx, fn, obs, c, K)) return rc;
    FrArgs fr = {};
    if (const int rc = edges_check(ctx, fn, lum, channel, sigma, step, fr.l, fr.tp, R)) return rc;
    AVX_REQUIRE(ctx, smooth && smooth->struct_size == sizeof(avx_smooth_desc), "%s: smooth is NULL or struct_size mismatch (ABI %d)", fn, AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, smooth->radius >= 1 && smooth->radius <= kMaxSmoothRad, "%s: the smoothing radius must be 1..%d (got %d)", fn, kMaxSmoothRad, smooth->radius);
    AVX_REQUIRE(ctx, std::isfinite(smooth->keep) && smooth->keep > 0.0 && smooth->keep <= 1.0, "%s: the smoothing keep must be above 0 and at most 1 (got %g)", fn,
                smooth->keep);
    AVX_REQUIRE(ctx, smooth->iterations >= 0 && smooth->iterations <= kMaxSmoothIter, "%s: the smoothing iterations must be 0..%d (got %d)", fn, kMaxSmoothIter,
                smooth->iterations);
    const size_t npx = (size_t)H * W;
    const int P = (channel == AVX_EDGES_ACHROMATIC ? 0 : K) + (channel == AVX_EDGES_CHROMATIC ? 0 : 1);
    AVX_REQUIRE(ctx, ((uintptr_t)planes_out & 3) == 0, "%s: planes_out must be 4-byte aligned", fn);
    AVX_REQUIRE(ctx, !planes_out || !overlaps(planes_out, sizeof(float) * P * npx * n_frames, hwc, npx * 3 * n_frames),
                "%s: planes_out overlaps the input (in %p, planes %p)", fn, (const void*)hwc, (const void*)planes_out);

    // ---- the geometry: the front and the smoothing tile the frame by 64 x 32, the back by the fused kernel's owned blocks ----
    const int D = step, SR = smooth->radius;
    const size_t tiles_x = ((size_t)W + kBlockW - 1) / kBlockW, tiles = tiles_x * (((size_t)H + kBlockH - 1) / kBlockH);
    const size_t own_w = kBlockW - 2 * D, own_h = kBlockH - 2 * D;
    const size_t blocks_x = ((size_t)W + own_w - 1) / own_w, blocks = blocks_x * (((size_t)H + own_h - 1) / own_h);  // below 2^31
    // ---- the scratch: the partials of every frame, then two sets of P planes for a group of frames; a group is at least one frame ----
    const size_t part_bytes = (sizeof(double) * blocks * (size_t)n_frames + 255) & ~(size_t)255, frame_bytes = sizeof(float) * P * npx;
    size_t group = part_bytes < kScratchCap ? (kScratchCap - part_bytes) / (2 * frame_bytes) : 0;
    group = group < 1 ? 1 : group > (size_t)n_frames ? (size_t)n_frames : group;
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, part_bytes + 2 * group * frame_bytes, rec_dev, n_frames, &s, &ws)) return rc;
    double* partials = (double*)ws->d_scratch;
    float* set[2] = {(float*)((char*)ws->d_scratch + part_bytes), (float*)((char*)ws->d_scratch + part_bytes) + group * P * npx};

    SmArgs sm = {};
    sm.R = SR, sm.H = H, sm.W = W, sm.blocks_x = (unsigned)tiles_x, sm.lrcp = fr.l.rcp;
    for (int n = 1; n <= kMaxWindow; ++n) sm.rank[n] = (uint8_t)ceil(smooth->keep * (double)n);  // 1 .. n
    fr.R = R, fr.H = H, fr.W = W, fr.blocks_x = (unsigned)tiles_x;
    const size_t front_lds = sizeof(float) * blur_floats(R);
    const size_t smooth_lds = sizeof(float) * (size_t)(kBlockW + 2 * SR) * (kBlockH + 2 * SR) * P, back_lds = sizeof(float) * (size_t)kPlane * P;

    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        const unsigned n = (unsigned)(group < (size_t)n_frames - f0 ? group : (size_t)n_frames - f0);
        const uint8_t* in = hwc + f0 * npx * 3;
        int cur = 0;
        fr.in = in, fr.planes = set[cur];
        by_channel(K, channel, [&](auto k, auto ch, auto lu) {
            hipLaunchKernelGGL((k_smooth_front<decltype(k)::value, decltype(ch)::value, decltype(lu)::value>), dim3((unsigned)tiles, n), dim3(kThreads), front_lds, s,
                               fr, c);
        });
        for (int it = 0; it < smooth->iterations; ++it, cur ^= 1) {
            sm.src = set[cur], sm.dst = set[cur ^ 1];
            by_channel(K, channel, [&](auto k, auto ch, auto lu) {
                hipLaunchKernelGGL((k_receptor_smooth<decltype(k)::value, decltype(ch)::value, decltype(lu)::value>), dim3((unsigned)tiles, n), dim3(kThreads),
                                   smooth_lds, s, sm, c);
            });
        }
        AVX_HIP(ctx, hipGetLastError());
        if (planes_out) AVX_HIP(ctx, hipMemcpyAsync(planes_out + f0 * P * npx, set[cur], frame_bytes * n, hipMemcpyDeviceToDevice, s));
        BkArgs bk = {};
        bk.in = in, bk.planes = set[cur], bk.D = D, bk.blocks_x = (unsigned)blocks_x, bk.lrcp = fr.l.rcp;
        bk.o = {map_out ? map_out + f0 * npx * 3 : nullptr, ds_out ? ds_out + f0 * npx : nullptr, partials + f0 * blocks, rec_dev + f0, H, W, mode, 0, gain, threshold};
        by_channel(K, channel, [&](auto k, auto ch, auto lu) {
            hipLaunchKernelGGL((k_smooth_back<decltype(k)::value, decltype(ch)::value, decltype(lu)::value>), dim3((unsigned)blocks, n), dim3(kThreads), back_lds, s,
                               bk, c);
        });
    }
    return de_finish(ctx, s, partials, blocks, W, rec_dev, n_frames);
}
