// csrc/daynight.hip -- day or night, decided per frame on the device (include/avx.h: avx_luma_mode_u8,
// avx_luma_mode_finish, avx_dichromat_auto_u8).  The rule is RatUV._choose_mode (animals/rat_uv.py:99-104): night when the median
// Rec.709 luma of the sRGB frame is below a threshold.  A median needs no selection here, because only its side of the threshold
// is asked for: count the pixels below T, and keep the largest luma below and the smallest luma not below for the one case in
// which the count alone does not decide (an even pixel count split exactly in half; avx_luma_mode_finish).
//
// k_luma_mode: a streaming kernel, grid (chunks, frames), a grid-stride loop over units of 16 pixels.  Y = (t0[R] + t1[G]) + t2[B]
// with the three 256-entry float32 tables in LDS: two float32 adds per pixel, nothing a compiler could contract, and the values
// are those NumPy forms (luma_tables below).  A frame whose first byte is 16-byte aligned reads a full unit as three 16-byte loads;
// its last, partial unit and every unit of an unaligned frame are read by bytes (a frame of a batch starts at f * 3 H W bytes, so
// the choice is per frame, uniform in a workgroup).  A thread keeps (count, max bits below, min bits not below); a workgroup
// reduces them by wave shuffles and three LDS words per wave (1024 threads, 16 waves), then thread 0 applies at most three integer atomics to the frame's
// record: add, unsigned max, unsigned min.  Y >= 0, so the order of the bit patterns is the order of the values, and all three are
// independent of arrival order: a frame's record is the same bytes in any batch and any grid.  No grid-wide synchronisation.
#include <cmath>

#include "avx_internal.h"

namespace {

constexpr int kThreads = 1024;
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr int kLumaSlot = 12;  // avx_ws::consts

// t_c[v] = float32(w_c * float32(v / 255)): NumPy's `w_c * (u8.astype(float32) / 255.0)`, whose Python scalars meet a float32 array
// as float32.  Division and multiplication are correctly rounded on both sides, so these are the same bits.
void luma_tables(float* t) {
    const float w[3] = {(float)0.2126, (float)0.7152, (float)0.0722};
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const volatile float x = (float)v / 255.0f;  // (volatile: rounded to float32 here, whatever the host's evaluation method)
            const volatile float y = w[c] * x;
            t[c * 256 + v] = y;
        }
}

struct LumaTables {
    float t[768];
    LumaTables() { luma_tables(t); }
};

struct Acc {
    uint32_t below = 0, maxb = 0, mina = kInfBits;
    __device__ __forceinline__ void see(float y, float thr) {
        const uint32_t b = __float_as_uint(y);
        if (y < thr) {
            ++below;
            maxb = b > maxb ? b : maxb;
        } else {
            mina = b < mina ? b : mina;
        }
    }
};

__global__ void k_luma_init(avx_luma_mode_rec* __restrict__ rec, int n_frames) {
    const int f = threadIdx.x;
    if (f >= n_frames) return;
    rec[f].below = 0;
    rec[f].max_below = 0.0f;
    rec[f].min_at_or_above = __uint_as_float(kInfBits);
    rec[f].pad_ = 0;
}

// thr: the smallest float32 >= the threshold, so that (Y < thr) in float32 is (Y < threshold) in double
__global__ __launch_bounds__(kThreads) void k_luma_mode(const uint8_t* __restrict__ in, uint32_t npx, float thr, const float* __restrict__ tables,
                                                        avx_luma_mode_rec* __restrict__ rec) {
    __shared__ float tab[768];
    __shared__ uint32_t wred[3][kThreads / 64];
    const int tid = threadIdx.x, f = blockIdx.y;
    for (int i = tid; i < 768; i += kThreads) tab[i] = tables[i];
    __syncthreads();
    const uint8_t* fa = in + (size_t)f * npx * 3;
    const bool aligned = ((uintptr_t)fa & 15) == 0;
    const uint32_t units = (npx + 15) / 16;
    const uint32_t step = gridDim.x * kThreads;  // (at most num_cus * 1024 units, and units <= 2^27: u + step does not wrap)
    Acc acc;
    for (uint32_t u = blockIdx.x * kThreads + tid; u < units; u += step) {
        const uint32_t p0 = u * 16;
        const uint8_t* q = fa + (size_t)p0 * 3;
        if (aligned && p0 + 16 <= npx) {
            const uint4* pv = reinterpret_cast<const uint4*>(q);
            const uint4 a0 = pv[0], a1 = pv[1], a2 = pv[2];
            const uint32_t w[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint32_t c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int byte = 3 * i + k;
                    c[k] = (w[byte >> 2] >> (8 * (byte & 3))) & 255u;
                }
                acc.see((tab[c[0]] + tab[256 + c[1]]) + tab[512 + c[2]], thr);
            }
        } else {
            const uint32_t n = npx - p0 < 16u ? npx - p0 : 16u;
            for (uint32_t i = 0; i < n; ++i) acc.see((tab[q[3 * i]] + tab[256 + q[3 * i + 1]]) + tab[512 + q[3 * i + 2]], thr);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc.below += __shfl_down(acc.below, o);
        const uint32_t m = __shfl_down(acc.maxb, o), n = __shfl_down(acc.mina, o);
        acc.maxb = m > acc.maxb ? m : acc.maxb;
        acc.mina = n < acc.mina ? n : acc.mina;
    }
    if ((tid & 63) == 0) wred[0][tid >> 6] = acc.below, wred[1][tid >> 6] = acc.maxb, wred[2][tid >> 6] = acc.mina;
    __syncthreads();
    if (tid == 0) {
        uint32_t b = wred[0][0], m = wred[1][0], n = wred[2][0];
        for (int w = 1; w < kThreads / 64; ++w) {
            b += wred[0][w];
            m = wred[1][w] > m ? wred[1][w] : m;
            n = wred[2][w] < n ? wred[2][w] : n;
        }
        avx_luma_mode_rec* r = rec + f;
        if (b) atomicAdd(&r->below, b);
        if (m) atomicMax(reinterpret_cast<uint32_t*>(&r->max_below), m);
        if (n != kInfBits) atomicMin(reinterpret_cast<uint32_t*>(&r->min_at_or_above), n);
    }
}

bool night_of(const avx_luma_mode_rec& r, uint64_t n, double T) {
    const uint64_t c2 = 2 * (uint64_t)r.below;
    if (c2 != n) return c2 > n;
    const volatile float sum = r.max_below + r.min_at_or_above;  // np.median of an even count: np.mean of the two middle float32 values
    const volatile float mid = sum / 2.0f;
    return (double)mid < T;
}

int check_luma_args(avx_ctx* ctx, const char* who, int n_frames, int H, int W, double threshold) {
    AVX_REQUIRE(ctx, n_frames >= 1 && n_frames <= 16, "%s: n_frames must be 1..16 (got %d)", who, n_frames);
    AVX_REQUIRE(ctx, H >= 1 && W >= 1 && (uint64_t)H * (uint64_t)W < (1ull << 31), "%s: bad frame size %d x %d (H * W must be below 2^31)", who, H, W);
    AVX_REQUIRE(ctx, threshold >= 0.0 && threshold <= 1.0, "%s: threshold %g outside [0, 1]", who, threshold);  // (also refuses nan)
    return AVX_OK;
}

}  // namespace

void avx_luma_tables_host(float* dst768) { luma_tables(dst768); }

extern "C" int avx_luma_mode_u8(avx_ctx* ctx, const uint8_t* in_hwc, int n_frames, int H, int W, double threshold, avx_luma_mode_rec* rec_dev,
                                void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, in_hwc && rec_dev, "avx_luma_mode_u8: NULL buffer (in %p, rec %p)", (const void*)in_hwc, (void*)rec_dev);
    if (const int rc = check_luma_args(ctx, "avx_luma_mode_u8", n_frames, H, W, threshold)) return rc;
    AVX_REQUIRE(ctx, ((uintptr_t)rec_dev & 15) == 0, "avx_luma_mode_u8: rec_dev must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    static const LumaTables kTables;  // (computed once)
    void* d_tab = nullptr;
    if (const int rc = avx_const_upload(ctx, ws, kLumaSlot, kTables.t, sizeof(kTables.t), s, &d_tab)) return rc;
    float thr = (float)threshold;
    if ((double)thr < threshold) thr = nextafterf(thr, INFINITY);
    const uint32_t npx = (uint32_t)H * (uint32_t)W;
    const size_t units = ((size_t)npx + 15) / 16;
    size_t blocks = (units + kThreads - 1) / kThreads;
    // One workgroup of 1024 threads per CU over the batch: every workgroup ends in three atomics on records that share a cache line or
    // two, and those serialise -- measured, 8 workgroups of 256 threads per CU took 64 us for a 4K batch of eight, this form 47.
    const size_t cap = ((size_t)ctx->num_cus + n_frames - 1) / n_frames;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_luma_init, dim3(1), dim3(64), 0, s, rec_dev, n_frames);
    AVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_luma_mode, dim3((unsigned)blocks, n_frames), dim3(kThreads), 0, s, in_hwc, npx, thr, (const float*)d_tab, rec_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_luma_mode_finish(avx_ctx* ctx, const avx_luma_mode_rec* rec_host, int n_frames, int H, int W, double threshold, uint8_t* modes_host) {
    AVX_REQUIRE(ctx, rec_host && modes_host, "avx_luma_mode_finish: NULL buffer");
    if (const int rc = check_luma_args(ctx, "avx_luma_mode_finish", n_frames, H, W, threshold)) return rc;
    const uint64_t n = (uint64_t)H * (uint64_t)W;
    for (int f = 0; f < n_frames; ++f) {
        AVX_REQUIRE(ctx, rec_host[f].below <= n, "avx_luma_mode_finish: record %d counts %u of %llu pixels", f, rec_host[f].below, (unsigned long long)n);
        modes_host[f] = night_of(rec_host[f], n, threshold) ? 1 : 0;
    }
    return AVX_OK;
}

extern "C" int avx_dichromat_auto_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W, const avx_dichromat_desc* d,
                                     const avx_night_desc* nd, double threshold, uint8_t* modes_host, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, d != nullptr && d->struct_size == sizeof(avx_dichromat_desc), "avx_dichromat_auto_u8: desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, nd != nullptr && nd->struct_size == sizeof(avx_night_desc), "avx_dichromat_auto_u8: night desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, in_hwc && out_hwc, "avx_dichromat_auto_u8: NULL frame pointer");
    AVX_REQUIRE(ctx, !d->in_f32, "avx_dichromat_auto_u8: in_f32 = 1: the day/night decision is defined on uint8 frames");
    if (const int rc = check_luma_args(ctx, "avx_dichromat_auto_u8", n_frames, H, W, threshold)) return rc;
    AVX_REQUIRE(ctx, H >= 13 && W >= 13, "avx_dichromat_auto_u8: frame %d x %d is smaller than 13 x 13 (the night entry's least size, whatever the frames decide)", H,
                W);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    constexpr size_t kRecBytes = sizeof(avx_luma_mode_rec) * 16;
    if (!ws->d_luma_rec) AVX_HIP(ctx, hipMalloc(&ws->d_luma_rec, kRecBytes));
    if (!ws->h_luma_rec) AVX_HIP(ctx, hipHostMalloc(&ws->h_luma_rec, kRecBytes, hipHostMallocDefault));
    avx_luma_mode_rec* rec = static_cast<avx_luma_mode_rec*>(ws->h_luma_rec);
    if (const int rc = avx_luma_mode_u8(ctx, in_hwc, n_frames, H, W, threshold, static_cast<avx_luma_mode_rec*>(ws->d_luma_rec), stream)) return rc;
    AVX_HIP(ctx, hipMemcpyAsync(rec, ws->d_luma_rec, sizeof(avx_luma_mode_rec) * (size_t)n_frames, hipMemcpyDeviceToHost, s));
    AVX_HIP(ctx, hipStreamSynchronize(s));
    uint8_t modes[16];
    if (const int rc = avx_luma_mode_finish(ctx, rec, n_frames, H, W, threshold, modes)) return rc;
    if (modes_host) memcpy(modes_host, modes, (size_t)n_frames);
    const size_t frame = (size_t)H * W * 3;
    for (int f0 = 0; f0 < n_frames;) {
        int f1 = f0 + 1;
        while (f1 < n_frames && modes[f1] == modes[f0]) ++f1;
        const int rc = modes[f0] ? avx_dichromat_night_u8(ctx, in_hwc + f0 * frame, out_hwc + f0 * frame, f1 - f0, H, W, d, nd, stream)
                                 : avx_dichromat_u8(ctx, in_hwc + f0 * frame, out_hwc + f0 * frame, f1 - f0, H, W, d, stream);
        if (rc) return rc;
        f0 = f1;
    }
    return AVX_OK;
}
