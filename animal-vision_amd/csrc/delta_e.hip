// csrc/delta_e.hip -- CIEDE2000 colour difference maps on the device (the definition is include/avx.h's): per pixel of
// two uint8 sRGB batches the colour difference dE00 in CIELAB (D65), as a float32 plane, as a picture (AVX_DELTA_E_HEAT, _PLAIN; the
// map alone or A | B | map side by side) and as a record per frame: the histogram of dE in bins of 0.5, the float64 sum, the largest
// dE with the first pixel that attains it, and the number of pixels beyond the threshold.
//
// k_delta_e: grid (chunks, frames); a workgroup owns kChunk = 4096 consecutive pixels of a frame -- a function of H and W alone, so
// that the float64 sum of a frame is formed in one order whatever the batch.  The walk of a chunk -- both frames into LDS, thread t
// on pixels t, t + 256, ..., the map's bytes back through LDS, the panels out in 16-byte stores or bytes -- is delta_e_walk.h's,
// shared with receptor.hip; the value of a pixel is this file's: Lab of both (a 256-entry decode table in LDS, the anchored matrix
// form, cbrtf) and dE00 in radians throughout (the four cosines of T from one sincosf by the multiple-angle formulas).  A pixel whose
// codes are equal is 0 by definition and skips the arithmetic; the branch is taken by a wave whose 64 pixels are all equal.  The
// arithmetic is the vector unit's: nothing here is bound by bytes.
// The map's quantiser is delta_e_common.h's de_map_colour, float32 with one rounding per operation and nothing fused (its __fsub_rn(),
// __fmul_rn() and __fadd_rn() name them): v = min(floor(G x + 0.5), 255) with x = dE - T in the heat mode and dE in the plain mode.
// The record: the histogram is counted in LDS (zeros in a register) and flushed with one atomic per non-empty bin; a thread adds its
// pixels' dE in float64 in pixel order, the workgroup sums in ssim_window.h's fixed order into partials[frame][chunk], and
// k_delta_e_final adds a frame's partials in index order: no float atomics.  The largest dE is one 64-bit integer maximum over
// (float bits of dE << 32) | (0xFFFFFFFF - pixel index): dE is never negative, so its bits order as its value, and among equals the
// earlier pixel wins; the key lies in the bytes of (max_de, max_x) until k_delta_e_final takes it apart.
// The Lab transfer function, ciede2000, the key, a thread's tally, the workgroup's share of the record, the map's colour and the
// host side's checks and launch frame are delta_e_common.h's, shared with the four other colour difference entries.  k_delta_e_final,
// which finishes the records of all five, is defined here and nowhere else: they reach it through avx_delta_e_final_launch.
#include "delta_e_common.h"
#include "delta_e_walk.h"

namespace {

// M': the sRGB -> XYZ (D65) matrix with every row divided by its own sum; columns 0 and 2, the anchored form needs no other
constexpr float kX0 = (float)(0.4124564 / kSX), kX2 = (float)(0.1804375 / kSX);
constexpr float kY0 = (float)(0.2126729 / kSY), kY2 = (float)(0.0721750 / kSY);
constexpr float kZ0 = (float)(0.0193339 / kSZ), kZ2 = (float)(0.9503041 / kSZ);

// r, g, b: decoded (linear) samples.  t_i = g + M'_i0 (r - g) + M'_i2 (b - g): r = g = b gives t_X = t_Y = t_Z = g exactly, a = b = 0
__device__ __forceinline__ void lab_of(float r, float g, float b, float& L, float& A, float& B) {
    const float dr = r - g, db = b - g;
    const float fx = lab_f((g + kX0 * dr) + kX2 * db);
    const float fy = lab_f((g + kY0 * dr) + kY2 * db);
    const float fz = lab_f((g + kZ0 * dr) + kZ2 * db);
    L = 116.0f * fy - 16.0f;
    A = 500.0f * (fx - fy);
    B = 200.0f * (fy - fz);
}

// dE00 of two pixels whose codes differ
struct Ciede {
    __device__ __forceinline__ float operator()(const float* lut, int ar, int ag, int ab, int br, int bg, int bb) const {
        float L1, a1, b1, L2, a2, b2;
        lab_of(lut[ar], lut[ag], lut[ab], L1, a1, b1);
        lab_of(lut[br], lut[bg], lut[bb], L2, a2, b2);
        return ciede2000(L1, a1, b1, L2, a2, b2);
    }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_delta_e(DeArgs p) {
    de_chunk_walk<VEC>(p, Ciede());
}

// grid (frames): the body is delta_e_common.h's de_final
__global__ __launch_bounds__(kThreads) void k_delta_e_final(const double* __restrict__ partials, size_t n_partials, int W, avx_delta_e_rec* __restrict__ rec) {
    de_final(partials, n_partials, W, rec);
}

static_assert(sizeof(avx_delta_e_rec) == 1048 && offsetof(avx_delta_e_rec, max_de) == 1032, "avx_delta_e_rec: the key needs 8 aligned bytes at max_de");

}  // namespace

int avx_delta_e_final_launch(avx_ctx* ctx, const double* partials, size_t n_partials, int W, avx_delta_e_rec* rec_dev, int n_frames, hipStream_t s) {
    hipLaunchKernelGGL(k_delta_e_final, dim3(n_frames), dim3(kThreads), 0, s, partials, n_partials, W, rec_dev);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_delta_e_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold,
                              int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream) {
    static const char fn[] = "avx_delta_e_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, layout, rec_dev, de_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, a_hwc, b_hwc, n_frames, H, W, layout, map_out)) return rc;
    return de_walk_launch(ctx, a_hwc, b_hwc, n_frames, H, W, mode, gain, threshold, layout, map_out, rec_dev, de_out, stream,
                          [](bool vec, dim3 grid, hipStream_t s, const DeArgs& p) {
                              if (vec) hipLaunchKernelGGL(k_delta_e<true>, grid, dim3(kThreads), 0, s, p);
                              else hipLaunchKernelGGL(k_delta_e<false>, grid, dim3(kThreads), 0, s, p);
                          });
}
