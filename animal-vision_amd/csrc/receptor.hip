// csrc/receptor.hip -- receptor-noise-limited colour distance maps on the device (Vorobyev & Osorio 1998; the definition
// is include/avx.h's): per pixel of two uint8 sRGB batches the distance dS, in just-noticeable differences, between the two colours as
// an observer with K = 2, 3 or 4 receptor classes tells them apart -- as a float32 plane, as a picture and as a record per frame,
// which are avx_delta_e_u8's in every respect but the value.
//
// k_receptor<K>: the chunk walk is delta_e_walk.h's one copy, shared with delta_e.hip, and the map, the record and the host side's checks
// and launch frame are delta_e_common.h's, shared with all the colour difference entries; the value of a pixel is
// this file's: the K catches of both pixels (the decode table in LDS, the anchored matrix form: a grey has every catch equal to g), K
// divisions and K logf for the contrasts, and the quadratic form of their differences (receptor_common.h's Rnl<K>, shared with
// receptor_acuity.hip).  The observer's constants -- the normalised matrix, the weights of the pairs and the reciprocal of the
// denominator, formed on the host in double and rounded once -- are kernel arguments; the kernel is instantiated on K so that the loops
// over classes and pairs unroll.
#include "delta_e_common.h"
#include "delta_e_walk.h"
#include "receptor_common.h"

namespace {

template <int K, bool VEC>
__global__ __launch_bounds__(kThreads) void k_receptor(DeArgs p, RnlArgs c) {
    de_chunk_walk<VEC>(p, Rnl<K>{c});
}

template <int K>
void launch_receptor(bool vec, dim3 grid, hipStream_t s, const DeArgs& p, const RnlArgs& c) {
    if (vec) hipLaunchKernelGGL((k_receptor<K, true>), grid, dim3(kThreads), 0, s, p, c);
    else hipLaunchKernelGGL((k_receptor<K, false>), grid, dim3(kThreads), 0, s, p, c);
}

}  // namespace

extern "C" int avx_receptor_delta_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                     int mode, float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out,
                                     void* stream) {
    static const char fn[] = "avx_receptor_delta_u8";
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, fn, n_frames, H, W, mode, gain, threshold, layout, rec_dev, ds_out)) return rc;
    if (const int rc = de_check_pair(ctx, fn, a_hwc, b_hwc, n_frames, H, W, layout, map_out)) return rc;
    RnlArgs c;
    int K;
    if (const int rc = rnl_constants(ctx, fn, obs, c, K)) return rc;

    return de_walk_launch(ctx, a_hwc, b_hwc, n_frames, H, W, mode, gain, threshold, layout, map_out, rec_dev, ds_out, stream,
                          [&](bool vec, dim3 grid, hipStream_t s, const DeArgs& p) {
                              if (K == 2) launch_receptor<2>(vec, grid, s, p, c);
                              else if (K == 3) launch_receptor<3>(vec, grid, s, p, c);
                              else launch_receptor<4>(vec, grid, s, p, c);
                          });
}
