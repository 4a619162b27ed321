// csrc/mst_mfma.hip -- fused matrix-core kernels for the two GEMM neighbourhoods of an MST++ MSAB block
// (reference: ml/MST_plus_plus/predict_code/architecture/MST_Plus_Plus.py, MS_MSA :88-139, PreNorm :57-65,
// FeedForward :141-158), float16 activations with channel groups stored 32 wide (C in {32, 64, 128}).
//
//   avx_mst_qkv_gram      to_q / to_k / to_v (:118-120) + F.normalize's column norms (:127-128) + k^T q over ALL
//                         pixels (:129) in ONE pass over x: q and k never reach memory (they are consumed from the
//                         accumulators by the Gram MFMA), only v is written.  Replaces a (N x 3C) GEMM, a second
//                         pass over its output for the Gram matrix and a strided copy of v.
//   avx_mst_ln_gemm_gelu  PreNorm's LayerNorm -> FeedForward's first 1x1 conv (C -> 4C) -> GELU: the normalised
//                         row is built in registers (K = C is the whole row) and the GELU runs on the accumulators,
//                         so the (N x 4C) hidden tensor is written once instead of written, re-read and re-written.
//
// Both are HBM-streaming kernels around v_mfma_f32_32x32x8_f16: a wave owns 32 pixels at a time; its x fragment
// (lane = pixel + 32 * half, each lane C/2 CONTIGUOUS channels of its row) is operand A for "pixels x channels"
// results and operand B for "channels x pixels" results.  The K order inside the product is free, so it is chosen
// to match that contiguous load: step s, lane half h, element j  <->  input channel h*C/2 + 4s + j; the weights are
// pre-packed on the host into exactly that fragment order ([tile][step][lane] x 4 halfs, held in LDS).
//   * "pixels x channels" (q, k): D lane (channel, half) holds pixels 8*(v/4) + 4*half + v%4 -- which IS the K-layout
//     of the next MFMA's operands, so k^T q needs only a float->half pack of the accumulators.
//   * "channels x pixels" (v, hidden): the weight columns of a tile are permuted at pack time so that D lane
//     (pixel, half) holds channels 16*half + v, v = 0..15: 32 contiguous bytes per lane, 64 per pixel and tile.
// Rounding points follow the autocast pipeline of predict_torch.py:109: GEMM results are rounded to float16 before
// anything consumes them; LayerNorm statistics, the Gram accumulation and the norms are float32.
#include <hip/hip_fp16.h>

#include "avx_internal.h"
#include "mst_common.h"
#include "mst_convt_lines.h"

namespace {

constexpr int kT = 256;  // 4 waves, each marching over its own 32-pixel tiles

__device__ __forceinline__ float16_t mfma(half4_t a, half4_t b, float16_t c) { return __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float16_t mfma16(half8_t a, half8_t b, float16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// lane (p = lane & 31, h = lane >> 5) loads channels [h*C/2, (h+1)*C/2) of pixel tile*32 + p; rows past n read as zero
template <int C>
__device__ __forceinline__ void load_x(const __half* __restrict__ x, size_t tile, size_t n, int lane, half4_t (&xf)[C / 8]) {
    const int p = lane & 31, h = lane >> 5;
    const size_t row = tile * 32 + p;
    if (row < n) {
        const uint4* src = reinterpret_cast<const uint4*>(x + row * (size_t)C + h * (C / 2));
#pragma unroll
        for (int q = 0; q < C / 16; ++q) {
            const uint4 v = src[q];
            const half8_t h8 = __builtin_bit_cast(half8_t, v);
            xf[2 * q] = half4_t{h8[0], h8[1], h8[2], h8[3]};
            xf[2 * q + 1] = half4_t{h8[4], h8[5], h8[6], h8[7]};
        }
    } else {
#pragma unroll
        for (int s = 0; s < C / 8; ++s) xf[s] = half4_t{0, 0, 0, 0};
    }
}

// lane (pixel p, half h) holds channels 16h + v of a 32-channel tile: two 16-byte stores
__device__ __forceinline__ void store_tile16(__half* dst /* row base + 32*tile + 16*h */, const _Float16 (&o)[16]) {
    half8_t a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = o[i]; b[i] = o[8 + i]; }
    reinterpret_cast<uint4*>(dst)[0] = __builtin_bit_cast(uint4, a);
    reinterpret_cast<uint4*>(dst)[1] = __builtin_bit_cast(uint4, b);
}

// ---- to_q/to_k/to_v + column norms + Gram ------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kT) void k_mst_qkv(const __half* __restrict__ x, const uint2* __restrict__ wpack /*[3*HD][KS][64]*/, size_t n,
                                                __half* __restrict__ v_out /*[n][C]*/, float* __restrict__ partial /*[blocks][HD][34][32]*/) {
    constexpr int KS = C / 8, HD = C / 32, NT = 3 * HD;
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NT * KS * 64; i += kT) wl[i] = wpack[i];
    __syncthreads();
    auto W = [&](int t, int s) { return __builtin_bit_cast(half4_t, wl[(t * KS + s) * 64 + lane]); };
    float16_t G[HD];
    float nq[HD], nk[HD];
#pragma unroll
    for (int hd = 0; hd < HD; ++hd) {
#pragma unroll
        for (int v = 0; v < 16; ++v) G[hd][v] = 0.f;
        nq[hd] = 0.f;
        nk[hd] = 0.f;
    }
    const size_t ntiles = (n + 31) / 32;
    const int p = lane & 31, h = lane >> 5;
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (size_t)gridDim.x * 4) {
        half4_t xf[KS];
        load_x<C>(x, tile, n, lane, xf);
        if constexpr (C > 32) asm volatile("" ::: "memory");  // keep the weight fragments in LDS: hoisted out of this loop they cost 6*C VGPRs
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float16_t dq, dk;
#pragma unroll
            for (int v = 0; v < 16; ++v) { dq[v] = 0.f; dk[v] = 0.f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) dq = mfma(xf[s], W(hd, s), dq);        // D[pixel][q channel]
#pragma unroll
            for (int s = 0; s < KS; ++s) dk = mfma(xf[s], W(HD + hd, s), dk);   // D[pixel][k channel]
            half4_t aq[4], ak[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    aq[s4][j] = (_Float16)dq[4 * s4 + j];
                    ak[s4][j] = (_Float16)dk[4 * s4 + j];
                    const float fq = (float)aq[s4][j], fk = (float)ak[s4][j];
                    nq[hd] = __builtin_fmaf(fq, fq, nq[hd]);
                    nk[hd] = __builtin_fmaf(fk, fk, nk[hd]);
                }
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) G[hd] = mfma(ak[s4], aq[s4], G[hd]);  // G[i][j] += sum_px k[px][i] q[px][j]
        }
        const size_t row = tile * 32 + p;
        if (v_out)  // NULL: the attention tail forms v from x itself (avx_mst_attn_tail with wv): this pass only reads
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float16_t dv;
#pragma unroll
            for (int v = 0; v < 16; ++v) dv[v] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) dv = mfma(W(2 * HD + hd, s), xf[s], dv);  // D[v channel (permuted)][pixel]
            _Float16 o[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) o[v] = (_Float16)dv[v];
            if (row < n) store_tile16(v_out + row * (size_t)C + 32 * hd + 16 * h, o);
        }
    }
    // block partial: [hd][34][32] = 32 Gram rows (i = k channel, j = q channel), then sum q^2, then sum k^2
    __syncthreads();  // the weights in LDS are dead: the same bytes hold the per-wave results now
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int hd = 0; hd < HD; ++hd) {
        float* mine = red + ((size_t)wave * HD + hd) * 34 * 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) mine[(8 * (v / 4) + 4 * h + (v % 4)) * 32 + p] = G[hd][v];
        const float sq = nq[hd] + __shfl_xor(nq[hd], 32), sk = nk[hd] + __shfl_xor(nk[hd], 32);
        if (h == 0) { mine[32 * 32 + p] = sq; mine[33 * 32 + p] = sk; }
    }
    __syncthreads();
    for (int i = tid; i < HD * 34 * 32; i += kT) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[(size_t)w * HD * 34 * 32 + i];
        partial[(size_t)blockIdx.x * HD * 34 * 32 + i] = s;
    }
}

// one wave per output element over the block partials (same shape as csrc/mst.hip's: deterministic tree)
__global__ void k_mst_qkv_final(const float* __restrict__ partial, int nblocks, int heads, float* gram /*[heads][32][32]*/, float* nq /*[heads*32]*/,
                                float* nk) {
    // a wave sums FOUR neighbouring entries over the workgroups' partials: lane l takes workgroups l, l + 64, ... with 16-byte loads (a quarter
    // of each 64-byte sector it touches instead of a sixteenth: the one-entry form moved 32x the bytes it summed), then the lanes combine
    const int i0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 4, lane = threadIdx.x & 63, tot = heads * 34 * 32;
    if (i0 >= tot) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = lane; b < nblocks; b += 64) {
        const float4 v = *reinterpret_cast<const float4*>(partial + (size_t)b * tot + i0);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s.x += __shfl_xor(s.x, o); s.y += __shfl_xor(s.y, o); s.z += __shfl_xor(s.z, o); s.w += __shfl_xor(s.w, o); }
    if (lane != 0) return;
    const float r4[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + q, hd = i / (34 * 32), e = i - hd * 34 * 32, r = e >> 5, c = e & 31;
        if (r < 32) gram[(hd * 32 + r) * 32 + c] = r4[q];
        else if (r == 32) nq[hd * 32 + c] = __fsqrt_rn(r4[q]);
        else nk[hd * 32 + c] = __fsqrt_rn(r4[q]);
    }
}

// ---- LayerNorm -> 1x1 conv (C -> 4C) -> GELU -----------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kT) void k_mst_ffn1(const __half* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                 const uint2* __restrict__ wpack /*[4*HD][KS][64]*/, size_t n, __half* __restrict__ out /*[n][4C]*/) {
    constexpr int KS = C / 8, HD = C / 32, NT = 4 * HD;
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    float* gl = reinterpret_cast<float*>(smem + (size_t)NT * KS * 64 * sizeof(uint2));  // [C] gamma, [C] beta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NT * KS * 64; i += kT) wl[i] = wpack[i];
    for (int i = tid; i < C; i += kT) { gl[i] = gamma[i]; gl[C + i] = beta[i]; }
    __syncthreads();
    auto W = [&](int t, int s) { return __builtin_bit_cast(half4_t, wl[(t * KS + s) * 64 + lane]); };
    const size_t ntiles = (n + 31) / 32;
    const int p = lane & 31, h = lane >> 5;
    const float cnt = (float)(HD * 31);
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (size_t)gridDim.x * 4) {
        half4_t xf[KS];
        load_x<C>(x, tile, n, lane, xf);
        if constexpr (C > 32) asm volatile("" ::: "memory");  // weight fragments stay in LDS (see k_mst_qkv)
        // LayerNorm over the 31 real channels of every 32-wide group (channel c of this lane: h*C/2 + 4s + j; c % 32 == 31
        // is the zero padding): two-pass float32 statistics, the row is split over lanes p and p + 32
        auto is_pad = [&](int st, int j) { return ((h * (C / 2) + 4 * st + j) & 31) == 31; };
        float s1 = 0.f;
#pragma unroll
        for (int st = 0; st < KS; ++st)
#pragma unroll
            for (int j = 0; j < 4; ++j) s1 += is_pad(st, j) ? 0.f : (float)xf[st][j];
        const float mean = (s1 + __shfl_xor(s1, 32)) / cnt;
        float s2 = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = is_pad(s, j) ? 0.f : (float)xf[s][j] - mean;
                s2 = __builtin_fmaf(d, d, s2);
            }
        const float rstd = rsqrtf((s2 + __shfl_xor(s2, 32)) / cnt + eps);
        half4_t yf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const float4 g4 = *reinterpret_cast<const float4*>(gl + h * (C / 2) + 4 * s);
            const float4 b4 = *reinterpret_cast<const float4*>(gl + C + h * (C / 2) + 4 * s);
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                yf[s][j] = is_pad(s, j) ? (_Float16)0.f : (_Float16)(((float)xf[s][j] - mean) * rstd * gg[j] + bb[j]);
            }
        }
        const size_t row = tile * 32 + p;
        __half* orow = out + row * (size_t)(4 * C) + 16 * h;
#pragma unroll 2
        for (int t = 0; t < NT; ++t) {
            float16_t d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) d = mfma(W(t, s), yf[s], d);  // D[hidden channel (permuted)][pixel]
            _Float16 o[16];
#pragma unroll
            for (int v = 0; v < 16; v += 2) {
                const float2_t g = gelu_fast2(float2_t{(float)(_Float16)d[v], (float)(_Float16)d[v + 1]});
                o[v] = (_Float16)g.x;
                o[v + 1] = (_Float16)g.y;
            }
            if (row < n) store_tile16(orow + 32 * t, o);
        }
    }
}

// ---- depthwise 3x3 -> GELU -> 1x1 conv (4C -> C) -> + residual -------------------------------------------------------
// FeedForward :147-149 and the block's `+ x` (:184).  A workgroup owns a tile of ROWS rows x 32 pixels:
//   phase 1 (all 256 threads, thread = one group of 8 hidden channels x a few pixels, its 72 taps in registers for the
//            whole launch): depthwise 3x3 on ROWS-row strips straight from global memory (each input row of a strip is
//            loaded once and feeds up to three output rows), packed float32 FMAs, exact-erf GELU, float16 result into an
//            LDS tile [ROWS][32 px][4C] (row pitch padded by 16 B: the fragment reads below are conflict-free);
//   phase 2 (one (row, 32-channel output tile) per wave): the tile is operand B of "channels x pixels" MFMAs against
//            the pre-packed W2 fragments, then + residual, float16, 32 contiguous bytes per lane.
// The (N x 4C) GELU output never reaches memory.

template <int C, int ROWS, int PXT, bool PF, int MINW>
__global__ __launch_bounds__(kT, MINW) void k_mst_ffn2(const __half* __restrict__ hid /*[B][H][W][4C]*/, const float* __restrict__ w9 /*[4C][9]*/,
                                                    const uint2* __restrict__ w2pack /*[C/32][4C/8][64]*/, const __half* res /*[B][H][W][C]*/,
                                                    __half* out /*may alias res*/, int B, int H, int W) {
    constexpr int C4 = 4 * C, CV = C4 / 8, PXS = kT / CV, TW = 32 * PXT, IPT = TW / PXS, KS2 = C4 / 8, NT = C / 32;
    constexpr int PITCH = C4 * 2 + 16;  // bytes per pixel of the LDS tile
    static_assert(ROWS * PXT * NT == 4, "one (row, 32-pixel group, output tile) per wave");
    static_assert(!PF || IPT % 2 == 0, "the prefetching schedule alternates two register buffers");
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    float* w9l = reinterpret_cast<float*>(smem + (size_t)NT * KS2 * 64 * sizeof(uint2));  // [9][4C] depthwise taps, tap-major
    unsigned char* tileb = reinterpret_cast<unsigned char*>(w9l + 9 * C4);                 // [ROWS][TW][PITCH]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NT * KS2 * 64; i += kT) wl[i] = w2pack[i];
    for (int i = tid; i < 9 * C4; i += kT) { const int c = i / 9, t = i - 9 * c; w9l[t * C4 + c] = w9[i]; }
    const int cg = tid % CV, pslot = tid / CV;
    const int xt = (W + TW - 1) / TW, strips = (H + ROWS - 1) / ROWS;
    const long total = (long)B * strips * xt;
    const int p = lane & 31, h = lane >> 5;
    const int mr = wave / (PXT * NT), mp = (wave / NT) % PXT, mt = wave % NT;  // phase 2: this wave's row, 32-pixel group and output-channel tile
    struct Pos { int x0, y0; long b; };
    auto pos_of = [&](long tile) { return Pos{(int)(tile % xt) * TW, (int)((tile / xt) % strips) * ROWS, tile / ((long)xt * strips)}; };
    // Branch-free loads: every tap reads a CLAMPED (always valid) address and out-of-image taps are zeroed with a select when
    // they are consumed, so all 3 * (ROWS + 2) loads of an item are in flight together (a guarded load per tap made each one
    // wait for the previous).  Latency is hidden by occupancy: the taps live in LDS, not in 72 registers per thread.
    auto issue = [&](const Pos& t, int i, uint4 (&raw)[ROWS + 2][3]) {
        const int xw = t.x0 + pslot + PXS * i, xc = xw < W ? xw : W - 1;
#pragma unroll
        for (int rr = 0; rr < ROWS + 2; ++rr) {  // input row y0 - 1 + rr
            const int yy = t.y0 - 1 + rr;
            const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
            const __half* rowp = hid + ((t.b * H + yc) * (size_t)W) * C4 + (size_t)cg * 8;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = xc + kx - 1;
                const int xxc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
                raw[rr][kx] = *reinterpret_cast<const uint4*>(rowp + (size_t)xxc * C4);
            }
        }
    };
    auto consume = [&](const Pos& t, int i, const uint4 (&raw)[ROWS + 2][3]) {
        const int px = pslot + PXS * i, xw = t.x0 + px, xc = xw < W ? xw : W - 1;
        const bool interior = t.x0 > 0 && t.x0 + TW < W && t.y0 > 0 && t.y0 + ROWS < H;  // uniform: no tap leaves the image
        float2_t acc[ROWS][4];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = float2_t{0.f, 0.f};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            float2_t wt[3][4];  // this tap column's weights (LDS; lanes of one channel group read the same 32 bytes)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float4 a = *reinterpret_cast<const float4*>(w9l + (ky * 3 + kx) * C4 + cg * 8);
                const float4 c = *reinterpret_cast<const float4*>(w9l + (ky * 3 + kx) * C4 + cg * 8 + 4);
                wt[ky][0] = float2_t{a.x, a.y}; wt[ky][1] = float2_t{a.z, a.w}; wt[ky][2] = float2_t{c.x, c.y}; wt[ky][3] = float2_t{c.z, c.w};
            }
            const int xx = xc + kx - 1;
            const bool xok = xx >= 0 && xx < W;
#pragma unroll
            for (int rr = 0; rr < ROWS + 2; ++rr) {
                const int yy = t.y0 - 1 + rr;
                uint4 rw = raw[rr][kx];
                if (!interior) {
                    const bool ok = xok && yy >= 0 && yy < H;
                    rw.x = ok ? rw.x : 0u; rw.y = ok ? rw.y : 0u; rw.z = ok ? rw.z : 0u; rw.w = ok ? rw.w : 0u;
                }
                const half8_t h8 = __builtin_bit_cast(half8_t, rw);
                float2_t f[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) f[q] = float2_t{(float)h8[2 * q], (float)h8[2 * q + 1]};
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {  // this input row is tap row ky of output row r = rr - ky
                    const int r = rr - ky;
                    if (r < 0 || r >= ROWS) continue;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[r][q] = __builtin_elementwise_fma(f[q], wt[ky][q], acc[r][q]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            half8_t o;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float2_t g = gelu_fast2(acc[r][q]);
                o[2 * q] = (_Float16)g.x;
                o[2 * q + 1] = (_Float16)g.y;
            }
            *reinterpret_cast<uint4*>(tileb + ((size_t)r * TW + px) * PITCH + cg * 16) = __builtin_bit_cast(uint4, o);
        }
    };
    for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const Pos t = pos_of(tile);
        __syncthreads();  // phase 2 of the previous tile is done with the LDS tile (and the tables are loaded, first time round)
        // Two schedules, picked per channel count by measurement (1080p: C = 32 385 vs 405 us, C = 64 261 vs 223 us):
        //  PF = false: one item at a time, <= 168 VGPRs, three workgroups per CU hide the load latency;
        //  PF = true : the next item's taps are loaded into a second register buffer while this one computes (252 VGPRs, two
        //              workgroups per CU).  The items are unrolled so the loads in flight can be counted: across a loop
        //              back-edge the compiler falls back to s_waitcnt vmcnt(0) and the prefetch is serialised.
        if constexpr (!PF) {
#pragma unroll 1
            for (int i = 0; i < IPT; ++i) {
                uint4 raw[ROWS + 2][3];
                issue(t, i, raw);
                consume(t, i, raw);
            }
        } else {
            uint4 rawA[ROWS + 2][3], rawB[ROWS + 2][3];
            issue(t, 0, rawA);
#pragma unroll
            for (int i = 0; i < IPT; i += 2) {  // straight-line code: the compiler counts the loads in flight (vmcnt) exactly
                issue(t, i + 1, rawB);
                consume(t, i, rawA);
                if (i + 2 < IPT) issue(t, i + 2, rawA);
                consume(t, i + 1, rawB);
            }
        }
        __syncthreads();
        {
            float16_t d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.f;
            const unsigned char* src = tileb + ((size_t)mr * TW + mp * 32 + p) * PITCH + h * (C4 / 2) * 2;  // this lane's 2C contiguous hidden channels
#pragma unroll
            for (int s2 = 0; s2 < KS2 / 2; ++s2) {
                const half8_t h8 = __builtin_bit_cast(half8_t, *reinterpret_cast<const uint4*>(src + 16 * s2));
                const half4_t b0 = half4_t{h8[0], h8[1], h8[2], h8[3]}, b1 = half4_t{h8[4], h8[5], h8[6], h8[7]};
                d = mfma(__builtin_bit_cast(half4_t, wl[(mt * KS2 + 2 * s2) * 64 + lane]), b0, d);
                d = mfma(__builtin_bit_cast(half4_t, wl[(mt * KS2 + 2 * s2 + 1) * 64 + lane]), b1, d);
            }
            const int yo = t.y0 + mr, xw = t.x0 + mp * 32 + p;
            if (yo < H && xw < W) {
                const size_t off = ((t.b * H + yo) * (size_t)W + xw) * C + 32 * mt + 16 * h;
                const half8_t r0 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(res + off)[0]);
                const half8_t r1 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(res + off)[1]);
                _Float16 o[16];
#pragma unroll
                for (int v = 0; v < 8; ++v) { o[v] = (_Float16)(d[v] + (float)r0[v]); o[8 + v] = (_Float16)(d[8 + v] + (float)r1[v]); }
                store_tile16(out + off, o);
            }
        }
    }
}

// ---- out = [add +] a @ W [+ a2 @ W2] (C -> C) --------------------------------------------------------------------
// MS_MSA's fused `attn @ v -> proj` (one C x C matrix per frame) accumulated onto pos_emb + x, and the decoder's 1x1
// fusion conv over [up | skip] (:257) as two half-K products (the concatenated tensor is never built).
template <int C>
__global__ __launch_bounds__(kT) void k_mst_rowgemm_add(const __half* __restrict__ a, const uint2* __restrict__ wpack /*[C/32][KS][64]*/,
                                                        const __half* __restrict__ a2 /*or NULL*/, const uint2* __restrict__ wpack2, const __half* add /*or NULL*/,
                                                        __half* out /*may alias add*/, size_t n) {
    constexpr int KS = C / 8, NT = C / 32;
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    uint2* wl2 = wl + NT * KS * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NT * KS * 64; i += kT) { wl[i] = wpack[i]; if (a2) wl2[i] = wpack2[i]; }
    __syncthreads();
    const size_t ntiles = (n + 31) / 32;
    const int p = lane & 31, h = lane >> 5;
    for (size_t tile = (size_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (size_t)gridDim.x * 4) {
        half4_t xf[KS], xg[KS];
        load_x<C>(a, tile, n, lane, xf);
        if (a2) load_x<C>(a2, tile, n, lane, xg);
        const size_t row = tile * 32 + p;
        if constexpr (C > 32) asm volatile("" ::: "memory");  // weight fragments stay in LDS (see k_mst_qkv)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const size_t off = row * (size_t)C + 32 * t + 16 * h;
            half8_t r0 = {0, 0, 0, 0, 0, 0, 0, 0}, r1 = r0;
            if (add && row < n) {
                r0 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(add + off)[0]);
                r1 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(add + off)[1]);
            }
            float16_t d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) d = mfma(__builtin_bit_cast(half4_t, wl[(t * KS + s) * 64 + lane]), xf[s], d);
            if (a2) {
#pragma unroll
                for (int s = 0; s < KS; ++s) d = mfma(__builtin_bit_cast(half4_t, wl2[(t * KS + s) * 64 + lane]), xg[s], d);
            }
            _Float16 o[16];
#pragma unroll
            for (int v = 0; v < 8; ++v) { o[v] = (_Float16)(d[v] + (float)r0[v]); o[8 + v] = (_Float16)(d[8 + v] + (float)r1[v]); }
            if (row < n) store_tile16(out + off, o);
        }
    }
}

template <int C>
int launch_rowgemm_add(avx_ctx* ctx, const void* a, const void* wpack, const void* a2, const void* wpack2, const void* add, void* out, size_t n, hipStream_t s) {
    constexpr int KS = C / 8, NT = C / 32;
    const size_t lds = (size_t)2 * NT * KS * 64 * sizeof(uint2);
    const size_t ntiles = (n + 31) / 32;
    long blocks = (long)((ntiles + 3) / 4);
    const long cap = (long)ctx->num_cus * (C == 128 ? 2 : 8);
    if (blocks > cap) blocks = cap;
    auto k = k_mst_rowgemm_add<C>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)a, (const uint2*)wpack, (const __half*)a2, (const uint2*)wpack2,
                       (const __half*)add, (__half*)out, n);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

// ---- attention matrix -> fused projection weight, in fragment order -----------------------------------------------------
// MS_MSA :127-135 after the Gram pass: attn = softmax_j((k_i . q_j) / (|k_i| |q_j|) * rescale) per head (F.normalize's
// eps = 1e-12 on the norms; the padding column 31 takes no part), then M = blockdiag(attn_h^T) @ W_proj^T so that
// proj(attn @ v) == v @ M.  One small launch instead of a dozen elementwise ones; M leaves already packed for
// k_mst_rowgemm_add ("channels x pixels" fragments, see the header).
__global__ __launch_bounds__(256) void k_mst_attn_pack(const float* __restrict__ gram /*[HD][32][32]*/, const float* __restrict__ nq, const float* __restrict__ nk,
                                                       const float* __restrict__ rescale /*[HD]*/, const float* __restrict__ wpt /*[C][C] = W_proj^T*/, int C,
                                                       __half* __restrict__ mpack /*[C/32][C/8][64][4] | layout 1: [C/32][C/16][64][8]*/, int layout) {
    __shared__ float A[4][32][33];
    const int HD = C / 32, KS = C / 8, tid = threadIdx.x;
    for (int idx = tid; idx < HD * 1024; idx += 256) {
        const int hd = idx >> 10, i = (idx >> 5) & 31, j = idx & 31;
        A[hd][i][j] = gram[idx] / (fmaxf(nk[hd * 32 + i], 1e-12f) * fmaxf(nq[hd * 32 + j], 1e-12f)) * rescale[hd];
    }
    __syncthreads();
    if (tid < HD * 32) {
        float* row = A[tid >> 5][tid & 31];
        float m = row[0];
        for (int j = 1; j < 31; ++j) m = fmaxf(m, row[j]);
        float sum = 0.f;
        for (int j = 0; j < 31; ++j) { const float e = __expf(row[j] - m); row[j] = e; sum += e; }
        const float inv = 1.0f / sum;
        for (int j = 0; j < 31; ++j) row[j] *= inv;
        row[31] = 0.f;
    }
    __syncthreads();
    {  // every block repeats the (tiny) softmax above and then packs its own 256 entries of M
        const int idx = blockIdx.x * 256 + tid;
        int k = 0, n = 0;
        if (layout == 0) {  // v_mfma_f32_32x32x8_f16 fragments of k_mst_rowgemm_add
            const int e = idx & 3, lane = (idx >> 2) & 63, s = (idx >> 8) % KS, t = (idx >> 8) / KS;
            const int hh = lane >> 5, m = lane & 31;
            k = hh * (C / 2) + 4 * s + e;                                    // input channel (row of M)
            n = 32 * t + 16 * ((m & 7) >> 2) + 4 * (m >> 3) + (m & 3);       // output channel (column of M)
        } else if (layout == 1) {  // v_mfma_f32_32x32x16_f16 fragments of k_mst_attn_tail (csrc/mst_fused.hip): lane half hh carries input channels
                  // [hh C/2, (hh + 1) C/2) in steps of 8, and a result lane (pixel, hd) ends up with output channels hd C/2 + 16 t + v
            const int e = idx & 7, lane = (idx >> 3) & 63, s = (idx >> 9) % (C / 16), t = (idx >> 9) / (C / 16);
            const int hh = lane >> 5, m = lane & 31;
            k = hh * (C / 2) + 8 * s + e;
            n = ((m >> 2) & 1) * (C / 2) + 16 * t + (m & 3) + 4 * (m >> 3);
        }
        if (layout == 2) {  // block-diagonal v_mfma_f32_16x16x32_f16 fragments of k_mst_attn_tail_mx (csrc/mst_fused.hip): [C/8 octets][C/16 steps][64][8]; result row
                            // m = 8 s + c is output channel 8 o + c at tile row s, K slot q of step t2 carries row q & 1 and input channels 16 t2 + 8 (q >> 1) + e
            const int e = idx & 7, lane = (idx >> 3) & 63, t2 = (idx >> 9) % (C / 16), o = (idx >> 9) / (C / 16);
            const int m = lane & 15, q2 = lane >> 4;
            if ((q2 & 1) != (m >> 3)) { mpack[idx] = __float2half(0.f); return; }
            k = 16 * t2 + 8 * (q2 >> 1) + e;
            n = 8 * o + (m & 7);
        }
        const int hd = k >> 5, j = k & 31;
        float acc = 0.f;
        for (int i = 0; i < 32; ++i) acc = __builtin_fmaf(A[hd][i][j], wpt[(size_t)(hd * 32 + i) * C + n], acc);
        mpack[idx] = __float2half(acc);
    }
}

// ---- dense 3x3 conv (C -> C, zero padding 1) [+ add]: MST.embedding / mapping (:199, :228), conv_out (:277) ----------------
// Implicit GEMM with K = 9 taps x C: a wave owns 32 consecutive pixels of one image row; for every tap its x fragment is
// the (clamped, then zero-masked) neighbour row chunk, multiplied against that tap's pre-packed C x C weight.
template <int C>
__global__ __launch_bounds__(kT) void k_mst_conv3x3(const __half* __restrict__ x /*[B][H][W][C]*/, const uint2* __restrict__ wpack /*[9][C/32][KS][64]*/,
                                                    const __half* __restrict__ add /*or NULL*/, __half* __restrict__ out, int B, int H, int W) {
    constexpr int KS = C / 8, NT = C / 32;
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 9 * NT * KS * 64; i += kT) wl[i] = wpack[i];
    __syncthreads();
    const int xt = (W + 31) / 32;
    const long total = (long)B * H * xt;
    const int p = lane & 31, h = lane >> 5;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < total; tile += (long)gridDim.x * 4) {
        const int x0 = (int)(tile % xt) * 32, y = (int)((tile / xt) % H);
        const long b = tile / ((long)xt * H);
        const int xw = x0 + p, xc = xw < W ? xw : W - 1;
        half4_t xf[9][KS];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = xc + tap % 3 - 1;
            const int yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy), xxc = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
            const uint4* src = reinterpret_cast<const uint4*>(x + ((b * H + yc) * (size_t)W + xxc) * C + h * (C / 2));
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
            for (int q = 0; q < C / 16; ++q) {
                uint4 v = src[q];
                v.x = ok ? v.x : 0u; v.y = ok ? v.y : 0u; v.z = ok ? v.z : 0u; v.w = ok ? v.w : 0u;
                const half8_t h8 = __builtin_bit_cast(half8_t, v);
                xf[tap][2 * q] = half4_t{h8[0], h8[1], h8[2], h8[3]};
                xf[tap][2 * q + 1] = half4_t{h8[4], h8[5], h8[6], h8[7]};
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float16_t d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int s = 0; s < KS; ++s) d = mfma(__builtin_bit_cast(half4_t, wl[((tap * NT + t) * KS + s) * 64 + lane]), xf[tap][s], d);
            if (xw < W) {
                const size_t off = ((b * H + y) * (size_t)W + xw) * C + 32 * t + 16 * h;
                half8_t r0 = {0, 0, 0, 0, 0, 0, 0, 0}, r1 = r0;
                if (add) {
                    r0 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(add + off)[0]);
                    r1 = __builtin_bit_cast(half8_t, reinterpret_cast<const uint4*>(add + off)[1]);
                }
                _Float16 o[16];
#pragma unroll
                for (int v = 0; v < 8; ++v) { o[v] = (_Float16)(d[v] + (float)r0[v]); o[8 + v] = (_Float16)(d[8 + v] + (float)r1[v]); }
                store_tile16(out + off, o);
            }
        }
    }
}

// ---- pos_emb: depthwise 3x3 -> GELU -> depthwise 3x3 (+ x + bias) in one pass (MS_MSA :104-106, :136-137) ------------------
// A workgroup owns a TH x TW pixel tile: phase 1 evaluates the first conv + GELU on the (TH+2) x (TW+2) halo region into LDS
// (float16, zero outside the image: the second conv's zero padding applies to THIS map), phase 2 runs the second conv from
// LDS and adds the residual and the projection bias.  The intermediate map never reaches memory (2 of the 5 passes saved).
template <int C, int TH, int TW>
__global__ __launch_bounds__(kT) void k_mst_posemb(const __half* __restrict__ v, const float* __restrict__ w1 /*[C][9]*/, const float* __restrict__ w2 /*[C][9]*/,
                                                   const __half* __restrict__ res, const float* __restrict__ bias /*[C]*/, __half* __restrict__ out, int B, int H,
                                                   int W) {
    constexpr int CV = C / 8, PH = TH + 2, PW = TW + 2;
    static_assert(PH % 2 == 0 && kT % CV == 0, "row pairs in phase 1; fixed channel group per thread");
    extern __shared__ __align__(16) unsigned char smem[];
    __half* wl = reinterpret_cast<__half*>(smem);                                   // [2][9][C] taps, tap-major, float16 (the model's own values: the float32 table holds them exactly)
    float* bl = reinterpret_cast<float*>(wl + 2 * 9 * C);                           // [C] bias
    unsigned char* mid = reinterpret_cast<unsigned char*>(bl + C);                  // [PH][PW][C] float16
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * C; i += kT) { const int c = i / 9, t = i - 9 * c; wl[t * C + c] = __float2half(w1[i]); wl[9 * C + t * C + c] = __float2half(w2[i]); }
    for (int i = tid; i < C; i += kT) bl[i] = bias ? bias[i] : 0.f;
    const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;
    const long total = (long)B * ty * tx;
    const int cg = tid % CV;  // kT % CV == 0: a thread keeps its channel group, so each phase holds its 72 taps (nine 16-byte registers of float16) for the launch
    auto taps = [&](const __half* wbase, uint4 (&wt)[9]) {
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const uint4*>(wbase + t * C + cg * 8);
    };
    // float16 data x float16 taps, float32 accumulation: one v_fma_mix_f32 per MAC, no conversion instructions (mst_common.h)
    auto mac8 = [&](float (&acc)[8], const uint4& hv, const uint4& wv) {
        fma_mix_lo(acc[0], hv.x, wv.x); fma_mix_hi(acc[1], hv.x, wv.x);
        fma_mix_lo(acc[2], hv.y, wv.y); fma_mix_hi(acc[3], hv.y, wv.y);
        fma_mix_lo(acc[4], hv.z, wv.z); fma_mix_hi(acc[5], hv.z, wv.z);
        fma_mix_lo(acc[6], hv.w, wv.w); fma_mix_hi(acc[7], hv.w, wv.w);
    };
    __syncthreads();
    for (long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int x0 = (int)(tile % tx) * TW, y0 = (int)((tile / tx) % ty) * TH;
        const long b = tile / ((long)tx * ty);
        // every pixel phase 1 touches (rows y0 - 2 .. y0 + TH + 1, columns x0 - 2 .. x0 + TW + 1) inside the frame: no clamping, no masks
        const bool interior = y0 >= 2 && y0 + TH + 2 <= H && x0 >= 2 && x0 + TW + 2 <= W;
        __syncthreads();  // the previous tile's phase 2 is done with `mid`
        uint4 wt1[9];  // reloaded per tile and phase (nine LDS reads): resident for the launch, the two sets cost 72 registers and a wave of occupancy
        taps(wl, wt1);
#pragma unroll 1
        for (int it = tid; it < (PH / 2) * PW * CV; it += kT) {  // one item = two vertically adjacent pixels of the halo region
            const int pp = it / CV, c = pp % PW, r = 2 * (pp / PW);
            const int yy = y0 - 1 + r, xx = x0 - 1 + c;
            uint4 raw[4][3];
            if (interior) {
                const __half* base = v + ((b * H + yy - 1) * (size_t)W + xx - 1) * C + cg * 8;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) raw[rr][kx] = *reinterpret_cast<const uint4*>(base + ((size_t)rr * W + kx) * C);
            } else {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)  // branch-free: clamped addresses, out-of-image taps zeroed
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int y2 = yy - 1 + rr, x2 = xx + kx - 1;
                        const bool ok = y2 >= 0 && y2 < H && x2 >= 0 && x2 < W;
                        const int yc = y2 < 0 ? 0 : (y2 >= H ? H - 1 : y2), xc = x2 < 0 ? 0 : (x2 >= W ? W - 1 : x2);
                        uint4 rw = *reinterpret_cast<const uint4*>(v + ((b * H + yc) * (size_t)W + xc) * C + cg * 8);
                        rw.x = ok ? rw.x : 0u; rw.y = ok ? rw.y : 0u; rw.z = ok ? rw.z : 0u; rw.w = ok ? rw.w : 0u;
                        raw[rr][kx] = rw;
                    }
            }
            float acc[2][8];
#pragma unroll
            for (int o2 = 0; o2 < 2; ++o2)
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[o2][q] = 0.f;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int o2 = 0; o2 < 2; ++o2) {  // input row rr is tap row ky = rr - o2 of output o2
                        const int ky = rr - o2;
                        if (ky < 0 || ky > 2) continue;
                        mac8(acc[o2], raw[rr][kx], wt1[ky * 3 + kx]);
                    }
#pragma unroll
            for (int o2 = 0; o2 < 2; ++o2) {
                const int ym = yy + o2;
                const bool inside = interior || (ym >= 0 && ym < H && xx >= 0 && xx < W);
                unsigned o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float2_t g = gelu_fast2(float2_t{acc[o2][2 * q], acc[o2][2 * q + 1]});
                    o[q] = inside ? pack_f16(g.x, g.y) : 0u;
                }
                *reinterpret_cast<uint4*>(mid + (((size_t)(r + o2) * PW + c) * C + cg * 8) * 2) = uint4{o[0], o[1], o[2], o[3]};
            }
        }
        __syncthreads();
        uint4 wt2[9];
        taps(wl + 9 * C, wt2);
#pragma unroll 1
        for (int it = tid; it < TH * TW * CV; it += kT) {
            const int pp = it / CV, c = pp % TW, r = pp / TW;
            const int yo = y0 + r, xo = x0 + c;
            if (yo >= H || xo >= W) continue;
            float acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) mac8(acc, *reinterpret_cast<const uint4*>(mid + (((size_t)(r + t / 3) * PW + c + t % 3) * C + cg * 8) * 2), wt2[t]);
            const size_t off = ((b * H + yo) * (size_t)W + xo) * C + cg * 8;
            uint4 rr = uint4{0u, 0u, 0u, 0u};
            if (res) rr = *reinterpret_cast<const uint4*>(res + off);
            const unsigned rw[4] = {rr.x, rr.y, rr.z, rr.w};
            unsigned o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // (acc + residual) + bias, the float16 residual taken as it is (x * 1.0 + acc)
                float s0 = acc[2 * q], s1 = acc[2 * q + 1];
                fma_mix_lo(s0, rw[q], 0x3c003c00u); fma_mix_hi(s1, rw[q], 0x3c003c00u);
                o[q] = pack_f16(s0 + bl[cg * 8 + 2 * q], s1 + bl[cg * 8 + 2 * q + 1]);
            }
            *reinterpret_cast<uint4*>(out + off) = uint4{o[0], o[1], o[2], o[3]};
        }
    }
}

template <int C, int TH, int TW>
int launch_posemb(avx_ctx* ctx, const void* v, const float* w1, const float* w2, const void* res, const float* bias, void* out, int B, int H, int W, hipStream_t s) {
    const size_t lds = sizeof(__half) * 2 * 9 * C + sizeof(float) * C + (size_t)(TH + 2) * (TW + 2) * C * 2;
    const long total = (long)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    const long cap = (long)ctx->num_cus * (lds > 40 * 1024 ? 3 : 5);
    auto k = k_mst_posemb<C, TH, TW>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)(total < cap ? total : cap)), dim3(kT), lds, s, (const __half*)v, w1, w2, (const __half*)res, bias, (__half*)out, B, H, W);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

// ---- ConvTranspose2d(C -> C/2, kernel 2, stride 2) + bias: MST decoder upsampling (:214, :256) -------------------------
// Kernel size == stride: output pixel (2y + dy, 2x + dx) depends on input pixel (y, x) alone, through tap (dy, dx) -- four
// independent C x C/2 GEMMs whose results interleave in the output.  A wave takes 32 consecutive input pixels of a row and
// writes, per tap and output-channel tile, 32 contiguous bytes per lane at the scattered output pixel.
// With `skip` / `wskip` the decoder's 1x1 fusion conv over [up | skip] (:257) rides along: its `up` half is folded into the taps on
// the host (W_tap @ W_up^T, a C x C/2 matrix per tap; bias likewise) and its `skip` half is a second product on the output pixel's
// own skip row -- `up` and the concatenation never exist, and the level's input is read once instead of being written and re-read.
// GRAM (C = 64 -> 32 output channels): the Gram pass of the MSAB block that follows runs on the rounded output in registers, as in
// csrc/mst_fused.hip::k_mst_conv3x3_lds<., true> (a lane holds channels 16 h + v of its output pixel: the K = 16 operand order of k_mst_qkv16).
template <int C, bool GRAM = false>
__global__ __launch_bounds__(kT) void k_mst_convt2x2(const __half* __restrict__ x /*[B][H][W][C]*/, const uint2* __restrict__ wpack /*[4][C/64][C/8][64]*/,
                                                     const float* __restrict__ bias /*[C/2]*/, const __half* __restrict__ skip /*[B][2H][2W][C/2] or NULL*/,
                                                     const uint2* __restrict__ wskip /*[C/64][C/16][64]*/, __half* __restrict__ out /*[B][2H][2W][C/2]*/, int B,
                                                     int H, int W, const uint4* __restrict__ wqk = nullptr /*[2][2][64]*/, float* __restrict__ partial = nullptr /*[blocks][34][32]*/) {
    constexpr int KS = C / 8, CO = C / 2, NT = CO / 32, KSS = CO / 8;
    static_assert(!GRAM || C == 64, "the Gram epilogue is for the 32-channel output level");
    extern __shared__ __align__(16) unsigned char smem[];
    uint2* wl = reinterpret_cast<uint2*>(smem);
    float* bl = reinterpret_cast<float*>(smem + (size_t)4 * NT * KS * 64 * sizeof(uint2));
    uint2* wsl = reinterpret_cast<uint2*>(bl + CO);
    uint4* wq = reinterpret_cast<uint4*>(wsl + NT * KSS * 64);  // GRAM only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * NT * KS * 64; i += kT) wl[i] = wpack[i];
    for (int i = tid; i < CO; i += kT) bl[i] = bias[i];
    if (skip)
        for (int i = tid; i < NT * KSS * 64; i += kT) wsl[i] = wskip[i];
    float16_t G;
    float nq = 0.f, nk = 0.f;
    if constexpr (GRAM) {
        for (int i = tid; i < 4 * 64; i += kT) wq[i] = wqk[i];
#pragma unroll
        for (int v = 0; v < 16; ++v) G[v] = 0.f;
    }
    __syncthreads();
    const int xt = (W + 31) / 32;
    const long total = (long)B * H * xt;
    const int p = lane & 31, h = lane >> 5;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < total; tile += (long)gridDim.x * 4) {
        const int x0 = (int)(tile % xt) * 32, y = (int)((tile / xt) % H);
        const long b = tile / ((long)xt * H);
        const int xw = x0 + p;
        half4_t xf[KS];
        {
            const size_t row = (size_t)((b * H + y) * (long)W + (xw < W ? xw : W - 1));
            const uint4* src = reinterpret_cast<const uint4*>(x + row * C + h * (C / 2));
#pragma unroll
            for (int q = 0; q < C / 16; ++q) {
                const half8_t h8 = __builtin_bit_cast(half8_t, src[q]);
                xf[2 * q] = half4_t{h8[0], h8[1], h8[2], h8[3]};
                xf[2 * q + 1] = half4_t{h8[4], h8[5], h8[6], h8[7]};
            }
        }
        if constexpr (C > 64) asm volatile("" ::: "memory");  // weight fragments stay in LDS
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
            const size_t opix = ((size_t)(b * 2 * H + 2 * y + (tap >> 1)) * (size_t)(2 * W) + (size_t)(2 * (xw < W ? xw : W - 1) + (tap & 1)));
            half4_t sf[KSS];
            if (skip) {  // lane (p, h): channels [h CO/2, (h + 1) CO/2) of the OUTPUT pixel's skip row
                const uint4* src = reinterpret_cast<const uint4*>(skip + opix * CO + h * (CO / 2));
#pragma unroll
                for (int q = 0; q < CO / 16; ++q) {
                    const half8_t h8 = __builtin_bit_cast(half8_t, src[q]);
                    sf[2 * q] = half4_t{h8[0], h8[1], h8[2], h8[3]};
                    sf[2 * q + 1] = half4_t{h8[4], h8[5], h8[6], h8[7]};
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float16_t d;
#pragma unroll
                for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) d = mfma(__builtin_bit_cast(half4_t, wl[((tap * NT + t) * KS + s) * 64 + lane]), xf[s], d);
                if (skip) {
#pragma unroll
                    for (int s = 0; s < KSS; ++s) d = mfma(__builtin_bit_cast(half4_t, wsl[(t * KSS + s) * 64 + lane]), sf[s], d);
                }
                _Float16 o[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) o[v] = (_Float16)(d[v] + bl[32 * t + 16 * h + v]);
                if (xw < W) store_tile16(out + opix * CO + 32 * t + 16 * h, o);
                if constexpr (GRAM) {
                    half8_t o0, o1;
#pragma unroll
                    for (int v = 0; v < 8; ++v) { o0[v] = xw < W ? o[v] : (_Float16)0.f; o1[v] = xw < W ? o[8 + v] : (_Float16)0.f; }  // columns past the edge take no part
                    float16_t dq, dk;
#pragma unroll
                    for (int v = 0; v < 16; ++v) { dq[v] = 0.f; dk[v] = 0.f; }
                    dq = mfma16(o0, __builtin_bit_cast(half8_t, wq[0 * 64 + lane]), dq);  // D[pixel][q channel]
                    dq = mfma16(o1, __builtin_bit_cast(half8_t, wq[1 * 64 + lane]), dq);
                    dk = mfma16(o0, __builtin_bit_cast(half8_t, wq[2 * 64 + lane]), dk);  // D[pixel][k channel]
                    dk = mfma16(o1, __builtin_bit_cast(half8_t, wq[3 * 64 + lane]), dk);
                    unsigned aq[8], ak[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        aq[j] = pack_f16(dq[2 * j], dq[2 * j + 1]);
                        ak[j] = pack_f16(dk[2 * j], dk[2 * j + 1]);
                        fma_mix_lo(nq, aq[j], aq[j]); fma_mix_hi(nq, aq[j], aq[j]);
                        fma_mix_lo(nk, ak[j], ak[j]); fma_mix_hi(nk, ak[j], ak[j]);
                    }
#pragma unroll
                    for (int b2 = 0; b2 < 2; ++b2)
                        G = mfma16(__builtin_bit_cast(half8_t, uint4{ak[4 * b2], ak[4 * b2 + 1], ak[4 * b2 + 2], ak[4 * b2 + 3]}),
                                   __builtin_bit_cast(half8_t, uint4{aq[4 * b2], aq[4 * b2 + 1], aq[4 * b2 + 2], aq[4 * b2 + 3]}), G);
                }
            }
        }
    }
    if constexpr (GRAM) {  // this workgroup's partial: [34][32] = 32 Gram rows, sum q^2, sum k^2 (as k_mst_qkv16); the weights in LDS are dead
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);
        float* mine = red + (size_t)wave * 34 * 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) mine[(8 * (v / 4) + 4 * h + (v % 4)) * 32 + p] = G[v];
        const float sq = nq + __shfl_xor(nq, 32), sk = nk + __shfl_xor(nk, 32);
        if (h == 0) { mine[32 * 32 + p] = sq; mine[33 * 32 + p] = sk; }
        __syncthreads();
        for (int i = tid; i < 34 * 32; i += kT) {
            float sum = 0.f;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) sum += red[(size_t)w4 * 34 * 32 + i];
            partial[(size_t)blockIdx.x * 34 * 32 + i] = sum;
        }
    }
}

// ---- the upsampling on v_mfma_f32_32x32x16_f16 --------------------------------------------------------------------------------------------
// k_mst_convt2x2's walk, scattered 32-byte stores, bias add and rounding with the tap and skip products on the K = 16 form: a lane's contiguous
// half row as loaded (one uint4 = 8 channels) IS one K = 16 operand (step q, lane half h, element j <-> input channel h C/2 + 8 q + j), the weights
// are ml/mst_plus_plus.py::pack_fragments16(..., halfrow=True) -- the same LDS bytes as the K = 8 fragments, read 16 at a time.  Inside a wave-tile
// the x row and ALL FOUR taps' skip rows are requested in front of the first MFMA (16 more registers at C = 64, 64 at C = 128), so the products
// of tap 0 run under the loads of taps 1-3 instead of each tap paying its own round trip.  NW waves share one weight image.
// GRAM: the Gram pass of the MSAB block that follows, over the pixel's CO = C / 2 rounded output channels (HD = CO / 32 heads).  A lane holds
// channels 32 t + 16 h + v of its output pixel: at CO = 32 that is k_mst_qkv16's operand as it stands; at CO = 64 the two half-waves trade 16
// channels each (eight v_permlane32_swap per tap) and lane (p, h) ends with channels 32 h .. 32 h + 31 -- again that operand, so q and k are the
// bits k_mst_qkv16 forms from the stored row and wqk is pack_qkv16's (tiles [0, 2 HD)).  Partials are laid out as k_mst_qkv16 writes them.
template <int C, int NW, bool SKIP, bool GRAM>
__global__ __launch_bounds__(64 * NW, C == 64 ? 4 : 1) void k_mst_convt2x2_16(const __half* __restrict__ x /*[B][H][W][C]*/, const uint4* __restrict__ wpack /*[4][C/64][C/16][64]*/,
                                                            const float* __restrict__ bias /*[C/2]*/, const __half* __restrict__ skip /*[B][2H][2W][C/2]*/,
                                                            const uint4* __restrict__ wskip /*[C/64][C/32][64]*/, __half* __restrict__ out /*[B][2H][2W][C/2]*/, int B,
                                                            int H, int W, const uint4* __restrict__ wqk /*[2 HD][C/32][64]*/, float* __restrict__ partial /*[blocks][HD][34][32]*/) {
    constexpr int KS = C / 16, CO = C / 2, NT = CO / 32, KSS = CO / 16, HD = NT;
    static_assert(!GRAM || SKIP, "the Gram epilogue belongs to the fused decoder step");
    extern __shared__ __align__(16) unsigned char smem[];
    uint4* wl = reinterpret_cast<uint4*>(smem);
    float* bl = reinterpret_cast<float*>(wl + 4 * NT * KS * 64);
    uint4* wsl = reinterpret_cast<uint4*>(bl + CO);
    uint4* wq = wsl + (SKIP ? NT * KSS * 64 : 0);  // GRAM only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * NT * KS * 64; i += 64 * NW) wl[i] = wpack[i];
    for (int i = tid; i < CO; i += 64 * NW) bl[i] = bias[i];
    if constexpr (SKIP)
        for (int i = tid; i < NT * KSS * 64; i += 64 * NW) wsl[i] = wskip[i];
    float16_t G[GRAM ? HD : 1];
    float nq[GRAM ? HD : 1], nk[GRAM ? HD : 1];
    if constexpr (GRAM) {
        for (int i = tid; i < 2 * HD * KSS * 64; i += 64 * NW) wq[i] = wqk[i];
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
#pragma unroll
            for (int v = 0; v < 16; ++v) G[hd][v] = 0.f;
            nq[hd] = 0.f;
            nk[hd] = 0.f;
        }
    }
    __syncthreads();
    const int xt = (W + 31) / 32;
    const long total = (long)B * H * xt;
    const int p = lane & 31, h = lane >> 5;
    for (long tile = (long)blockIdx.x * NW + wave; tile < total; tile += (long)gridDim.x * NW) {
        const int x0 = (int)(tile % xt) * 32, y = (int)((tile / xt) % H);
        const long b = tile / ((long)xt * H);
        const int xw = x0 + p, xc = xw < W ? xw : W - 1;
        uint4 xr[KS], sr[SKIP ? 4 : 1][KSS];
        {
            const uint4* src = reinterpret_cast<const uint4*>(x + (size_t)((b * H + y) * (long)W + xc) * C + h * (C / 2));
#pragma unroll
            for (int q = 0; q < KS; ++q) xr[q] = src[q];
        }
        const size_t opix0 = (size_t)(b * 2 * H + 2 * y) * (size_t)(2 * W) + (size_t)(2 * xc);  // tap (dy, dx): + dy 2W + dx
        if constexpr (SKIP) {  // lane (p, h): channels [h CO/2, (h + 1) CO/2) of the OUTPUT pixel's skip row, all four taps in flight with x
#pragma unroll
            for (int tap = 0; tap < 4; ++tap) {
                const uint4* src = reinterpret_cast<const uint4*>(skip + (opix0 + (size_t)(tap >> 1) * (size_t)(2 * W) + (tap & 1)) * CO + h * (CO / 2));
#pragma unroll
                for (int q = 0; q < KSS; ++q) sr[tap][q] = src[q];
            }
        }
        asm volatile("" ::: "memory");  // weight fragments stay in LDS, the loads stay in front of the products
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
            const size_t opix = opix0 + (size_t)(tap >> 1) * (size_t)(2 * W) + (tap & 1);
            uint4 og[NT][2];  // the rounded output row: channels 32 t + 16 h + 8 b + j
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float16_t d;
#pragma unroll
                for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) d = mfma16(__builtin_bit_cast(half8_t, wl[((tap * NT + t) * KS + s) * 64 + lane]), __builtin_bit_cast(half8_t, xr[s]), d);
                if constexpr (SKIP) {
#pragma unroll
                    for (int s = 0; s < KSS; ++s) d = mfma16(__builtin_bit_cast(half8_t, wsl[(t * KSS + s) * 64 + lane]), __builtin_bit_cast(half8_t, sr[tap][s]), d);
                }
                _Float16 o[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) o[v] = (_Float16)(d[v] + bl[32 * t + 16 * h + v]);
                if (xw < W) store_tile16(out + opix * CO + 32 * t + 16 * h, o);
                if constexpr (GRAM) {
                    half8_t o0, o1;
#pragma unroll
                    for (int v = 0; v < 8; ++v) { o0[v] = xw < W ? o[v] : (_Float16)0.f; o1[v] = xw < W ? o[8 + v] : (_Float16)0.f; }  // columns past the edge take no part
                    og[t][0] = __builtin_bit_cast(uint4, o0);
                    og[t][1] = __builtin_bit_cast(uint4, o1);
                }
            }
            if constexpr (GRAM) {
                half8_t xq[KSS];  // k_mst_qkv16's operand: step s of lane (p, h) carries channels h CO/2 + 8 s + j of the pixel
                if constexpr (NT == 1) {
                    xq[0] = __builtin_bit_cast(half8_t, og[0][0]);
                    xq[1] = __builtin_bit_cast(half8_t, og[0][1]);
                } else {  // the half-waves trade: h = 0 gives its 16 channels of tile 1 for its partner's 16 of tile 0, and each ends with one whole tile of its pixel
                    unsigned a[8] = {og[0][0].x, og[0][0].y, og[0][0].z, og[0][0].w, og[0][1].x, og[0][1].y, og[0][1].z, og[0][1].w};
                    unsigned c[8] = {og[1][0].x, og[1][0].y, og[1][0].z, og[1][0].w, og[1][1].x, og[1][1].y, og[1][1].z, og[1][1].w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {  // v_permlane32_swap: lanes 32-63 of a <-> lanes 0-31 of c
                        const auto r = __builtin_amdgcn_permlane32_swap(a[i], c[i], false, false);
                        a[i] = r[0];
                        c[i] = r[1];
                    }
                    xq[0] = __builtin_bit_cast(half8_t, uint4{a[0], a[1], a[2], a[3]});
                    xq[1] = __builtin_bit_cast(half8_t, uint4{a[4], a[5], a[6], a[7]});
                    xq[2] = __builtin_bit_cast(half8_t, uint4{c[0], c[1], c[2], c[3]});
                    xq[3] = __builtin_bit_cast(half8_t, uint4{c[4], c[5], c[6], c[7]});
                }
#pragma unroll
                for (int hd = 0; hd < HD; ++hd) {
                    float16_t dq, dk;
#pragma unroll
                    for (int v = 0; v < 16; ++v) { dq[v] = 0.f; dk[v] = 0.f; }
#pragma unroll
                    for (int s = 0; s < KSS; ++s) dq = mfma16(xq[s], __builtin_bit_cast(half8_t, wq[(hd * KSS + s) * 64 + lane]), dq);         // D[pixel][q channel]
#pragma unroll
                    for (int s = 0; s < KSS; ++s) dk = mfma16(xq[s], __builtin_bit_cast(half8_t, wq[((HD + hd) * KSS + s) * 64 + lane]), dk);  // D[pixel][k channel]
                    unsigned aq[8], ak[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        aq[j] = pack_f16(dq[2 * j], dq[2 * j + 1]);
                        ak[j] = pack_f16(dk[2 * j], dk[2 * j + 1]);
                        fma_mix_lo(nq[hd], aq[j], aq[j]); fma_mix_hi(nq[hd], aq[j], aq[j]);
                        fma_mix_lo(nk[hd], ak[j], ak[j]); fma_mix_hi(nk[hd], ak[j], ak[j]);
                    }
#pragma unroll
                    for (int b2 = 0; b2 < 2; ++b2)
                        G[hd] = mfma16(__builtin_bit_cast(half8_t, uint4{ak[4 * b2], ak[4 * b2 + 1], ak[4 * b2 + 2], ak[4 * b2 + 3]}),
                                       __builtin_bit_cast(half8_t, uint4{aq[4 * b2], aq[4 * b2 + 1], aq[4 * b2 + 2], aq[4 * b2 + 3]}), G[hd]);
                }
            }
        }
    }
    if constexpr (GRAM) {  // this workgroup's partial: [hd][34][32] = 32 Gram rows, sum q^2, sum k^2 (as k_mst_qkv16); the weights in LDS are dead
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float* mine = red + ((size_t)wave * HD + hd) * 34 * 32;
#pragma unroll
            for (int v = 0; v < 16; ++v) mine[(8 * (v / 4) + 4 * h + (v % 4)) * 32 + p] = G[hd][v];
            const float sq = nq[hd] + __shfl_xor(nq[hd], 32), sk = nk[hd] + __shfl_xor(nk[hd], 32);
            if (h == 0) { mine[32 * 32 + p] = sq; mine[33 * 32 + p] = sk; }
        }
        __syncthreads();
        for (int i = tid; i < HD * 34 * 32; i += 64 * NW) {
            float sum = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) sum += red[(size_t)w * HD * 34 * 32 + i];
            partial[(size_t)blockIdx.x * HD * 34 * 32 + i] = sum;
        }
    }
}

// waves per workgroup and workgroups per CU of every instantiation (profiles/r12/resource_usage_mst_mfma.txt): C = 64 runs four workgroups of four
// waves per CU (the kernel is held to the 128 registers of four waves per SIMD, which it meets without spilling); C = 128 shares one weight image (72 KB, 88 KB with the q / k weights) among 8 waves: with the skip rows a wave holds 188 registers (223
// with the Gram epilogue), so one workgroup fills a CU at two waves per SIMD; at 12 and 16 waves per workgroup the compiler spills (17 .. 79 registers)
template <int C, bool SKIP, bool GRAM> struct convt16_geom {
    static constexpr int NW = C == 128 ? 8 : 4, PER_CU = C == 128 ? (SKIP ? 1 : 2) : 4;
};

template <int C, bool SKIP, bool GRAM>
int launch_convt16(avx_ctx* ctx, avx_ws* ws, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H, int W,
                   const void* wqk, float* gram, float* nq, float* nk, hipStream_t s) {
    constexpr int NW = convt16_geom<C, SKIP, GRAM>::NW, KS = C / 16, CO = C / 2, NT = CO / 32, KSS = CO / 16, HD = NT;
    size_t lds = sizeof(uint4) * ((size_t)4 * NT * KS * 64 + (SKIP ? NT * KSS * 64 : 0) + (GRAM ? 2 * HD * KSS * 64 : 0)) + sizeof(float) * CO;
    if (GRAM && lds < sizeof(float) * NW * HD * 34 * 32) lds = sizeof(float) * NW * HD * 34 * 32;  // the waves' results land where the weights were
    const long total = (long)B * H * ((W + 31) / 32);
    long blocks = (total + NW - 1) / NW;
    const long cap = (long)ctx->num_cus * convt16_geom<C, SKIP, GRAM>::PER_CU;
    if (blocks > cap) blocks = cap;
    float* partial = nullptr;
    if (GRAM) {
        int rc = avx_ensure_scratch(ctx, ws, sizeof(float) * (size_t)blocks * HD * 34 * 32);
        if (rc) return rc;
        partial = (float*)ws->d_scratch;
    }
    auto k = k_mst_convt2x2_16<C, NW, SKIP, GRAM>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * NW), lds, s, (const __half*)x, (const uint4*)wpack, bias, (const __half*)skip, (const uint4*)wskip, (__half*)out, B,
                       H, W, (const uint4*)wqk, partial);
    AVX_HIP(ctx, hipGetLastError());
    if (GRAM) return avx_mst_qkv_final_launch(ctx, partial, (int)blocks, HD, gram, nq, nk, s);
    return AVX_OK;
}

// ---- the fused upsampling with whole-line memory accesses ------------------------------------------------------------------------------------
// k_mst_convt2x2_16<C, NW, true, GRAM>'s products, roundings and Gram epilogue; what changes is how a wave-tile's two skip rows come in and its two
// output rows go out.  Above, every skip load and every store moves 16 bytes per lane out of every other pixel: 32 (C = 64) or 64 (C = 128) lines
// addressed per instruction, each line finished by four or eight instructions of two taps.  Here an output row of a wave-tile -- 64 pixels x C bytes,
// one run in `skip` and in `out` -- crosses in 1 KB pieces, one instruction a piece:
//   in    LDS-direct loads (inline asm as in csrc/mst_fused.hip::k_mst_down4x4_dma: the compiler would drain vmcnt before every LDS read) into a
//         wave-private row area; which chunk a lane fetches is permuted (csrc/mst_convt_lines.h) so that the operand reads -- one ds_read_b128 per
//         tap and step, pixel 2 p + dx -- are conflict-free.  A partial tile clamps its offsets into the run: in-range duplicates, read by no real pixel.
//   out   the rounded 32 bytes per (tap, t) are written to the same area (its operands are in registers by then), swizzled; the wave reads the run back
//         with lane l holding chunk 64 i + l and stores 1 KB per instruction; lanes past the row's end repeat its last chunk (the same bytes to the same place).
// AREAS row areas per wave: with 2 (C = 64; 16 waves, 12 with the epilogue, share one weight image) row dy of the NEXT tile is requested when row dy of
// this one has been stored, a row's products ahead of its use; with 1 (C = 128, 8 waves, 154 KB) the next row is requested as soon as this one's run
// has been read back, in front of its stores.  A wave waits for its own loads only: every row is NP loads and NP stores whatever the tile, and s_waitcnt vmcnt(n)
// leaves outstanding exactly what was issued behind the request it waits for (never more than was issued: that is what makes the count safe).  x is loaded
// into registers one tile ahead.  Tiles go wave g, g + waves, ... as above, coordinates advancing with carries.  One workgroup per CU: its Gram partial sums
// the same per-wave sums as k_mst_convt2x2_16's workgroups do, grouped differently.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // "m0 is reserved": nothing of the compiler's lives in M0 across this kernel (no indirect register indexing, no LDS-load builtin)
__device__ __forceinline__ void ln_dma16(const void* base /*the same in every lane*/, unsigned ofs, unsigned lds_base /*the same in every lane*/) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(__builtin_amdgcn_readfirstlane(lds_base)), "v"(ofs), "s"(base) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int C, bool GRAM> struct convt_ln_geom {  // NP = C / 16: the 16-byte chunks of a pixel and, a run being 64 pixels, the 1 KB pieces of a row (mst_convt_lines.h's cpp)
    static constexpr int NW = C == 128 ? 8 : GRAM ? 12 : 16, AREAS = C == 128 ? 1 : 2, KS = C / 16, CO = C / 2, NT = CO / 32, KSS = CO / 16, HD = NT, NP = C / 16, ROWB = 64 * C;
    static constexpr int WBYTES = 16 * (4 * NT * KS * 64 + NT * KSS * 64 + (GRAM ? 2 * HD * KSS * 64 : 0)) + 4 * CO;
    static constexpr int LDS = (WBYTES + 1023) / 1024 * 1024 + 1024 /*the areas start on a 1 KB boundary of the LDS*/ + NW * AREAS * ROWB;
    static_assert(LDS <= 160 * 1024 && (!GRAM || 4 * NW * HD * 34 * 32 <= LDS), "one workgroup per CU");
};
template <int C, int NW_, bool GRAM>
__global__ __launch_bounds__(64 * NW_, 1) void k_mst_convt2x2_16_ln(const __half* __restrict__ x /*[B][H][W][C]*/, const uint4* __restrict__ wpack /*[4][C/64][C/16][64]*/,
                                                                  const float* __restrict__ bias /*[C/2]*/, const __half* __restrict__ skip /*[B][2H][2W][C/2]*/,
                                                                  const uint4* __restrict__ wskip /*[C/64][C/32][64]*/, __half* __restrict__ out /*[B][2H][2W][C/2]*/, int B,
                                                                  int H, int W, const uint4* __restrict__ wqk /*[2 HD][C/32][64]*/, float* __restrict__ partial /*[blocks][HD][34][32]*/) {
    using G_ = convt_ln_geom<C, GRAM>;
    static_assert(NW_ == G_::NW, "the geometry is convt_ln_geom's");
    constexpr int NW = G_::NW, AREAS = G_::AREAS, KS = G_::KS, CO = G_::CO, NT = G_::NT, KSS = G_::KSS, HD = G_::HD, NP = G_::NP, ROWB = G_::ROWB;
    using run_t = unsigned __attribute__((ext_vector_type(4 * NP)));
    using u4_t = unsigned __attribute__((ext_vector_type(4)));
    extern __shared__ __align__(16) unsigned char smem[];
    uint4* wl = reinterpret_cast<uint4*>(smem);
    float* bl = reinterpret_cast<float*>(wl + 4 * NT * KS * 64);
    uint4* wsl = reinterpret_cast<uint4*>(bl + CO);
    uint4* wq = wsl + NT * KSS * 64;  // GRAM only
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 4 * NT * KS * 64; i += 64 * NW) wl[i] = wpack[i];
    for (int i = tid; i < CO; i += 64 * NW) bl[i] = bias[i];
    for (int i = tid; i < NT * KSS * 64; i += 64 * NW) wsl[i] = wskip[i];
    float16_t G[GRAM ? HD : 1];
    float nq[GRAM ? HD : 1], nk[GRAM ? HD : 1];
    if constexpr (GRAM) {
        for (int i = tid; i < 2 * HD * KSS * 64; i += 64 * NW) wq[i] = wqk[i];
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
#pragma unroll
            for (int v = 0; v < 16; ++v) G[hd][v] = 0.f;
            nq[hd] = 0.f;
            nk[hd] = 0.f;
        }
    }
    __syncthreads();
    const int xt = (W + 31) / 32;
    const unsigned total = (unsigned)B * (unsigned)H * (unsigned)xt;  // < 2^31: the launcher refuses more
    const int p = lane & 31, h = lane >> 5;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned a0 = __builtin_amdgcn_readfirstlane(((lds0 + (unsigned)G_::WBYTES + 1023u) & ~1023u) + (unsigned)wave * (AREAS * ROWB));  // this wave's areas, as M0 wants them
    unsigned char* const area = smem + (a0 - lds0);
    // this lane's places, fixed for the launch
    int fo[NP], ob[2][KSS], wb[2][NT][2];
    const int rb[2] = {convt_ln_out_byte(NP, lane), convt_ln_out_byte(NP, 64 + lane) - 1024};  // read-back of piece i: 1024 i + rb[i & 1] (the swizzle knows i by its parity alone)
#pragma unroll
    for (int i = 0; i < NP; ++i) fo[i] = 1024 * i + 16 * convt_ln_skip_chunk(NP, i, lane);
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
#pragma unroll
        for (int s = 0; s < KSS; ++s) ob[dx][s] = convt_ln_operand_byte(NP, p, h, dx, s);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            wb[dx][t][0] = convt_ln_out_byte(NP, (2 * p + dx) * NP + 4 * t + 2 * h);
            wb[dx][t][1] = convt_ln_out_byte(NP, (2 * p + dx) * NP + 4 * t + 2 * h + 1);
        }
    }
    // the walk: tile = (row yb = b H + y of x, column xi), this wave's first one and its stride
    const unsigned nwaves = gridDim.x * NW, first = blockIdx.x * NW + wave;
    const int sx = (int)(nwaves % (unsigned)xt), sy = (int)(nwaves / (unsigned)xt);
    int xi = (int)(first % (unsigned)xt), yb = (int)(first / (unsigned)xt);
    unsigned tile = first;
    // row dy of tile (yb, xi): the run's first byte in skip / out, and how many of its 64 C bytes are inside the row
    auto run_ofs = [&](int yb_, int xi_, int dy) { return ((size_t)(2 * yb_ + dy) * (size_t)(2 * W) + (size_t)(64 * xi_)) * (size_t)C; };
    auto run_len = [&](int xi_) { const int px = 2 * W - 64 * xi_; return (px < 64 ? px : 64) * C; };
    auto request = [&](int yb_, int xi_, int dy, int a) {  // NP loads, whatever the tile: the counts of s_waitcnt rest on it
        const char* base = reinterpret_cast<const char*>(skip) + run_ofs(yb_, xi_, dy);
        const int last = run_len(xi_) - 16;
#pragma unroll
        for (int i = 0; i < NP; ++i) ln_dma16(base, (unsigned)(fo[i] < last ? fo[i] : last), a0 + a * ROWB + i * 1024);
    };
    auto load_x = [&](int yb_, int xi_, u4_t (&r)[KS]) {
        const int xw = 32 * xi_ + p;
        const u4_t* src = reinterpret_cast<const u4_t*>(x + ((size_t)yb_ * (size_t)W + (size_t)(xw < W ? xw : W - 1)) * C + h * (C / 2));
#pragma unroll
        for (int q = 0; q < KS; ++q) r[q] = src[q];
    };
    if (tile < total) {
        u4_t xr[KS];
        load_x(yb, xi, xr);
#pragma unroll
        for (int q = 0; q < KS; ++q) asm volatile("" : "+v"(xr[q]));  // the first x has arrived HERE: left pending into the loop, the wait for it would run in front of every tile and drain the queue
        request(yb, xi, 0, 0);
        if constexpr (AREAS == 2) request(yb, xi, 1, 1);
        // What the counted waits rest on:
        //   1. every row issues exactly NP LDS-direct loads (request) and exactly NP stores, whatever the tile: partial, last of the walk, or whole;
        //   2. behind the request a row waits for, at least AREAS * NP of those have been issued when it waits: AREAS == 2: the NP stores of the row before and the
        //      NP loads of the next request; AREAS == 1: the NP stores of the row before (the request goes in front of them);
        //   3. anything else in between (the x loads) only makes vmcnt(AREAS * NP) wait for more, never for less: the counter retires in issue order.
        // The wave's first row has fewer operations behind it, so it is waited for here, outright; from then on every wait is the steady state's.
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AREAS - 1) * NP) : "memory");
        for (;;) {
            int nxi = xi + sx, nyb = yb + sy;
            if (nxi >= xt) { nxi -= xt; ++nyb; }
            const bool more = tile + nwaves < total && tile + nwaves > tile;
            if (!more) { nxi = xi; nyb = yb; }  // the last tile requests itself again: valid addresses, the same number of loads
            const int xw = 32 * xi + p, lastc = run_len(xi) / 16 - 1;
            u4_t xn[KS];  // the next tile's x, requested a tile ahead: by the time it is used every wait below has long covered it
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                unsigned char* const ar = area + (AREAS == 2 ? dy : 0) * ROWB;
                // (2) above: this row's request has AREAS * NP counted operations behind it
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AREAS * NP) : "memory");
                if (dy == 0) load_x(nyb, nxi, xn);
                uint4 sr[2][KSS];
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                    for (int s = 0; s < KSS; ++s) sr[dx][s] = *reinterpret_cast<const uint4*>(ar + ob[dx][s]);
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int tap = 2 * dy + dx;
                    uint4 og[NT][2];  // the rounded output row: channels 32 t + 16 h + 8 b + j
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        float16_t d;
#pragma unroll
                        for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
                        for (int s = 0; s < KS; ++s) d = mfma16(__builtin_bit_cast(half8_t, wl[((tap * NT + t) * KS + s) * 64 + lane]), __builtin_bit_cast(half8_t, xr[s]), d);
#pragma unroll
                        for (int s = 0; s < KSS; ++s) d = mfma16(__builtin_bit_cast(half8_t, wsl[(t * KSS + s) * 64 + lane]), __builtin_bit_cast(half8_t, sr[dx][s]), d);
                        half8_t o0, o1;
#pragma unroll
                        for (int v = 0; v < 8; ++v) { o0[v] = (_Float16)(d[v] + bl[32 * t + 16 * h + v]); o1[v] = (_Float16)(d[8 + v] + bl[32 * t + 16 * h + 8 + v]); }
                        *reinterpret_cast<uint4*>(ar + wb[dx][t][0]) = __builtin_bit_cast(uint4, o0);
                        *reinterpret_cast<uint4*>(ar + wb[dx][t][1]) = __builtin_bit_cast(uint4, o1);
                        if constexpr (GRAM) {
#pragma unroll
                            for (int v = 0; v < 8; ++v) { o0[v] = xw < W ? o0[v] : (_Float16)0.f; o1[v] = xw < W ? o1[v] : (_Float16)0.f; }  // columns past the edge take no part
                            og[t][0] = __builtin_bit_cast(uint4, o0);
                            og[t][1] = __builtin_bit_cast(uint4, o1);
                        }
                    }
                    if constexpr (GRAM) {  // as in k_mst_convt2x2_16
                        half8_t xq[KSS];
                        if constexpr (NT == 1) {
                            xq[0] = __builtin_bit_cast(half8_t, og[0][0]);
                            xq[1] = __builtin_bit_cast(half8_t, og[0][1]);
                        } else {
                            unsigned a[8] = {og[0][0].x, og[0][0].y, og[0][0].z, og[0][0].w, og[0][1].x, og[0][1].y, og[0][1].z, og[0][1].w};
                            unsigned c[8] = {og[1][0].x, og[1][0].y, og[1][0].z, og[1][0].w, og[1][1].x, og[1][1].y, og[1][1].z, og[1][1].w};
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                const auto r = __builtin_amdgcn_permlane32_swap(a[i], c[i], false, false);
                                a[i] = r[0];
                                c[i] = r[1];
                            }
                            xq[0] = __builtin_bit_cast(half8_t, uint4{a[0], a[1], a[2], a[3]});
                            xq[1] = __builtin_bit_cast(half8_t, uint4{a[4], a[5], a[6], a[7]});
                            xq[2] = __builtin_bit_cast(half8_t, uint4{c[0], c[1], c[2], c[3]});
                            xq[3] = __builtin_bit_cast(half8_t, uint4{c[4], c[5], c[6], c[7]});
                        }
#pragma unroll
                        for (int hd = 0; hd < HD; ++hd) {
                            float16_t dq, dk;
#pragma unroll
                            for (int v = 0; v < 16; ++v) { dq[v] = 0.f; dk[v] = 0.f; }
#pragma unroll
                            for (int s = 0; s < KSS; ++s) dq = mfma16(xq[s], __builtin_bit_cast(half8_t, wq[(hd * KSS + s) * 64 + lane]), dq);
#pragma unroll
                            for (int s = 0; s < KSS; ++s) dk = mfma16(xq[s], __builtin_bit_cast(half8_t, wq[((HD + hd) * KSS + s) * 64 + lane]), dk);
                            unsigned aq[8], ak[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                aq[j] = pack_f16(dq[2 * j], dq[2 * j + 1]);
                                ak[j] = pack_f16(dk[2 * j], dk[2 * j + 1]);
                                fma_mix_lo(nq[hd], aq[j], aq[j]); fma_mix_hi(nq[hd], aq[j], aq[j]);
                                fma_mix_lo(nk[hd], ak[j], ak[j]); fma_mix_hi(nk[hd], ak[j], ak[j]);
                            }
#pragma unroll
                            for (int b2 = 0; b2 < 2; ++b2)
                                G[hd] = mfma16(__builtin_bit_cast(half8_t, uint4{ak[4 * b2], ak[4 * b2 + 1], ak[4 * b2 + 2], ak[4 * b2 + 3]}),
                                               __builtin_bit_cast(half8_t, uint4{aq[4 * b2], aq[4 * b2 + 1], aq[4 * b2 + 2], aq[4 * b2 + 3]}), G[hd]);
                        }
                    }
                }
                // the run as it goes to memory: lane l holds chunk 64 i + l; past the row's end it holds the row's last chunk once more and stores the same bytes to
                // the same place, so every row is NP stores, taken or not, and the waits above can count them
                run_t ov;
                int oc[NP];
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const bool in = 64 * i + lane <= lastc;
                    oc[i] = in ? 64 * i + lane : lastc;
                    const uint4 v = *reinterpret_cast<const uint4*>(ar + (in ? rb[i & 1] + 1024 * i : convt_ln_out_byte(NP, lastc)));
                    ov[4 * i] = v.x; ov[4 * i + 1] = v.y; ov[4 * i + 2] = v.z; ov[4 * i + 3] = v.w;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the area is read out: the next request may land in it
                unsigned char* const dst = reinterpret_cast<unsigned char*>(out) + run_ofs(yb, xi, dy);
                // the row to request now: AREAS == 2: row dy of the next tile; AREAS == 1: the next row, in front of this row's stores
                if constexpr (AREAS == 1) request(dy == 0 ? yb : nyb, dy == 0 ? xi : nxi, dy ^ 1, 0);
#pragma unroll
                for (int i = 0; i < NP; ++i)
                    *reinterpret_cast<uint4*>(dst + 16 * oc[i]) = uint4{ov[4 * i], ov[4 * i + 1], ov[4 * i + 2], ov[4 * i + 3]};
                if constexpr (AREAS == 2) request(nyb, nxi, dy, dy);
            }
#pragma unroll
            for (int q = 0; q < KS; ++q) asm volatile("" : "+v"(xn[q]));  // taken here, last tile or not: the loads stay where they were written, in front of both rows' stores
            if (!more) break;
#pragma unroll
            for (int q = 0; q < KS; ++q) xr[q] = xn[q];
            xi = nxi;
            yb = nyb;
            tile += nwaves;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last requests land before the area is reused below
    }
    if constexpr (GRAM) {  // this workgroup's partial, as in k_mst_convt2x2_16; the weights and the areas in LDS are dead
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float* mine = red + ((size_t)wave * HD + hd) * 34 * 32;
#pragma unroll
            for (int v = 0; v < 16; ++v) mine[(8 * (v / 4) + 4 * h + (v % 4)) * 32 + p] = G[hd][v];
            const float sq = nq[hd] + __shfl_xor(nq[hd], 32), sk = nk[hd] + __shfl_xor(nk[hd], 32);
            if (h == 0) { mine[32 * 32 + p] = sq; mine[33 * 32 + p] = sk; }
        }
        __syncthreads();
        for (int i = tid; i < HD * 34 * 32; i += 64 * NW) {
            float sum = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) sum += red[(size_t)w * HD * 34 * 32 + i];
            partial[(size_t)blockIdx.x * HD * 34 * 32 + i] = sum;
        }
    }
}

template <int C, bool GRAM>
int launch_convt16_ln(avx_ctx* ctx, avx_ws* ws, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H, int W,
                      const void* wqk, float* gram, float* nq, float* nk, hipStream_t s) {
    using G_ = convt_ln_geom<C, GRAM>;
    const long total = (long)B * H * ((W + 31) / 32);
    AVX_REQUIRE(ctx, total < 0x7fffffffl && (long)B * H * 2 < 0x7fffffffl, "avx_mst_convt2x2_fuse16_ln: %ld wave-tiles (fewer than 2^31)", total);
    long blocks = (total + G_::NW - 1) / G_::NW;
    if (blocks > ctx->num_cus) blocks = ctx->num_cus;
    float* partial = nullptr;
    if (GRAM) {
        int rc = avx_ensure_scratch(ctx, ws, sizeof(float) * (size_t)blocks * G_::HD * 34 * 32);
        if (rc) return rc;
        partial = (float*)ws->d_scratch;
    }
    auto k = k_mst_convt2x2_16_ln<C, G_::NW, GRAM>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G_::LDS));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * G_::NW), G_::LDS, s, (const __half*)x, (const uint4*)wpack, bias, (const __half*)skip, (const uint4*)wskip, (__half*)out, B,
                       H, W, (const uint4*)wqk, partial);
    AVX_HIP(ctx, hipGetLastError());
    if (GRAM) return avx_mst_qkv_final_launch(ctx, partial, (int)blocks, G_::HD, gram, nq, nk, s);
    return AVX_OK;
}

// ---- the same pass on v_mfma_f32_32x32x16_f16 (gfx950's double-rate form) ------------------------------------------------------------------
// k_mst_qkv above is BOUND by its K = 8 MFMAs (64 cycles each: 144 per 32 pixels at C = 128 is 70 us of matrix-core time per 4K launch at a
// sixteenth of the pixels, 77 us at C = 64, 93 at C = 32); the K = 16 form does the same products in a quarter of the cycles and leaves
// the pass to its one read of x.  Fragment order (ml/mst_plus_plus.py::pack_qkv16): step q, lane half h, element j <-> input channel
// h C/2 + 8 q + j -- again the order in which a lane holds its contiguous half row, one 16-byte load per step.  A "pixels x channels"
// accumulator (lane = channel, registers v <-> pixels 8 (v / 4) + 4 h + v % 4) packs into TWO K = 16 operands of the Gram MFMA (registers
// 0-7 and 8-15: the K order is free and k and q use the same one).  Norms: sum of squares of the float16-rounded values, taken from the
// packed pair by v_fma_mix_f32 (no conversion back).  NW waves per workgroup: 8 at C = 128, where the 98 KB of weights in LDS allow one
// workgroup per CU and four waves left every SIMD alone with its latencies.
template <int C, int NW>
__global__ __launch_bounds__(64 * NW) void k_mst_qkv16(const __half* __restrict__ x, const uint4* __restrict__ wpack /*[3*HD][C/16][64]*/, size_t n,
                                                      __half* __restrict__ v_out /*[n][C] or NULL*/, float* __restrict__ partial /*[blocks][HD][34][32]*/) {
    constexpr int KS = C / 16, HD = C / 32, NT = 3 * HD;
    extern __shared__ __align__(16) unsigned char smem[];
    uint4* wl = reinterpret_cast<uint4*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < NT * KS * 64; i += 64 * NW) wl[i] = wpack[i];
    __syncthreads();
    auto W = [&](int t, int s) { return __builtin_bit_cast(half8_t, wl[(t * KS + s) * 64 + lane]); };
    float16_t G[HD];
    float nq[HD], nk[HD];
#pragma unroll
    for (int hd = 0; hd < HD; ++hd) {
#pragma unroll
        for (int v = 0; v < 16; ++v) G[hd][v] = 0.f;
        nq[hd] = 0.f;
        nk[hd] = 0.f;
    }
    const size_t ntiles = (n + 31) / 32;
    const int p = lane & 31, h = lane >> 5;
    auto load_row = [&](size_t tile, uint4 (&u)[KS]) {  // rows past the end: the last row's bytes, zeroed when they are used
        const size_t row = tile * 32 + p;
        const uint4* src = reinterpret_cast<const uint4*>(x + (row < n ? row : n - 1) * (size_t)C + h * (C / 2));
#pragma unroll
        for (int q = 0; q < KS; ++q) u[q] = src[q];
    };
    constexpr bool PF = C <= 64;  // next tile's row in flight under this tile's MFMAs (C = 128: the registers go to the four Gram accumulators)
    uint4 xn[KS];
    size_t tile = (size_t)blockIdx.x * NW + wave;
    if (PF && tile < ntiles) load_row(tile, xn);
    for (; tile < ntiles; tile += (size_t)gridDim.x * NW) {
        const size_t row = tile * 32 + p;
        half8_t xf[KS];
        if (!PF) load_row(tile, xn);
#pragma unroll
        for (int q = 0; q < KS; ++q) xf[q] = __builtin_bit_cast(half8_t, row < n ? xn[q] : uint4{0u, 0u, 0u, 0u});
        if (PF && tile + (size_t)gridDim.x * NW < ntiles) load_row(tile + (size_t)gridDim.x * NW, xn);
        if constexpr (C > 32) asm volatile("" ::: "memory");  // keep the weight fragments in LDS: hoisted out of this loop they cost 6 C VGPRs
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float16_t dq, dk;
#pragma unroll
            for (int v = 0; v < 16; ++v) { dq[v] = 0.f; dk[v] = 0.f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) dq = mfma16(xf[s], W(hd, s), dq);        // D[pixel][q channel]
#pragma unroll
            for (int s = 0; s < KS; ++s) dk = mfma16(xf[s], W(HD + hd, s), dk);   // D[pixel][k channel]
            unsigned aq[8], ak[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                aq[j] = pack_f16(dq[2 * j], dq[2 * j + 1]);
                ak[j] = pack_f16(dk[2 * j], dk[2 * j + 1]);
                fma_mix_lo(nq[hd], aq[j], aq[j]); fma_mix_hi(nq[hd], aq[j], aq[j]);
                fma_mix_lo(nk[hd], ak[j], ak[j]); fma_mix_hi(nk[hd], ak[j], ak[j]);
            }
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2)  // G[i][j] += sum_px k[px][i] q[px][j], 16 pixels per instruction
                G[hd] = mfma16(__builtin_bit_cast(half8_t, uint4{ak[4 * b2], ak[4 * b2 + 1], ak[4 * b2 + 2], ak[4 * b2 + 3]}),
                               __builtin_bit_cast(half8_t, uint4{aq[4 * b2], aq[4 * b2 + 1], aq[4 * b2 + 2], aq[4 * b2 + 3]}), G[hd]);
        }
        if (v_out)  // NULL: the attention tail forms v from x itself (avx_mst_attn_tail_x): this pass only reads
#pragma unroll
        for (int hd = 0; hd < HD; ++hd) {
            float16_t dv;
#pragma unroll
            for (int v = 0; v < 16; ++v) dv[v] = 0.f;
#pragma unroll
            for (int s = 0; s < KS; ++s) dv = mfma16(W(2 * HD + hd, s), xf[s], dv);  // D[v channel (permuted)][pixel]
            if (row < n) {
                unsigned o[8];
#pragma unroll
                for (int v = 0; v < 8; ++v) o[v] = pack_f16(dv[2 * v], dv[2 * v + 1]);
                uint4* dst = reinterpret_cast<uint4*>(v_out + row * (size_t)C + 32 * hd + 16 * h);
                dst[0] = uint4{o[0], o[1], o[2], o[3]};
                dst[1] = uint4{o[4], o[5], o[6], o[7]};
            }
        }
    }
    // block partial: [hd][34][32] = 32 Gram rows (i = k channel, j = q channel), then sum q^2, then sum k^2
    __syncthreads();  // the weights in LDS are dead: the same bytes hold the per-wave results now
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int hd = 0; hd < HD; ++hd) {
        float* mine = red + ((size_t)wave * HD + hd) * 34 * 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) mine[(8 * (v / 4) + 4 * h + (v % 4)) * 32 + p] = G[hd][v];
        const float sq = nq[hd] + __shfl_xor(nq[hd], 32), sk = nk[hd] + __shfl_xor(nk[hd], 32);
        if (h == 0) { mine[32 * 32 + p] = sq; mine[33 * 32 + p] = sk; }
    }
    __syncthreads();
    for (int i = tid; i < HD * 34 * 32; i += 64 * NW) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += red[(size_t)w * HD * 34 * 32 + i];
        partial[(size_t)blockIdx.x * HD * 34 * 32 + i] = s;
    }
}

template <int C, int NW>
int launch_qkv16(avx_ctx* ctx, avx_ws* ws, const void* x, const void* wpack, size_t n, void* v_out, float* gram, float* nq, float* nk, hipStream_t s) {
    constexpr int KS = C / 16, HD = C / 32;
    const size_t wbytes = (size_t)3 * HD * KS * 64 * sizeof(uint4), rbytes = sizeof(float) * NW * HD * 34 * 32;
    const size_t lds = wbytes > rbytes ? wbytes : rbytes;
    const size_t ntiles = (n + 31) / 32;
    long blocks = (long)((ntiles + NW - 1) / NW);
    long per_cu = (long)(160 * 1024 / lds);
    if (per_cu > 16 / NW * 2) per_cu = 16 / NW * 2;  // at most 8 waves per SIMD's worth of workgroups
    if (per_cu < 1) per_cu = 1;
    const long cap = (long)ctx->num_cus * per_cu;
    if (blocks > cap) blocks = cap;
    int rc = avx_ensure_scratch(ctx, ws, sizeof(float) * (size_t)blocks * HD * 34 * 32);
    if (rc) return rc;
    float* partial = (float*)ws->d_scratch;
    auto k = k_mst_qkv16<C, NW>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * NW), lds, s, (const __half*)x, (const uint4*)wpack, n, (__half*)v_out, partial);
    AVX_HIP(ctx, hipGetLastError());
    const int tot = HD * 34 * 32;
    hipLaunchKernelGGL(k_mst_qkv_final, dim3((tot / 4 * 64 + 255) / 256), dim3(256), 0, s, partial, (int)blocks, HD, gram, nq, nk);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

template <int C>
int launch_qkv(avx_ctx* ctx, avx_ws* ws, const void* x, const void* wpack, size_t n, void* v_out, float* gram, float* nq, float* nk, hipStream_t s) {
    constexpr int KS = C / 8, HD = C / 32;
    const size_t wbytes = (size_t)3 * HD * KS * 64 * sizeof(uint2), rbytes = sizeof(float) * 4 * HD * 34 * 32;
    const size_t lds = wbytes > rbytes ? wbytes : rbytes;
    const size_t ntiles = (n + 31) / 32;
    long blocks = (long)((ntiles + 3) / 4);
    const long cap = (long)ctx->num_cus * (lds > 64 * 1024 ? 1 : (lds > 32 * 1024 ? 2 : 4));
    if (blocks > cap) blocks = cap;
    int rc = avx_ensure_scratch(ctx, ws, sizeof(float) * (size_t)blocks * HD * 34 * 32);
    if (rc) return rc;
    float* partial = (float*)ws->d_scratch;
    auto k = k_mst_qkv<C>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, (const uint2*)wpack, n, (__half*)v_out, partial);
    AVX_HIP(ctx, hipGetLastError());
    const int tot = HD * 34 * 32;
    hipLaunchKernelGGL(k_mst_qkv_final, dim3((tot / 4 * 64 + 255) / 256), dim3(256), 0, s, partial, (int)blocks, HD, gram, nq, nk);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

template <int C>
int launch_ffn1(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* wpack, size_t n, void* out, hipStream_t s) {
    constexpr int KS = C / 8, HD = C / 32;
    const size_t lds = (size_t)4 * HD * KS * 64 * sizeof(uint2) + sizeof(float) * 2 * C;
    const size_t ntiles = (n + 31) / 32;
    long blocks = (long)((ntiles + 3) / 4);
    const long cap = (long)ctx->num_cus * (lds > 64 * 1024 ? 1 : (lds > 32 * 1024 ? 2 : 8));
    if (blocks > cap) blocks = cap;
    auto k = k_mst_ffn1<C>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, gamma, beta, eps, (const uint2*)wpack, n, (__half*)out);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

template <int C, int ROWS, int PXT, bool PF, int MINW>
int launch_ffn2(avx_ctx* ctx, const void* hid, const float* w9, const void* w2pack, const void* res, void* out, int B, int H, int W, hipStream_t s) {
    constexpr int C4 = 4 * C, KS2 = C4 / 8, NT = C / 32, PITCH = C4 * 2 + 16;
    const size_t lds = (size_t)NT * KS2 * 64 * sizeof(uint2) + sizeof(float) * 9 * C4 + (size_t)ROWS * 32 * PXT * PITCH;
    const long total = (long)B * ((H + ROWS - 1) / ROWS) * ((W + 32 * PXT - 1) / (32 * PXT));
    const long cap = (long)ctx->num_cus * MINW;  // resident workgroups per CU (registers / LDS)
    auto k = k_mst_ffn2<C, ROWS, PXT, PF, MINW>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)(total < cap ? total : cap)), dim3(kT), lds, s, (const __half*)hid, w9, (const uint2*)w2pack, (const __half*)res,
                       (__half*)out, B, H, W);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

}  // namespace

int avx_mst_qkv_final_launch(avx_ctx* ctx, const float* partial, int blocks, int heads, float* gram, float* nq, float* nk, hipStream_t s) {
    const int tot = heads * 34 * 32;
    hipLaunchKernelGGL(k_mst_qkv_final, dim3((tot / 4 * 64 + 255) / 256), dim3(256), 0, s, partial, blocks, heads, gram, nq, nk);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" {

int avx_mst_qkv_gram(avx_ctx* ctx, const void* x, const void* wpack, size_t n_pix, int C, void* v_out, float* gram, float* nq, float* nk, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack && gram && nq && nk && n_pix > 0, "avx_mst_qkv_gram: NULL pointer or empty tensor");  // v_out may be NULL
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_qkv_gram: C=%d (32, 64 or 128: 31-channel groups stored 32 wide)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack | (uintptr_t)v_out)) & 15u) == 0, "avx_mst_qkv_gram: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    if (C == 32) return launch_qkv<32>(ctx, ws, x, wpack, n_pix, v_out, gram, nq, nk, s);
    if (C == 64) return launch_qkv<64>(ctx, ws, x, wpack, n_pix, v_out, gram, nq, nk, s);
    return launch_qkv<128>(ctx, ws, x, wpack, n_pix, v_out, gram, nq, nk, s);
}

int avx_mst_qkv_gram16(avx_ctx* ctx, const void* x, const void* wpack16, size_t n_pix, int C, void* v_out, float* gram, float* nq, float* nk, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack16 && gram && nq && nk && n_pix > 0, "avx_mst_qkv_gram16: NULL pointer or empty tensor");  // v_out may be NULL
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_qkv_gram16: C=%d (32, 64 or 128: 31-channel groups stored 32 wide)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack16 | (uintptr_t)v_out)) & 15u) == 0, "avx_mst_qkv_gram16: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    if (C == 32) return launch_qkv16<32, 4>(ctx, ws, x, wpack16, n_pix, v_out, gram, nq, nk, s);
    if (C == 64) return launch_qkv16<64, 4>(ctx, ws, x, wpack16, n_pix, v_out, gram, nq, nk, s);
    return launch_qkv16<128, 8>(ctx, ws, x, wpack16, n_pix, v_out, gram, nq, nk, s);
}

int avx_mst_ln_gemm_gelu(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* wpack, size_t rows, int C, void* out,
                         void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && gamma && beta && wpack && out && rows > 0, "avx_mst_ln_gemm_gelu: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_ln_gemm_gelu: C=%d (32, 64 or 128: 31-channel groups stored 32 wide)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack | (uintptr_t)out)) & 15u) == 0, "avx_mst_ln_gemm_gelu: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 32) return launch_ffn1<32>(ctx, x, gamma, beta, eps, wpack, rows, out, s);
    if (C == 64) return launch_ffn1<64>(ctx, x, gamma, beta, eps, wpack, rows, out, s);
    return launch_ffn1<128>(ctx, x, gamma, beta, eps, wpack, rows, out, s);
}

int avx_mst_dw_gemm_add(avx_ctx* ctx, const void* hidden, const float* w_c9, const void* w2pack, const void* residual, void* out, int B, int H, int W,
                        int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, hidden && w_c9 && w2pack && residual && out && B > 0 && H > 0 && W > 0, "avx_mst_dw_gemm_add: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 32 || C == 64, "avx_mst_dw_gemm_add: C=%d (32 or 64)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)hidden | (uintptr_t)w2pack | (uintptr_t)residual | (uintptr_t)out)) & 15u) == 0,
                "avx_mst_dw_gemm_add: pointers must be 16-byte aligned");
    AVX_REQUIRE(ctx, hidden != out, "avx_mst_dw_gemm_add: the hidden tensor cannot be the output (the residual can)");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 32) return launch_ffn2<32, 2, 2, false, 3>(ctx, hidden, w_c9, w2pack, residual, out, B, H, W, s);
    return launch_ffn2<64, 2, 1, true, 2>(ctx, hidden, w_c9, w2pack, residual, out, B, H, W, s);
}

int avx_mst_rowgemm_add(avx_ctx* ctx, const void* a, const void* wpack, const void* a2, const void* wpack2, const void* add, void* out, size_t rows, int C,
                        void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, a && wpack && out && rows > 0 && (!a2 == !wpack2), "avx_mst_rowgemm_add: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_rowgemm_add: C=%d (32, 64 or 128)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)a | (uintptr_t)wpack | (uintptr_t)a2 | (uintptr_t)wpack2 | (uintptr_t)add | (uintptr_t)out)) & 15u) == 0,
                "avx_mst_rowgemm_add: pointers must be 16-byte aligned");
    AVX_REQUIRE(ctx, a != out && a2 != out, "avx_mst_rowgemm_add: a GEMM operand cannot be the output (the addend can)");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 32) return launch_rowgemm_add<32>(ctx, a, wpack, a2, wpack2, add, out, rows, s);
    if (C == 64) return launch_rowgemm_add<64>(ctx, a, wpack, a2, wpack2, add, out, rows, s);
    return launch_rowgemm_add<128>(ctx, a, wpack, a2, wpack2, add, out, rows, s);
}

static int attn_pack_impl(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                          int layout, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, gram && nq && nk && rescale && wproj_t && mpack, "avx_mst_attn_pack: NULL pointer");
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_attn_pack: C=%d (32, 64 or 128)", C);
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    hipLaunchKernelGGL(k_mst_attn_pack, dim3((unsigned)((layout == 2 ? 4 : 1) * C * C / 256)), dim3(256), 0, s, gram, nq, nk, rescale, wproj_t, C, (__half*)mpack, layout);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

int avx_mst_attn_pack(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                      void* stream) {
    return attn_pack_impl(ctx, gram, nq, nk, rescale, wproj_t, C, mpack, 0, stream);
}

int avx_mst_attn_pack16(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                        void* stream) {
    return attn_pack_impl(ctx, gram, nq, nk, rescale, wproj_t, C, mpack, 1, stream);
}

int avx_mst_attn_pack_mx(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                         void* stream) {
    return attn_pack_impl(ctx, gram, nq, nk, rescale, wproj_t, C, mpack, 2, stream);
}

int avx_mst_conv3x3_add(avx_ctx* ctx, const void* x, const void* wpack, const void* add, void* out, int B, int H, int W, int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack && out && B > 0 && H > 0 && W > 0, "avx_mst_conv3x3_add: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 32, "avx_mst_conv3x3_add: C=%d (32: the 31-channel full-resolution convs)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack | (uintptr_t)add | (uintptr_t)out)) & 15u) == 0, "avx_mst_conv3x3_add: pointers must be 16-byte aligned");
    AVX_REQUIRE(ctx, x != out, "avx_mst_conv3x3_add: in-place convolution is not possible");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    constexpr int KS = 4, NT = 1;
    const size_t lds = (size_t)9 * NT * KS * 64 * sizeof(uint2);
    const long total = (long)B * H * ((W + 31) / 32);
    long blocks = (total + 3) / 4;
    const long cap = (long)ctx->num_cus * 8;
    if (blocks > cap) blocks = cap;
    auto k = k_mst_conv3x3<32>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, (const uint2*)wpack, (const __half*)add, (__half*)out, B, H, W);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

int avx_mst_posemb(avx_ctx* ctx, const void* v, const float* w1_c9, const float* w2_c9, const void* residual, const float* bias, void* out, int B, int H, int W,
                   int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, v && w1_c9 && w2_c9 && out && B > 0 && H > 0 && W > 0, "avx_mst_posemb: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 32 || C == 64 || C == 128, "avx_mst_posemb: C=%d (32, 64 or 128)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)v | (uintptr_t)residual | (uintptr_t)out)) & 15u) == 0, "avx_mst_posemb: pointers must be 16-byte aligned");
    AVX_REQUIRE(ctx, v != out, "avx_mst_posemb: in-place convolution is not possible");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 32) return launch_posemb<32, 8, 32>(ctx, v, w1_c9, w2_c9, residual, bias, out, B, H, W, s);
    if (C == 64) return launch_posemb<64, 8, 16>(ctx, v, w1_c9, w2_c9, residual, bias, out, B, H, W, s);
    return launch_posemb<128, 4, 16>(ctx, v, w1_c9, w2_c9, residual, bias, out, B, H, W, s);
}

static int convt2x2_impl(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H, int W,
                         int C, void* stream);
int avx_mst_convt2x2(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, void* out, int B, int H, int W, int C, void* stream) {
    return convt2x2_impl(ctx, x, wpack, bias, nullptr, nullptr, out, B, H, W, C, stream);
}
int avx_mst_convt2x2_fuse(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H,
                          int W, int C, void* stream) {
    if (ctx && !(skip && wskip)) return avx_fail(ctx, AVX_ERR_INVALID, "avx_mst_convt2x2_fuse: skip / wskip is NULL");
    if (ctx && ((((uintptr_t)skip | (uintptr_t)wskip)) & 15u)) return avx_fail(ctx, AVX_ERR_INVALID, "avx_mst_convt2x2_fuse: pointers must be 16-byte aligned");
    return convt2x2_impl(ctx, x, wpack, bias, skip, wskip, out, B, H, W, C, stream);
}
// avx_mst_convt2x2_fuse at C = 64 (32 output channels) followed by avx_mst_qkv_gram16 (v_out = NULL) on its output, in one pass; one frame
int avx_mst_convt2x2_fuse_gram(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int H, int W, int C,
                               const void* wqk16, float* gram, float* nq, float* nk, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack && bias && skip && wskip && out && wqk16 && gram && nq && nk && H > 0 && W > 0, "avx_mst_convt2x2_fuse_gram: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 64, "avx_mst_convt2x2_fuse_gram: C=%d (64 input channels: the decoder step back to full resolution)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wskip | (uintptr_t)wqk16)) & 15u) == 0,
                "avx_mst_convt2x2_fuse_gram: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    const long total = (long)H * ((W + 31) / 32);
    long blocks = (total + 3) / 4;
    const long cap = (long)ctx->num_cus * 4;
    if (blocks > cap) blocks = cap;
    int rc = avx_ensure_scratch(ctx, ws, sizeof(float) * (size_t)blocks * 34 * 32);
    if (rc) return rc;
    float* partial = (float*)ws->d_scratch;
    size_t lds = (size_t)4 * 1 * 8 * 64 * sizeof(uint2) + sizeof(float) * 32 + (size_t)1 * 4 * 64 * sizeof(uint2) + (size_t)4 * 64 * sizeof(uint4);
    if (lds < sizeof(float) * 4 * 34 * 32) lds = sizeof(float) * 4 * 34 * 32;  // the four waves' results land where the weights were
    auto k = k_mst_convt2x2<64, true>;
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, (const uint2*)wpack, bias, (const __half*)skip, (const uint2*)wskip, (__half*)out, 1, H, W,
                       (const uint4*)wqk16, partial);
    AVX_HIP(ctx, hipGetLastError());
    return avx_mst_qkv_final_launch(ctx, partial, (int)blocks, 1, gram, nq, nk, s);
}
static int convt2x2_impl(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H, int W,
                         int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack && bias && out && B > 0 && H > 0 && W > 0, "avx_mst_convt2x2: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 64 || C == 128, "avx_mst_convt2x2: C=%d (64 or 128 input channels)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack | (uintptr_t)out)) & 15u) == 0, "avx_mst_convt2x2: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const long total = (long)B * H * ((W + 31) / 32);
    long blocks = (total + 3) / 4;
    const long cap = (long)ctx->num_cus * (C == 128 ? 2 : 8);
    if (blocks > cap) blocks = cap;
    if (C == 64) {
        const size_t lds = (size_t)4 * 1 * 8 * 64 * sizeof(uint2) + sizeof(float) * 32 + (size_t)1 * 4 * 64 * sizeof(uint2);
        AVX_HIP(ctx, hipFuncSetAttribute((const void*)k_mst_convt2x2<64, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_mst_convt2x2<64, false>), dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, (const uint2*)wpack, bias, (const __half*)skip,
                           (const uint2*)wskip, (__half*)out, B, H, W);
    } else {
        const size_t lds = (size_t)4 * 2 * 16 * 64 * sizeof(uint2) + sizeof(float) * 64 + (size_t)2 * 8 * 64 * sizeof(uint2);
        AVX_HIP(ctx, hipFuncSetAttribute((const void*)k_mst_convt2x2<128, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_mst_convt2x2<128, false>), dim3((unsigned)blocks), dim3(kT), lds, s, (const __half*)x, (const uint2*)wpack, bias, (const __half*)skip,
                           (const uint2*)wskip, (__half*)out, B, H, W);
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

// avx_mst_convt2x2 / avx_mst_convt2x2_fuse (skip and wskip16 both NULL / both given) on K = 16 MFMAs: wpack16 / wskip16 are pack_fragments16(..., halfrow=True)
int avx_mst_convt2x2_fuse16(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int B, int H, int W,
                            int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack16 && bias && out && B > 0 && H > 0 && W > 0 && (!skip == !wskip16), "avx_mst_convt2x2_fuse16: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 64 || C == 128, "avx_mst_convt2x2_fuse16: C=%d (64 or 128 input channels)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack16 | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wskip16)) & 15u) == 0,
                "avx_mst_convt2x2_fuse16: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 64) {
        if (skip) return launch_convt16<64, true, false>(ctx, nullptr, x, wpack16, bias, skip, wskip16, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
        return launch_convt16<64, false, false>(ctx, nullptr, x, wpack16, bias, nullptr, nullptr, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
    }
    if (skip) return launch_convt16<128, true, false>(ctx, nullptr, x, wpack16, bias, skip, wskip16, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
    return launch_convt16<128, false, false>(ctx, nullptr, x, wpack16, bias, nullptr, nullptr, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
}

// avx_mst_convt2x2_fuse16 followed by avx_mst_qkv_gram16 (v_out = NULL) on its C / 2 output channels (heads = C / 64), in one pass; one frame
int avx_mst_convt2x2_fuse16_gram(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int H, int W,
                                 int C, int heads, const void* wqk16, float* gram, float* nq, float* nk, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack16 && bias && skip && wskip16 && out && wqk16 && gram && nq && nk && H > 0 && W > 0, "avx_mst_convt2x2_fuse16_gram: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, (C == 64 || C == 128) && heads == C / 64, "avx_mst_convt2x2_fuse16_gram: C=%d, heads=%d (64 or 128 input channels, one head per 32 output channels)", C, heads);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack16 | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wskip16 | (uintptr_t)wqk16)) & 15u) == 0,
                "avx_mst_convt2x2_fuse16_gram: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    if (C == 64) return launch_convt16<64, true, true>(ctx, ws, x, wpack16, bias, skip, wskip16, out, 1, H, W, wqk16, gram, nq, nk, s);
    return launch_convt16<128, true, true>(ctx, ws, x, wpack16, bias, skip, wskip16, out, 1, H, W, wqk16, gram, nq, nk, s);
}

// avx_mst_convt2x2_fuse16 (with skip) / avx_mst_convt2x2_fuse16_gram with whole-line memory accesses (k_mst_convt2x2_16_ln): the same arguments, the same `out` to the bit
int avx_mst_convt2x2_fuse16_ln(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int B, int H, int W,
                               int C, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack16 && bias && out && skip && wskip16 && B > 0 && H > 0 && W > 0, "avx_mst_convt2x2_fuse16_ln: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, C == 64 || C == 128, "avx_mst_convt2x2_fuse16_ln: C=%d (64 or 128 input channels)", C);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack16 | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wskip16)) & 15u) == 0,
                "avx_mst_convt2x2_fuse16_ln: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    if (C == 64) return launch_convt16_ln<64, false>(ctx, nullptr, x, wpack16, bias, skip, wskip16, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
    return launch_convt16_ln<128, false>(ctx, nullptr, x, wpack16, bias, skip, wskip16, out, B, H, W, nullptr, nullptr, nullptr, nullptr, s);
}

int avx_mst_convt2x2_fuse16_gram_ln(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int H, int W,
                                    int C, int heads, const void* wqk16, float* gram, float* nq, float* nk, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, x && wpack16 && bias && skip && wskip16 && out && wqk16 && gram && nq && nk && H > 0 && W > 0, "avx_mst_convt2x2_fuse16_gram_ln: NULL pointer or empty tensor");
    AVX_REQUIRE(ctx, (C == 64 || C == 128) && heads == C / 64, "avx_mst_convt2x2_fuse16_gram_ln: C=%d, heads=%d (64 or 128 input channels, one head per 32 output channels)", C, heads);
    AVX_REQUIRE(ctx, ((((uintptr_t)x | (uintptr_t)wpack16 | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wskip16 | (uintptr_t)wqk16)) & 15u) == 0,
                "avx_mst_convt2x2_fuse16_gram_ln: pointers must be 16-byte aligned");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    if (C == 64) return launch_convt16_ln<64, true>(ctx, ws, x, wpack16, bias, skip, wskip16, out, 1, H, W, wqk16, gram, nq, nk, s);
    return launch_convt16_ln<128, true>(ctx, ws, x, wpack16, bias, skip, wskip16, out, 1, H, W, wqk16, gram, nq, nk, s);
}

// Where k_mst_convt2x2_16_ln's bytes sit in a wave's row area (csrc/mst_convt_lines.h, the kernel's own functions run on the host); byte offsets, any array may be NULL:
//   fetch[i * 64 + l]                          the byte of the row's run that lane l of piece i fetches; it lands at area byte 1024 i + 16 l
//   operand[(dx * KSS + s) * 64 + lane]        the area byte lane (p, h) reads as its operand of tap dx, step s (KSS = C / 32)
//   out_write[((dx * NT + t) * 2 + b) * 64 + lane]  the area byte lane (p, h) writes its channels 32 t + 16 h + 8 b ... + 7 of pixel 2 p + dx to (NT = C / 64)
//   out_read[i * 64 + l]                       the area byte lane l reads back for the run's byte 1024 i + 16 l
int avx_mst_convt_lines_map(int C, int* fetch, int* operand, int* out_write, int* out_read) {
    if (C != 64 && C != 128) return AVX_ERR_INVALID;
    const int np = C / 16, kss = C / 32, nt = C / 64;  // np: chunks per pixel = pieces per row
    for (int lane = 0; lane < 64; ++lane) {
        const int p = lane & 31, h = lane >> 5;
        for (int i = 0; i < np; ++i) {
            if (fetch) fetch[i * 64 + lane] = 1024 * i + 16 * convt_ln_skip_chunk(np, i, lane);
            if (out_read) out_read[i * 64 + lane] = convt_ln_out_byte(np, 64 * i + lane);
        }
        for (int dx = 0; dx < 2; ++dx) {
            for (int s = 0; s < kss; ++s)
                if (operand) operand[(dx * kss + s) * 64 + lane] = convt_ln_operand_byte(np, p, h, dx, s);
            for (int t = 0; t < nt; ++t)
                for (int b = 0; b < 2; ++b)
                    if (out_write) out_write[((dx * nt + t) * 2 + b) * 64 + lane] = convt_ln_out_byte(np, (2 * p + dx) * np + 4 * t + 2 * h + b);
        }
    }
    return AVX_OK;
}

}  // extern "C"
