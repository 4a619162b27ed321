// csrc/night.hip -- the dichromats at night: rod vision in front of the colour stage, tapetum bloom behind the post stage.
//
//   avx_dichromat_night_u8, per frame (oracle/cpu_ref.py functions):
//     srgb_to_linear(get_normalized_image(frame))                                   the day path's decode
//     apply_rod_vision: clip, L = 0.1 R + 0.8 G + 0.1 B, 11-tap sigma 1.2 blur of L, x = L (1 - c) + x c, clip(x boost, 0, 1) ** gamma
//     dichromat_color_stage -> post stage -> chroma compression                     as by day
//     apply_tapetum_bloom (strength > 0): mask = clip((L709 - 0.4) / 0.6, 0, 1), 25-tap sigma 3 blur of mask and frame, screen blend
//     encode_u8 through the float32 threshold table
//
//   k_night_front  tile + 5-pixel halo: decode, scotopic L -> LDS, separable 11-tap blur (reflection at the FRAME border), mix, boost,
//                  powf, colour stage in float32 -> three float32 planes per frame in the stream workspace's scratch
//   post stage     on those planes with the kernels of the float-frame routes (avx_planes_gaussian_blur_batch, avx_streak_planes_f32)
//   k_night_back   row gain and chroma compression; with bloom a tile + 12-pixel halo of mask and channels in LDS, the separable 25-tap
//                  blur of all four, screen blend; threshold-table encode -> uint8 HWC
//
// Arithmetic: float32 in source order (-ffp-contract=off), the blurs with the project's Gaussian contract (row: s = x[0] k[0], then
// s = fma(x[j], k[j], s) left to right; column: s = c k[r], then s = fma(x[+j] + x[-j], k[r+j], s)).  Held to +-1 code of the oracle
// (device powf; Cat's float64 tail is evaluated in float64 and rounded to the float32 planes).
//
// get_normalized_image's rule (a uint8 frame whose every byte is <= 1 is not divided by 255) is a whole-frame decision the front
// kernel cannot know in advance: every workgroup decodes with the table and adds what it saw to its frame's arrival word; the
// workgroup that completes the count runs the frame's tiles again with the 0/1 decode when no byte above 1 and some byte of 1 was
// seen.  Such frames are black to the eye; the second pass is one workgroup's and costs nothing where it does not run.
#include <cstdlib>

#include "dichromat_common.h"

using namespace avxk;

namespace {

constexpr int kRodR = 5, kRodK = 2 * kRodR + 1;        // gaussian_taps(11, 1.2)
constexpr int kBloomR = 12, kBloomK = 2 * kBloomR + 1;  // gaussian_taps(25, 3.0)
constexpr int kTW = 64, kTH = 32;                       // output tile of both kernels
constexpr int kFrontT = 256, kBackT = 512;
constexpr int kFrameWords = 2;                          // per frame: one 64-bit arrival word (k_night_front)
constexpr size_t kScratchCap = (size_t)1 << 30;

struct NightArgs {
    const uint8_t* in;    // uint8 HWC frames, or float32 HWC frames (in_f32)
    uint8_t* out;
    float* front;         // 3 planes per frame: what k_night_front writes
    const float* back;    // 3 planes per frame: what k_night_back reads (front, or the post stage's output)
    int H, W, tiles_x, tiles_y;
    int in_f32, cat;
    float M[9];
    double Bk[9];
    float alpha, one_minus_alpha;
    float keep_l, keep_x, boost, gamma;  // float32(1 - chroma_scale), float32(chroma_scale), ...
    float rod[kRodK];
    const float* decode_lut;
    unsigned long long* state;  // per frame: the arrival word of k_night_front, zeroed in front of every launch
    const float* row_gain;
    int row_gain_on, row_gain_clamp, chroma_enable;
    float chroma_keep, strength;
    float bloom[kBloomK];
    const float* thr;     // 255 encode thresholds + pad
};

// One tile of the front stage.  Ls: (TH + 10) x (TW + 10) scotopic L, Lr: its row pass, X: the tile's own samples for the mix -- the
// three codes of a pixel packed into a word (uint8 frames: decoded again through the table) or its three clipped linear floats (F32).
// A thread's loads of the haloed tile are all issued before the first is used: one trip to memory per tile, not one per sample.
template <bool F32, bool DARK>
__device__ void front_tile(const NightArgs& a, int f, int tile, float* Ls, float* Lr, uint32_t* X, const float* lut, uint32_t& seen_hi, uint32_t& seen_any) {
    constexpr int AW = kTW + 2 * kRodR, AH = kTH + 2 * kRodR;
    const int tid = threadIdx.x;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const size_t npx = (size_t)a.H * a.W;
    // ---- decode + clip + scotopic luminance ----
    constexpr int N1 = (AH * AW + kFrontT - 1) / kFrontT;
    auto decode_u8 = [&](uint32_t code, float& c0, float& c1, float& c2) {
        const uint32_t b0 = code & 255u, b1 = (code >> 8) & 255u, b2 = code >> 16;
        if (DARK) { c0 = b0 ? 1.0f : 0.0f; c1 = b1 ? 1.0f : 0.0f; c2 = b2 ? 1.0f : 0.0f; }
        else { c0 = lut[b0]; c1 = lut[b1]; c2 = lut[b2]; }
    };
    {
        uint32_t raw[N1][F32 ? 3 : 1];
#pragma unroll
        for (int k = 0; k < N1; ++k) {
            const int i = tid + k * kFrontT;
            const int ii = i < AH * AW ? i : 0;  // the idle lanes of the last round re-read sample 0
            const int ly = ii / AW, lx = ii - ly * AW;
            const int gy = reflect101(y0 - kRodR + ly, a.H), gx = reflect101(x0 - kRodR + lx, a.W);
            const size_t p = ((size_t)f * npx + (size_t)gy * a.W + gx) * 3;
            if constexpr (F32) {
                const uint32_t* pf = reinterpret_cast<const uint32_t*>(a.in) + p;
                raw[k][0] = pf[0]; raw[k][1] = pf[1]; raw[k][2] = pf[2];
            } else {
                raw[k][0] = (uint32_t)a.in[p] | ((uint32_t)a.in[p + 1] << 8) | ((uint32_t)a.in[p + 2] << 16);
            }
        }
#pragma unroll
        for (int k = 0; k < N1; ++k) {
            const int i = tid + k * kFrontT;
            if (i >= AH * AW) break;
            const int ly = i / AW, lx = i - ly * AW;
            const int y = ly - kRodR, x = lx - kRodR;
            const bool inner = y >= 0 && y < kTH && x >= 0 && x < kTW;
            float c0, c1, c2;
            if constexpr (F32) {
                c0 = srgb_eotf_f32(__uint_as_float(raw[k][0])); c1 = srgb_eotf_f32(__uint_as_float(raw[k][1])); c2 = srgb_eotf_f32(__uint_as_float(raw[k][2]));
            } else {
                seen_hi |= raw[k][0] & 0xfefefeu;
                seen_any |= raw[k][0];
                decode_u8(raw[k][0], c0, c1, c2);
                if (inner) X[y * kTW + x] = raw[k][0];
            }
            c0 = fminf(fmaxf(c0, 0.0f), 1.0f); c1 = fminf(fmaxf(c1, 0.0f), 1.0f); c2 = fminf(fmaxf(c2, 0.0f), 1.0f);
            Ls[i] = (0.1f * c0 + 0.8f * c1) + 0.1f * c2;
            if constexpr (F32) {
                if (inner) {
                    X[y * kTW + x] = __float_as_uint(c0); X[kTH * kTW + y * kTW + x] = __float_as_uint(c1); X[2 * kTH * kTW + y * kTW + x] = __float_as_uint(c2);
                }
            }
        }
    }
    __syncthreads();
    // ---- row pass: 4 outputs per unit from one 14-sample window ----
    for (int u = tid; u < AH * (kTW / 4); u += kFrontT) {
        const int ly = u / (kTW / 4), xs = (u - ly * (kTW / 4)) * 4;
        const float* row = Ls + ly * AW + xs;
        float w[4 + 2 * kRodR];
#pragma unroll
        for (int j = 0; j < 4 + 2 * kRodR; ++j) w[j] = row[j];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = w[i] * a.rod[0];
#pragma unroll
            for (int j = 1; j < kRodK; ++j) s = fma_t(w[i + j], a.rod[j], s);
            Lr[ly * kTW + xs + i] = s;
        }
    }
    __syncthreads();
    // ---- column pass, mix, boost, gamma, colour stage: 4 rows of one column per unit ----
    for (int u = tid; u < (kTH / 4) * kTW; u += kFrontT) {
        const int ys = (u / kTW) * 4, x = u - (u / kTW) * kTW;
        const int gx = x0 + x;
        if (gx >= a.W) continue;
        const float* col = Lr + ys * kTW + x;
        float w[4 + 2 * kRodR];
#pragma unroll
        for (int j = 0; j < 4 + 2 * kRodR; ++j) w[j] = col[j * kTW];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gy = y0 + ys + i;
            if (gy >= a.H) break;
            float s = w[i + kRodR] * a.rod[kRodR];
#pragma unroll
            for (int j = 1; j <= kRodR; ++j) s = fma_t(w[i + kRodR + j] + w[i + kRodR - j], a.rod[kRodR + j], s);
            float xin[3];
            if constexpr (F32) {
#pragma unroll
                for (int k = 0; k < 3; ++k) xin[k] = __uint_as_float(X[k * kTH * kTW + (ys + i) * kTW + x]);
            } else {
                decode_u8(X[(ys + i) * kTW + x], xin[0], xin[1], xin[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) xin[k] = fminf(fmaxf(xin[k], 0.0f), 1.0f);
            }
            float c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = s * a.keep_l + xin[k] * a.keep_x;
                v = fminf(fmaxf(v * a.boost, 0.0f), 1.0f);
                c[k] = powf(v, a.gamma);
            }
            float o0, o1, o2;
            if (!a.cat) {
                o0 = fma_t(c[2], a.M[2], fma_t(c[1], a.M[1], c[0] * a.M[0]));
                o1 = fma_t(c[2], a.M[5], fma_t(c[1], a.M[4], c[0] * a.M[3]));
                o2 = fma_t(c[2], a.M[8], fma_t(c[1], a.M[7], c[0] * a.M[6]));
            } else {  // cat_merge_stage's arithmetic (dichromat_common.h), rounded to the float32 planes
                const float l = fma_t(c[2], a.M[2], fma_t(c[1], a.M[1], c[0] * a.M[0]));
                const float m = fma_t(c[2], a.M[5], fma_t(c[1], a.M[4], c[0] * a.M[3]));
                const float sc = fma_t(c[2], a.M[8], fma_t(c[1], a.M[7], c[0] * a.M[6]));
                const float lm = a.alpha * l + a.one_minus_alpha * m;
                const double dlm = (double)lm, ds = (double)sc;
                o0 = (float)__builtin_fma(ds, a.Bk[2], __builtin_fma(dlm, a.Bk[1], dlm * a.Bk[0]));
                o1 = (float)__builtin_fma(ds, a.Bk[5], __builtin_fma(dlm, a.Bk[4], dlm * a.Bk[3]));
                o2 = (float)__builtin_fma(ds, a.Bk[8], __builtin_fma(dlm, a.Bk[7], dlm * a.Bk[6]));
            }
            float* dst = a.front + (size_t)f * npx * 3 + (size_t)gy * a.W + gx;
            dst[0] = o0; dst[npx] = o1; dst[2 * npx] = o2;
        }
    }
    __syncthreads();  // Ls / Lr / X are rewritten by the next tile
}

template <bool F32>
__global__ __launch_bounds__(kFrontT) void k_night_front(NightArgs a) {
    constexpr int AW = kTW + 2 * kRodR, AH = kTH + 2 * kRodR;
    __shared__ float Ls[AH * AW];
    __shared__ float Lr[AH * kTW];
    __shared__ uint32_t X[(F32 ? 3 : 1) * kTH * kTW];
    __shared__ float lut[256];
    __shared__ int redo;
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    if constexpr (!F32) {
        for (int i = tid; i < 256; i += kFrontT) lut[i] = a.decode_lut[i];
        __syncthreads();
    }
    uint32_t seen_hi = 0, seen_any = 0;
    front_tile<F32, false>(a, f, blockIdx.x, Ls, Lr, X, lut, seen_hi, seen_any);
    if constexpr (F32) return;  // normalised already: never the all-<=1 branch
    // Arrival: one 64-bit word per frame counts the workgroups that have finished (bits 0-20), those whose tile held a byte > 1
    // (bits 21-41) and those whose tile held a byte > 0 (bits 42-62); the workgroup whose own add completes the count reads all three
    // from that add's result.  A workgroup that saw a byte > 1 knows that the frame is divided by 255 and that no tile is ever run
    // again: it arrives without a fence.  One that did not makes its plane stores visible device-wide first (the second pass, if
    // there is one, stores to the same addresses and must come after them): every wave waits for its stores, the workgroup meets,
    // one lane releases at device scope and waits again, then adds.
    const int hi_wg = __syncthreads_or(seen_hi != 0u);
    const int any_wg = __syncthreads_or(seen_any != 0u);
    if (!hi_wg) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its plane stores have left the CU
        __syncthreads();
    }
    if (tid == 0) {
        if (!hi_wg) {  // one device-scope release for the workgroup, waited for, before the add that announces it
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned long long add = 1ull | (hi_wg ? 1ull << 21 : 0ull) | (any_wg ? 1ull << 42 : 0ull);
        const unsigned long long now = __hip_atomic_fetch_add(a.state + f, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + add;
        const bool last = (now & 0x1fffffull) == (unsigned long long)gridDim.x;
        redo = (last && ((now >> 21) & 0x1fffffull) == 0ull && (now >> 42) != 0ull) ? 1 : 0;
    }
    __syncthreads();
    if (!redo) return;
    // every byte of the frame is 0 or 1 and some are 1: get_normalized_image leaves them as 0.0 / 1.0
    const int tiles = a.tiles_x * a.tiles_y;
    for (int t = 0; t < tiles; ++t) front_tile<false, true>(a, f, t, Ls, Lr, X, lut, seen_hi, seen_any);
}

// row gain (apply_s_cone_vertical_gain) and chroma compression of one sample of the post stage's planes
__device__ __forceinline__ void back_point(const NightArgs& a, int gy, float (&v)[3]) {
    if (a.row_gain_on) {
        float b = v[2] * a.row_gain[gy];
        if (a.row_gain_clamp) b = b < 0.0f ? 0.0f : (b > 1.0f ? 1.0f : b);
        v[2] = b;
    }
    if (a.chroma_enable) {
        const float gray = ((v[0] + v[1]) + v[2]) / 3.0f;
        v[0] = gray + (v[0] - gray) * a.chroma_keep;
        v[1] = gray + (v[1] - gray) * a.chroma_keep;
        v[2] = gray + (v[2] - gray) * a.chroma_keep;
    }
}

template <bool BLOOM>
__global__ __launch_bounds__(kBackT) void k_night_back(NightArgs a) {
    constexpr int R = kBloomR, AW = kTW + 2 * R, AH = kTH + 2 * R;
    extern __shared__ __align__(16) float smem_back[];
    float* thr = smem_back;                  // 256
    float* A = thr + 256;                    // BLOOM: 4 planes (mask, x0, x1, x2) of AH x AW
    float* B = A + 4 * AH * AW;              // BLOOM: the row pass of one plane, AH x TW
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const size_t npx = (size_t)a.H * a.W;
    const float* src = a.back + (size_t)f * npx * 3;
    uint8_t* fout = a.out + (size_t)f * npx * 3;
    for (int i = tid; i < 256; i += kBackT) thr[i] = a.thr[i];
    if constexpr (!BLOOM) {
        __syncthreads();
        for (int i = tid; i < kTH * kTW; i += kBackT) {
            const int y = i / kTW, x = i - y * kTW;
            const int gy = y0 + y, gx = x0 + x;
            if (gy >= a.H || gx >= a.W) continue;
            const size_t p = (size_t)gy * a.W + gx;
            float v[3] = {src[p], src[npx + p], src[2 * npx + p]};
            back_point(a, gy, v);
            uint8_t* q = fout + p * 3;
            q[0] = (uint8_t)quantize<float>(v[0], thr);
            q[1] = (uint8_t)quantize<float>(v[1], thr);
            q[2] = (uint8_t)quantize<float>(v[2], thr);
        }
    } else {
        // ---- the haloed tile: clipped frame and mask ----
        constexpr int N1 = (AH * AW + kBackT - 1) / kBackT;
        float raw[N1][3];  // a thread's loads of the haloed tile are all issued before the first is used
#pragma unroll
        for (int k = 0; k < N1; ++k) {
            const int i = tid + k * kBackT;
            const int ii = i < AH * AW ? i : 0;  // the idle lanes of the last round re-read sample 0
            const int ly = ii / AW, lx = ii - ly * AW;
            const int gy = reflect101(y0 - R + ly, a.H), gx = reflect101(x0 - R + lx, a.W);
            const size_t p = (size_t)gy * a.W + gx;
            raw[k][0] = src[p]; raw[k][1] = src[npx + p]; raw[k][2] = src[2 * npx + p];
        }
#pragma unroll
        for (int k = 0; k < N1; ++k) {
            const int i = tid + k * kBackT;
            if (i >= AH * AW) break;
            const int gy = reflect101(y0 - R + i / AW, a.H);
            float v[3] = {raw[k][0], raw[k][1], raw[k][2]};
            back_point(a, gy, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf(v[c], 0.0f), 1.0f);
            const float L = (0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2];
            A[i] = fminf(fmaxf((L - 0.4f) / 0.6f, 0.0f), 1.0f);
            A[AH * AW + i] = v[0]; A[2 * AH * AW + i] = v[1]; A[3 * AH * AW + i] = v[2];
        }
        __syncthreads();
        // one unit of the column pass per thread: rows ys..ys+3 of column x
        static_assert((kTH / 4) * kTW == kBackT, "one column unit per thread");
        const int ys = (tid / kTW) * 4, x = tid - (tid / kTW) * kTW;
        float blur[4][4];
#pragma unroll 1
        for (int pl = 0; pl < 4; ++pl) {
            const float* P = A + pl * AH * AW;
            for (int u = tid; u < AH * (kTW / 4); u += kBackT) {
                const int ly = u / (kTW / 4), xs = (u - ly * (kTW / 4)) * 4;
                const float* row = P + ly * AW + xs;
                float w[4 + 2 * R];
#pragma unroll
                for (int j = 0; j < 4 + 2 * R; ++j) w[j] = row[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s = w[i] * a.bloom[0];
#pragma unroll
                    for (int j = 1; j < kBloomK; ++j) s = fma_t(w[i + j], a.bloom[j], s);
                    B[ly * kTW + xs + i] = s;
                }
            }
            __syncthreads();
            {
                const float* col = B + ys * kTW + x;
                float w[4 + 2 * R];
#pragma unroll
                for (int j = 0; j < 4 + 2 * R; ++j) w[j] = col[j * kTW];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float s = w[i + R] * a.bloom[R];
#pragma unroll
                    for (int j = 1; j <= R; ++j) s = fma_t(w[i + R + j] + w[i + R - j], a.bloom[R + j], s);
                    blur[pl][i] = s;
                }
            }
            __syncthreads();  // B is rewritten by the next plane
        }
        // ---- screen blend gated by the blurred mask, clip, encode ----
        const int gx = x0 + x;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gy = y0 + ys + i;
            if (gy >= a.H || gx >= a.W) continue;
            const int ai = (ys + i + R) * AW + x + R;
            uint8_t* q = fout + ((size_t)gy * a.W + gx) * 3;
            const float gate = a.strength * blur[0][i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xv = A[(c + 1) * AH * AW + ai];
                const float screen = 1.0f - (1.0f - xv) * (1.0f - blur[c + 1][i]);
                const float y = xv + gate * (screen - xv);
                q[c] = (uint8_t)quantize<float>(y, thr);
            }
        }
    }
}

constexpr size_t back_lds(bool bloom) {
    return sizeof(float) * (256 + (bloom ? (size_t)4 * (kTH + 2 * kBloomR) * (kTW + 2 * kBloomR) + (size_t)(kTH + 2 * kBloomR) * kTW : 0));
}
static_assert(back_lds(true) <= 160 * 1024, "the bloom tile does not fit the 160 KiB LDS of a CU");

}  // namespace

extern "C" int avx_dichromat_night_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W, const avx_dichromat_desc* d,
                                      const avx_night_desc* nd, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, d != nullptr && d->struct_size == sizeof(avx_dichromat_desc), "avx_dichromat_night_u8: desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, nd != nullptr && nd->struct_size == sizeof(avx_night_desc), "avx_dichromat_night_u8: night desc is NULL or struct_size mismatch (ABI %d)",
                AVX_ABI_VERSION);
    AVX_REQUIRE(ctx, in_hwc && out_hwc, "avx_dichromat_night_u8: NULL frame pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && H > 0 && W > 0, "avx_dichromat_night_u8: bad shape n=%d H=%d W=%d", n_frames, H, W);
    AVX_REQUIRE(ctx, H >= kBloomK / 2 + 1 && W >= kBloomK / 2 + 1,
                "avx_dichromat_night_u8: frame %d x %d is smaller than 13 x 13 (one reflection must cover the 12-pixel bloom radius)", H, W);
    AVX_REQUIRE(ctx, (size_t)H * W < ((size_t)1 << 29), "avx_dichromat_night_u8: frame too large");
    AVX_REQUIRE(ctx, d->color_mode == AVX_COLOR_MATRIX || d->color_mode == AVX_COLOR_CAT_MERGE, "avx_dichromat_night_u8: unknown color_mode %d", d->color_mode);
    AVX_REQUIRE(ctx, d->post_mode >= AVX_POST_NONE && d->post_mode <= AVX_POST_STREAK, "avx_dichromat_night_u8: unknown post_mode %d", d->post_mode);
    AVX_REQUIRE(ctx, nd->chroma_scale >= 0.0 && nd->chroma_scale <= 1.0, "avx_dichromat_night_u8: chroma_scale %g outside [0, 1]", nd->chroma_scale);
    AVX_REQUIRE(ctx, nd->luminance_boost > 0.0 && nd->gamma > 0.0, "avx_dichromat_night_u8: luminance_boost %g and gamma %g must be positive",
                nd->luminance_boost, nd->gamma);
    AVX_REQUIRE(ctx, nd->bloom_strength >= 0.0 && nd->bloom_strength <= 1.0, "avx_dichromat_night_u8: bloom_strength %g outside [0, 1]", nd->bloom_strength);
    AVX_REQUIRE(ctx, nd->rod_ksize == kRodK && nd->rod_taps_host, "avx_dichromat_night_u8: rod_ksize %d: the rod blur has %d taps", nd->rod_ksize, kRodK);
    const bool bloom = nd->bloom_strength > 0.0;
    AVX_REQUIRE(ctx, !bloom || (nd->bloom_ksize == kBloomK && nd->bloom_taps_host), "avx_dichromat_night_u8: bloom_ksize %d: the bloom blur has %d taps",
                nd->bloom_ksize, kBloomK);
    const bool cat = d->color_mode == AVX_COLOR_CAT_MERGE;
    if (d->post_mode == AVX_POST_GAUSS) {
        AVX_REQUIRE(ctx, d->ksize >= 1 && d->ksize <= AVX_MAX_KSIZE && (d->ksize & 1), "avx_dichromat_night_u8: ksize %d must be odd, 1..%d", d->ksize, AVX_MAX_KSIZE);
        AVX_REQUIRE(ctx, d->taps_host != nullptr, "avx_dichromat_night_u8: taps_host is NULL");
    }
    if (d->post_mode == AVX_POST_STREAK)
        AVX_REQUIRE(ctx, !cat && d->streak_rows_host != nullptr && d->streak_stride >= 48, "avx_dichromat_night_u8: AVX_POST_STREAK needs AVX_COLOR_MATRIX and its row tables");
    if (d->post_mode == AVX_POST_ROWGAIN) AVX_REQUIRE(ctx, d->row_gain_host != nullptr, "avx_dichromat_night_u8: row_gain_host is NULL");
    if (n_frames == 0) return AVX_OK;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;

    NightArgs a{};
    a.H = H; a.W = W;
    a.tiles_x = (W + kTW - 1) / kTW; a.tiles_y = (H + kTH - 1) / kTH;
    a.in_f32 = d->in_f32 ? 1 : 0;
    a.cat = cat ? 1 : 0;
    if (!cat) {
        for (int i = 0; i < 9; ++i) a.M[i] = d->matrix[i];
    } else {  // animal_utils.py:56-63 (float32) and :70-76 (float64), as avx_dichromat_u8
        static const float kRgbToLms[9] = {0.31399022f, 0.63951294f, 0.04649755f, 0.15537241f, 0.75789446f, 0.08670142f, 0.01775239f, 0.10944209f, 0.87256922f};
        static const double kLmsToRgb[9] = {5.472213, -4.6419606, 0.16963711, -1.125242, 2.2931712, -0.16789523, 0.02980164, -0.19318072, 1.1636479};
        for (int i = 0; i < 9; ++i) { a.M[i] = kRgbToLms[i]; a.Bk[i] = kLmsToRgb[i]; }
        a.alpha = d->cat_alpha;
        a.one_minus_alpha = d->cat_beta;
    }
    a.keep_l = (float)(1.0 - nd->chroma_scale);  // NumPy: the Python float (1 - chroma_scale) meets a float32 array as float32
    a.keep_x = (float)nd->chroma_scale;
    a.boost = (float)nd->luminance_boost;
    a.gamma = (float)nd->gamma;
    for (int i = 0; i < kRodK; ++i) a.rod[i] = (float)nd->rod_taps_host[i];
    a.strength = (float)nd->bloom_strength;
    if (bloom)
        for (int i = 0; i < kBloomK; ++i) a.bloom[i] = (float)nd->bloom_taps_host[i];
    a.decode_lut = ctx->d_decode_lut;
    a.thr = ctx->d_enc_thr_f32;
    a.chroma_enable = d->chroma_enable;
    a.chroma_keep = d->chroma_keep;
    if (d->post_mode == AVX_POST_ROWGAIN) {
        const int rcu = avx_upload_row_table(ctx, ws, d->row_gain_host, sizeof(float) * (size_t)H, s);
        if (rcu) return rcu;
        a.row_gain = ws->d_row_gain;
        a.row_gain_on = 1;
        a.row_gain_clamp = d->row_gain_clamp;
    }

    // ---- groups of frames whose planes fit the scratch cap ----
    const bool planes_post = d->post_mode == AVX_POST_GAUSS || d->post_mode == AVX_POST_STREAK;
    const size_t npx = (size_t)H * W;
    const size_t frame_bytes = sizeof(float) * 3 * npx * (planes_post ? 2 : 1);
    size_t fit = kScratchCap / frame_bytes;
    int group = (int)(fit < 1 ? 1 : fit > AVX_EW_MAX_FRAMES ? AVX_EW_MAX_FRAMES : fit);
    if (const char* e = getenv("AVX_NIGHT_GROUP")) {  // tests: reach the walk at small sizes
        const int v = atoi(e);
        if (v >= 1) group = v < AVX_EW_MAX_FRAMES ? v : AVX_EW_MAX_FRAMES;
    }
    if (group > n_frames) group = n_frames;
    { const int rc = avx_ensure_scratch(ctx, ws, frame_bytes * (size_t)group); if (rc) return rc; }
    const size_t state_words = (size_t)AVX_EW_MAX_FRAMES * kFrameWords;
    if (!a.in_f32 && ws->flags_cap < state_words) {
        if (ws->d_flags) { AVX_HIP(ctx, hipStreamSynchronize(s)); AVX_HIP(ctx, hipFree(ws->d_flags)); }
        ws->d_flags = nullptr;
        ws->flags_cap = 0;
        AVX_HIP(ctx, hipMalloc((void**)&ws->d_flags, sizeof(uint32_t) * state_words));
        ws->flags_cap = state_words;
    }
    a.state = reinterpret_cast<unsigned long long*>(ws->d_flags);  // (hipMalloc: aligned)
    float* p0 = (float*)ws->d_scratch;
    float* p1 = p0 + (size_t)group * 3 * npx;
    a.front = p0;
    a.back = planes_post ? p1 : p0;
    auto kback = bloom ? k_night_back<true> : k_night_back<false>;
    const size_t lds = back_lds(bloom);
    AVX_HIP(ctx, hipFuncSetAttribute((const void*)kback, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const size_t in_frame = 3 * npx * (a.in_f32 ? sizeof(float) : 1);
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int n = n_frames - f0 < group ? n_frames - f0 : group;
        a.in = in_hwc + (size_t)f0 * in_frame;
        a.out = out_hwc + (size_t)f0 * 3 * npx;
        if (!a.in_f32) AVX_HIP(ctx, hipMemsetAsync(a.state, 0, sizeof(uint32_t) * kFrameWords * (size_t)n, s));
        if (a.in_f32) hipLaunchKernelGGL(k_night_front<true>, dim3(tiles, n), dim3(kFrontT), 0, s, a);
        else hipLaunchKernelGGL(k_night_front<false>, dim3(tiles, n), dim3(kFrontT), 0, s, a);
        AVX_HIP(ctx, hipGetLastError());
        if (d->post_mode == AVX_POST_GAUSS) {
            const int rc = avx_planes_gaussian_blur_batch(ctx, p0, 3 * npx, p1, 3 * npx, n, 3, H, W, d->ksize, d->taps_host, 0, stream);
            if (rc) return rc;
        } else if (d->post_mode == AVX_POST_STREAK) {
            for (int f = 0; f < n; ++f) {
                const int rc = avx_streak_planes_f32(ctx, p0 + (size_t)f * 3 * npx, p1 + (size_t)f * 3 * npx, H, W, d->streak_rows_host, d->streak_stride, stream);
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL(kback, dim3(tiles, n), dim3(kBackT), lds, s, a);
        AVX_HIP(ctx, hipGetLastError());
    }
    return AVX_OK;
}
