// csrc/itp.hip -- dE_ITP of ITU-R BT.2124 on the device (the definition is include/avx.h's): per pixel of two batches,
// each either an HDR payload as stored (one of the four 10-bit formats, BT.2020 Y'CbCr, PQ or HLG) or uint8 sRGB frames shown at
// sdr_white nits, 720 x the distance in ICtCp with Ct halved -- as a float32 plane, as a picture and as a record per frame, which
// are avx_delta_e_u8's in every respect but the value and the source of the A and B panels.
//
// k_itp: grid (chunks, frames), one kernel for every mix of sides.  A workgroup owns kChunk = 4096 consecutive pixels of a frame pair,
// thread t takes pixels t, t + 256, ... of it, as in delta_e_walk.h: the float64 sum of a frame is formed in the order of the other
// colour difference kernels, a function of H and W alone.  What a side contributes to the chunk in contiguous bytes -- 12288 bytes of
// RGB, or 8192 bytes of luma -- goes into LDS first, in 16-byte, 8-byte or sample-sized loads, whichever the address and the length
// of the run admit; the choice moves bytes only.  The chroma samples of an HDR pixel are read where they lie (two 2-byte loads that
// neighbouring lanes share), and its chroma terms are formed per pixel: a chunk is a run of pixels, not of chroma blocks, and the
// six operations are nothing beside the 24 transcendentals a PQ pixel costs (12 for the EOTF, 12 for the three inverse curves).  The
// kind, the format and the transfer of a side are kernel arguments, uniform over the launch: the branches on them are scalar.
// A pixel whose samples are equal on two sides of one kind, range and transfer is 0 by definition and skips the arithmetic; the
// branch is taken by a wave whose 64 pixels are all equal.
// The map's bytes go back through LDS; the A and B panels of the side layout are copied from the callers' panel frames.  A thread's
// tally, the workgroup's share of the record, the map's quantiser and colour, the rows of the side layout and the host side's common
// checks and launch frame are delta_e_common.h's; HLG's inverse OETF, pw and the constants of the curves are yuv_hdr_px.h's.
#include "delta_e_common.h"
#include "yuv_hdr_px.h"

namespace {

constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // pixels of a workgroup, as delta_e_walk.h's

struct ItpSide {
    const uint8_t* data;   // HDR: payloads as stored; SDR: H x W x 3 frames
    const uint8_t* panel;  // H x W x 3 frames for the map (SDR: data); NULL without a map
    int hdr, tr;           // HDR: the transfer
    int sx, sy, il, sh;    // HDR: the format's traits (yuv_formats.h)
    int yo, cw;            // HDR: the luma offset; chroma blocks in a row
    float ys, cs;          // HDR: the scales of luma and chroma
    size_t ysz, csz, fsz;  // luma samples, chroma blocks, bytes of a frame
};

struct ItpC {
    float rv, gu, gv, bu, hlg_c;  // HdrC's
    float ksdr;                   // sdr_white / 10000
    float g0[3], g2[3];           // BT.709 -> BT.2020, columns 0 and 2 of rows R, G, B
};

struct ItpArgs {
    ItpSide a, b;
    ItpC c;
    int same;  // equal samples mean equal pixels
    DeOut o;   // partials: [frame][chunk]
};

// BT.2100 LMS over 4096 in the form anchored on green (every row sums to 4096), and ICtCp scaled by 720 with Ct halved, formed
// from L' - M' and S' - M': 6610 + 7003 = 13613, 17933 - 543 = 17390
constexpr float kL0 = 1688.0f / 4096.0f, kL2 = 262.0f / 4096.0f, kM0 = 683.0f / 4096.0f, kM2 = 462.0f / 4096.0f, kS0 = 99.0f / 4096.0f, kS2 = 3688.0f / 4096.0f;
constexpr float kT0 = (float)(360.0 * 6610.0 / 4096.0), kT2 = (float)(360.0 * 7003.0 / 4096.0);
constexpr float kP0 = (float)(720.0 * 17933.0 / 4096.0), kP2 = (float)(-720.0 * 543.0 / 4096.0);
constexpr float kPqM1f = (float)kPqM1, kPqW = (float)(1.0 - 3424.0 / 4096.0);
constexpr float kPqE = (float)(-2.0 * kPqM2 * 1.4426950408889634);  // -2 m2 log2(e)
constexpr float kA3 = (float)(1.0 / 3.0), kA5 = 0.2f, kA7 = (float)(1.0 / 7.0), kA9 = (float)(1.0 / 9.0);

// The PQ EOTF, E' in [0, 1] -> x = nits / 10000.  With p = E'^(1/m2) in [c1, 1], yuv_hdr_px.h's form c2 - c3 p cancels to 0.164 near the
// top and costs 6e-5 of x there, which is nothing in an 8-bit code and 0.005 dE_ITP here.  u = 1 - p = -expm1(t), t = ln(E') / m2 in
// [-0.09, 0] for every code above 0, by its series to t^6 (the next term is below 2^-28 of the sum); then p - c1 = (1 - c1) - u and
// c2 - c3 p = (1 - c1) + c3 u are formed without cancellation: two log2, one exp2 and one rcp.
constexpr float kPqT = (float)(1.0 / (kPqM2 * 1.4426950408889634));  // ln 2 / m2
__device__ __forceinline__ float pq_eotf_u(float e) {
    const float t = __builtin_amdgcn_logf(e > 0.0f ? e : 1.0f) * kPqT;
    float h = 1.0f + t * (float)(1.0 / 6.0);
    h = 1.0f + (t * 0.2f) * h;
    h = 1.0f + (t * 0.25f) * h;
    h = 1.0f + (t * (float)(1.0 / 3.0)) * h;
    h = 1.0f + (t * 0.5f) * h;
    const float u = -(t * h);
    const float num = kPqW - u, den = kPqW + kPqC3 * u;
    const float x = pw((num > 0.0f ? num : 0.0f) * __builtin_amdgcn_rcpf(den), kPqInvM1);
    return e > 0.0f ? x : 0.0f;
}

// The PQ inverse EOTF, x = nits / 10000 -> E'.  q = (c1 + c2 p) / (1 + c3 p) with p = x^m1 lies in [c1, 1] and is raised to m2 = 78.84,
// which multiplies the rounding of log2(q) by as much.  c1 = c3 - c2 + 1 gives 1 - q = (1 - c1) (1 - p) / (1 + c3 p) =: w without
// cancellation, and ln q = ln(1 - w) = -2 atanh(s), s = w / (2 - w) <= 0.09, by its odd series to s^9 (the next term is below 2^-30
// of the sum): one log2, two exp2 and one rcp.
__device__ __forceinline__ float pq_inv(float x) {
    const float p = pw(x, kPqM1f);
    const float n = kPqW * (1.0f - p), d = 1.0f + kPqC3 * p;
    const float s = n * __builtin_amdgcn_rcpf((d + d) - n);
    const float z = s * s;
    const float poly = 1.0f + z * (kA3 + z * (kA5 + z * (kA7 + z * kA9)));
    return __builtin_amdgcn_exp2f(kPqE * (s * poly));
}

// r, g, b: BT.2020 display light over 10000 nits -> (720 I, 360 Ct, 720 Cp); r = g = b gives L = M = S = g and T = P = 0 exactly
__device__ __forceinline__ void itp_of(float r, float g, float b, float& I, float& T, float& P) {
    const float dr = r - g, db = b - g;
    const float l = pq_inv((g + kL0 * dr) + kL2 * db);
    const float m = pq_inv((g + kM0 * dr) + kM2 * db);
    const float s = pq_inv((g + kS0 * dr) + kS2 * db);
    const float lm = l - m, sm = s - m;
    I = 360.0f * (l + m);
    T = kT0 * lm + kT2 * sm;
    P = kP0 * lm + kP2 * sm;
}

// the samples of pixel i of the chunk (frame pixel idx at row y, column x): (r8, g8, b8) or (Y, U, V), the latter as
// avx_yuv_hdr_to_rgb_u8 reads them: the chroma block's samples for every pixel of the block
__device__ __forceinline__ void side_samples(const ItpSide& S, const uint8_t* lds, const uint8_t* fr, int i, int y, int x, int& s0, int& s1, int& s2) {
    if (!S.hdr) {
        s0 = lds[3 * i], s1 = lds[3 * i + 1], s2 = lds[3 * i + 2];
        return;
    }
    const uint16_t* smp = (const uint16_t*)fr;
    const size_t r = (size_t)(y >> S.sy) * S.cw + (x >> S.sx);  // below csz
    s0 = (int)(((const uint16_t*)lds)[i] >> S.sh);
    s1 = (int)(smp[S.il ? S.ysz + 2 * r : S.ysz + r] >> S.sh);
    s2 = (int)(smp[S.il ? S.ysz + 2 * r + 1 : S.ysz + S.csz + r] >> S.sh);
}

__device__ __forceinline__ void side_itp(const ItpSide& S, const ItpC& c, const float* lut, int s0, int s1, int s2, float& I, float& T, float& P) {
    float r, g, b;
    if (!S.hdr) {
        const float lr = c.ksdr * lut[s0], lg = c.ksdr * lut[s1], lb = c.ksdr * lut[s2];
        const float dr = lr - lg, db = lb - lg;
        r = (lg + c.g0[0] * dr) + c.g2[0] * db;
        g = (lg + c.g0[1] * dr) + c.g2[1] * db;
        b = (lg + c.g0[2] * dr) + c.g2[2] * db;
    } else {
        const float yv = (float)(s0 - S.yo) * S.ys, cb = (float)(s1 - 512) * S.cs, cr = (float)(s2 - 512) * S.cs;
        const float er = clamp01(yv + c.rv * cr), eg = clamp01(yv + (c.gu * cb + c.gv * cr)), eb = clamp01(yv + c.bu * cb);
        if (S.tr == AVX_TRANSFER_PQ) {
            r = pq_eotf_u(er), g = pq_eotf_u(eg), b = pq_eotf_u(eb);
        } else {
            const float sr = hlg_inv_oetf(er, c.hlg_c), sg = hlg_inv_oetf(eg, c.hlg_c), sb = hlg_inv_oetf(eb, c.hlg_c);
            const float f = 0.1f * pw((kLumR * sr + kLumG * sg) + kLumB * sb, kHlgGammaM1);  // 1000 nits over 10000; 0 at Ys = 0
            r = f * sr, g = f * sg, b = f * sb;
        }
    }
    itp_of(r, g, b, I, T, P);
}

// n bytes, global -> LDS (16-byte aligned), in the widest loads that the address and n admit; unit: the size of a sample
__device__ __forceinline__ void stage_run(uint8_t* dst, const uint8_t* src, int n, int unit) {
    const uintptr_t al = (uintptr_t)src | (uintptr_t)n;
    if ((al & 15) == 0) {
        for (int j = threadIdx.x; j < n / 16; j += kThreads) reinterpret_cast<uint4*>(dst)[j] = reinterpret_cast<const uint4*>(src)[j];
    } else if ((al & 7) == 0) {
        for (int j = threadIdx.x; j < n / 8; j += kThreads) reinterpret_cast<uint2*>(dst)[j] = reinterpret_cast<const uint2*>(src)[j];
    } else if (unit == 2) {
        for (int j = threadIdx.x; j < n / 2; j += kThreads) reinterpret_cast<uint16_t*>(dst)[j] = reinterpret_cast<const uint16_t*>(src)[j];
    } else {
        for (int j = threadIdx.x; j < n; j += kThreads) dst[j] = src[j];
    }
}

// n bytes, LDS (16-byte aligned) -> global
__device__ __forceinline__ void unstage_run(uint8_t* dst, const uint8_t* src, int n) {
    const uintptr_t al = (uintptr_t)dst | (uintptr_t)n;
    if ((al & 15) == 0) {
        for (int j = threadIdx.x; j < n / 16; j += kThreads) reinterpret_cast<uint4*>(dst)[j] = reinterpret_cast<const uint4*>(src)[j];
    } else if ((al & 7) == 0) {
        for (int j = threadIdx.x; j < n / 8; j += kThreads) reinterpret_cast<uint2*>(dst)[j] = reinterpret_cast<const uint2*>(src)[j];
    } else {
        for (int j = threadIdx.x; j < n; j += kThreads) dst[j] = src[j];
    }
}

__global__ __launch_bounds__(kThreads) void k_itp(ItpArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t sa[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t sb[kChunk * 3];
    __shared__ __attribute__((aligned(16))) uint8_t so[kChunk * 3];
    __shared__ float lut[256];
    __shared__ DeRecLds lds;
    const DeOut& o = p.o;
    const int tid = threadIdx.x, f = blockIdx.y;
    const size_t npx = (size_t)o.H * o.W;  // below 2^32
    const size_t base = (size_t)blockIdx.x * kChunk;
    const int valid = (int)min((size_t)kChunk, npx - base);  // pixels of this chunk
    const uint8_t* fa = p.a.data + (size_t)f * p.a.fsz;
    const uint8_t* fb = p.b.data + (size_t)f * p.b.fsz;
    lut[tid] = __uint_as_float(kLabDecodeBits[tid]);
    lds.hist[tid] = 0;
    if (p.a.hdr) stage_run(sa, fa + base * 2, valid * 2, 2);
    else stage_run(sa, fa + base * 3, valid * 3, 1);
    if (p.b.hdr) stage_run(sb, fb + base * 2, valid * 2, 2);
    else stage_run(sb, fb + base * 3, valid * 3, 1);
    __syncthreads();

    const float G = o.gain, T = o.threshold;
    const bool any_hdr = p.a.hdr || p.b.hdr;
    const uint8_t* pa = o.out ? p.a.panel + ((size_t)f * npx + base) * 3 : nullptr;  // the chunk's pixels of A's panel
    DeTally tally;
    float* de_out = o.de ? o.de + (size_t)f * npx + base : nullptr;
#pragma unroll 1
    for (int i = tid; i < valid; i += kThreads) {
        int y = 0, x = 0;
        if (any_hdr) {
            const uint32_t idx = (uint32_t)(base + i);
            y = (int)(idx / (uint32_t)o.W), x = (int)(idx - (uint32_t)y * (uint32_t)o.W);
        }
        int a0, a1, a2, b0, b1, b2;
        side_samples(p.a, sa, fa, i, y, x, a0, a1, a2);
        side_samples(p.b, sb, fb, i, y, x, b0, b1, b2);
        float de = 0.0f;  // equal samples on sides read alike: 0 by definition
        if (!p.same || a0 != b0 || a1 != b1 || a2 != b2) {
            float ia, ta, qa, ib, tb, qb;
            side_itp(p.a, p.c, lut, a0, a1, a2, ia, ta, qa);
            side_itp(p.b, p.c, lut, b0, b1, b2, ib, tb, qb);
            const float di = ia - ib, dt = ta - tb, dp = qa - qb;
            de = (dt == 0.0f && dp == 0.0f) ? fabsf(di) : fsqrt((di * di + dt * dt) + dp * dp);
        }
        tally.add(de, (uint32_t)(base + i), T, lds.hist);
        if (de_out) de_out[i] = de;
        if (o.out) {
            uint32_t r, g, b;
            de_map_colour(de, G, T, o.mode, pa[3 * i], pa[3 * i + 1], pa[3 * i + 2], r, g, b);
            so[3 * i] = (uint8_t)r, so[3 * i + 1] = (uint8_t)g, so[3 * i + 2] = (uint8_t)b;
        }
    }
    __syncthreads();

    // ---- the panels out ----
    if (o.out && !o.side) {
        unstage_run(o.out + ((size_t)f * npx + base) * 3, so, valid * 3);
    } else if (o.out) {
        uint8_t* fo = o.out + (size_t)f * npx * 9;
        const uint8_t* pb = p.b.panel + ((size_t)f * npx + base) * 3;
        const size_t row = (size_t)o.W * 3;  // bytes of a panel's row
        const bool vec = o.W % 16 == 0 && (((uintptr_t)o.out | (uintptr_t)p.a.panel | (uintptr_t)p.b.panel) & 15) == 0;
        if (vec) de_side_rows_out<true>(fo, row, base, valid, pa, pb, so);
        else de_side_rows_out<false>(fo, row, base, valid, pa, pb, so);
    }

    // ---- the record ----
    de_record_share(tally, lds, o.partials + ((size_t)f * gridDim.x + blockIdx.x), o.rec + f);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
const char* const kFn = "avx_itp_delta";

int side_check(avx_ctx* ctx, const char* which, const avx_itp_side* s, int n_frames, int H, int W, bool with_map) {
    AVX_REQUIRE(ctx, s && s->struct_size == sizeof(avx_itp_side), "%s: side %s is NULL or of the wrong struct_size", kFn, which);
    AVX_REQUIRE(ctx, s->kind == AVX_ITP_SDR || s->kind == AVX_ITP_HDR, "%s: side %s: kind %d (0 sdr, 1 hdr)", kFn, which, s->kind);
    AVX_REQUIRE(ctx, s->data, "%s: side %s: NULL buffer", kFn, which);
    if (s->kind == AVX_ITP_HDR) {
        AVX_REQUIRE(ctx, fmt_ok(s->pix_fmt) && kTraits[s->pix_fmt].depth == 10,
                    "%s: side %s: pixel format %d (the 10-bit formats of enum avx_pix_fmt: %d yuv420p10le, %d yuv422p10le, %d yuv444p10le, %d p010le)", kFn,
                    which, s->pix_fmt, AVX_PIX_YUV420P10LE, AVX_PIX_YUV422P10LE, AVX_PIX_YUV444P10LE, AVX_PIX_P010LE);
        AVX_REQUIRE(ctx, H <= (1 << 15) && W <= (1 << 15), "%s: side %s: bad shape (%d frames of %d x %d)", kFn, which, n_frames, H, W);
        AVX_REQUIRE(ctx, s->full_range == 0 || s->full_range == 1, "%s: side %s: full_range %d (0 limited, 1 full)", kFn, which, s->full_range);
        AVX_REQUIRE(ctx, s->transfer == AVX_TRANSFER_PQ || s->transfer == AVX_TRANSFER_HLG, "%s: side %s: transfer %d (1 pq, 2 hlg)", kFn, which, s->transfer);
        AVX_REQUIRE(ctx, ((uintptr_t)s->data & 1) == 0, "%s: side %s: 16-bit samples need a 2-byte aligned payload", kFn, which);
        AVX_REQUIRE(ctx, !with_map || s->panel, "%s: side %s: a map needs the panel frames of an HDR side", kFn, which);
    }
    return AVX_OK;
}

ItpSide side_args(const avx_itp_side* s, int H, int W) {
    ItpSide o = {};
    o.data = s->data;
    o.hdr = s->kind == AVX_ITP_HDR;
    if (!o.hdr) {
        o.panel = s->data;
        o.fsz = (size_t)H * W * 3;
        return o;
    }
    const Traits& t = kTraits[s->pix_fmt];
    const HdrC c = hdr_constants(s->full_range, s->transfer, AVX_TONEMAP_CLIP, 1000.0, 203.0);  // the ranges' scales; the rest is not read
    o.panel = s->panel;
    o.tr = s->transfer;
    o.sx = t.sx, o.sy = t.sy, o.il = t.il, o.sh = s->pix_fmt == AVX_PIX_P010LE ? 6 : 0;
    o.yo = c.yo, o.ys = c.ys, o.cs = c.cs;
    o.cw = (W + (1 << t.sx) - 1) >> t.sx;
    o.ysz = (size_t)H * W, o.csz = chroma_blocks(t, H, W), o.fsz = frame_size(t, H, W);
    return o;
}

}  // namespace

extern "C" int avx_itp_delta(avx_ctx* ctx, const avx_itp_side* a, const avx_itp_side* b, double sdr_white, int n_frames, int H, int W, int mode, float gain,
                             float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    if (const int rc = de_check_options(ctx, kFn, n_frames, H, W, mode, gain, threshold, layout, rec_dev, de_out)) return rc;
    if (const int rc = side_check(ctx, "A", a, n_frames, H, W, map_out != nullptr)) return rc;
    if (const int rc = side_check(ctx, "B", b, n_frames, H, W, map_out != nullptr)) return rc;
    AVX_REQUIRE(ctx, std::isfinite(sdr_white) && sdr_white > 0.0, "%s: sdr_white %g must be finite and positive", kFn, sdr_white);

    ItpArgs p = {};
    p.a = side_args(a, H, W), p.b = side_args(b, H, W);
    const size_t npx = (size_t)H * W, rgb_bytes = (size_t)n_frames * npx * 3, map_bytes = rgb_bytes * (layout == AVX_DELTA_E_SIDE ? 3 : 1);
    if (map_out) {
        for (const ItpSide* s : {&p.a, &p.b})
            AVX_REQUIRE(ctx, !overlaps(map_out, map_bytes, s->data, (size_t)n_frames * s->fsz) && !overlaps(map_out, map_bytes, s->panel, rgb_bytes),
                        "%s: map_out overlaps an input (data %p, panel %p, map %p)", kFn, (const void*)s->data, (const void*)s->panel, (const void*)map_out);
    }

    const HdrC hc = hdr_constants(0, AVX_TRANSFER_PQ, AVX_TONEMAP_CLIP, 1000.0, 203.0);  // the BT.2020 matrix terms and HLG's c
    p.c.rv = hc.rv, p.c.gu = hc.gu, p.c.gv = hc.gv, p.c.bu = hc.bu, p.c.hlg_c = hc.hlg_c;
    p.c.ksdr = (float)(sdr_white / 10000.0);
    double m[3][3], mi[3][3];
    gamut_2020_to_709(m);
    inv3(m, mi);  // BT.709 -> BT.2020: every row sums to 1
    for (int i = 0; i < 3; ++i) p.c.g0[i] = (float)mi[i][0], p.c.g2[i] = (float)mi[i][2];
    p.same = p.a.hdr == p.b.hdr && (!p.a.hdr || (a->full_range == b->full_range && a->transfer == b->transfer));

    const size_t nchunks = (npx + kChunk - 1) / kChunk;  // below 2^20
    hipStream_t s;
    avx_ws* ws;
    if (const int rc = de_begin(ctx, stream, sizeof(double) * nchunks * (size_t)n_frames, rec_dev, n_frames, &s, &ws)) return rc;
    p.o = {map_out, de_out, (double*)ws->d_scratch, rec_dev, H, W, mode, layout == AVX_DELTA_E_SIDE, gain, threshold};
    hipLaunchKernelGGL(k_itp, dim3((unsigned)nchunks, n_frames), dim3(kThreads), 0, s, p);
    return de_finish(ctx, s, p.o.partials, nchunks, W, rec_dev, n_frames);
}
