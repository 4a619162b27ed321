// Probe for the 2:4-sparse form of the depthwise 3x3 units of MST++ (round 6): v_smfmac_f32_16x16x64_f16 against v_mfma_f32_16x16x32_f16.
//   (a) operand layout by one-hot inputs: A = one 1.0 at (lane La, element e) with the 2-bit index t in that element's field, B = a distinct
//       integer code per (lane, element).  D then SHOWS which row the A element feeds and, per column, which B element it was paired with:
//       the pairing A(q = La / 16, e, t) <-> B(q, j) is all a host pack needs (K itself is only a summation label).  Run for the index bits
//       in the low and the high half of the index register and several cbsz / abid, to see which field the instruction reads.
//   (b) ns per unit (8 channels x 2 rows x 16 px = 256 outputs) and SIMD at 4 waves per SIMD for four unit forms
//         3 x dense 16x16x32 | 1 x sparse 16x16x64 + 1 x dense | 2 x sparse | 1 x dense + 1 x sparse (the dense one takes C = 0 as an inline constant)
//       each alone (operands in registers), with the unit's three ds_read_b128, beside the prescaled GELU of phase 2a (gelu_mx<2>, pack, 8-byte
//       LDS store) and the GELU alone.
// Whole-kernel HIP-event timing, workgroups pinned to 4 waves per SIMD by their LDS size (as dw_block_probe.hip).
// hipcc -O3 --offload-arch=gfx950 -I../../animal-vision_amd/csrc smfmac_dw_probe.hip -o smfmac_dw_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "mst_common.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16 __attribute__((ext_vector_type(16)));

#define CK(x)                                                                                  \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } \
    } while (0)

// ---- (a) layout ----------------------------------------------------------------------------------------------------------------------
template <int CBSZ, int ABID>
__global__ __launch_bounds__(64) void k_layout(const h8* __restrict__ A, const unsigned* __restrict__ IDX, const h16* __restrict__ B, float* __restrict__ D) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    const f4 d = __builtin_amdgcn_smfmac_f32_16x16x64_f16(A[i], B[threadIdx.x], z, (int)IDX[i], CBSZ, ABID);
    *reinterpret_cast<f4*>(D + i * 4) = d;
}

constexpr int NCFG = 64 * 8 * 4;  // (La, e, t)

// one experiment: index bits at `shift` of the index register; prints how many of the NCFG one-hot runs follow the expected pairing and the pairing table of lanes 0 / 16 / 32 / 48
template <int CBSZ, int ABID>
static int layout_run(int shift, h8* dA, unsigned* dI, h16* dB, float* dD, bool table) {
    std::vector<_Float16> hA((size_t)NCFG * 64 * 8, (_Float16)0.f);
    std::vector<unsigned> hI((size_t)NCFG * 64, 0u);
    for (int cfg = 0; cfg < NCFG; ++cfg) {
        const int La = cfg / 32, e = (cfg / 4) % 8, t = cfg % 4;
        hA[((size_t)cfg * 64 + La) * 8 + e] = (_Float16)1.f;
        hI[(size_t)cfg * 64 + La] = (unsigned)t << (2 * e + shift);
    }
    CK(hipMemcpy(dA, hA.data(), hA.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dI, hI.data(), hI.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_layout<CBSZ, ABID>), dim3(NCFG), dim3(64), 0, 0, dA, dI, dB, dD);
    CK(hipDeviceSynchronize());
    std::vector<float> hD((size_t)NCFG * 256);
    CK(hipMemcpy(hD.data(), dD, hD.size() * 4, hipMemcpyDeviceToHost));
    int one_row = 0, row_ok = 0, col_ok = 0, pair_ok = 0;
    std::vector<int> pq(NCFG, -1), pj(NCFG, -1);
    for (int cfg = 0; cfg < NCFG; ++cfg) {
        const int La = cfg / 32, e = (cfg / 4) % 8, t = cfg % 4;
        const float* d = hD.data() + (size_t)cfg * 256;
        int nz = 0, m = -1;
        bool same_row = true, cols = true, same_b = true;
        int bq0 = -1, bj0 = -1;
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 4; ++r) {
                const float v = d[l * 4 + r];
                if (v == 0.f) continue;
                ++nz;
                const int mm = 4 * (l / 16) + r;  // the dense 16x16 result layout: lane l, register r = row 4 (l / 16) + r, column l % 16
                if (m < 0) m = mm;
                same_row &= mm == m;
                const int code = (int)v - 1, L = code / 16, j = code % 16;
                cols &= L % 16 == l % 16;
                if (bq0 < 0) { bq0 = L / 16; bj0 = j; }
                same_b &= L / 16 == bq0 && j == bj0;
            }
        if (nz == 16 && same_row) ++one_row;
        if (nz == 16 && same_row && m == La % 16) ++row_ok;
        if (nz == 16 && cols && same_b) { ++col_ok; pq[cfg] = bq0; pj[cfg] = bj0; }
        if (nz == 16 && cols && same_b && bq0 == La / 16 && bj0 == 4 * (e / 2) + t) ++pair_ok;
    }
    printf("cbsz %d abid %d, index field at bit %2d + 2 e:  one result row %4d / %d   row = La %% 16 %4d   column = B lane %% 16, one (q, j) %4d   B(q, j) = (La / 16, 4 (e / 2) + t) %4d\n",
           CBSZ, ABID, shift, one_row, NCFG, row_ok, col_ok, pair_ok);
    if (table)
        for (int La = 0; La < 64; La += 16) {
            printf("  A lane %2d:", La);
            for (int e = 0; e < 8; ++e) {
                printf("  e%d", e);
                for (int t = 0; t < 4; ++t) { const int cfg = (La * 8 + e) * 4 + t; printf(" %d.%-2d", pq[cfg], pj[cfg]); }
            }
            printf("   (B q.j per t = 0 .. 3)\n");
        }
    return 0;
}

// ---- (b) cost ------------------------------------------------------------------------------------------------------------------------
// UNIT 0: 3 dense, 1: sparse + dense, 2: 2 sparse, 3: dense + sparse, 9: none.  MODE 0: operands in registers, 1: + 3 ds_read_b128, 2: + gelu_mx<2> + pack + ds_write_b64, 3: GELU + store only
template <int UNIT, int MODE>
__global__ __launch_bounds__(256) void k_cost(float* out, int iters, float seed) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 32 * 1024 / 4; i += 256) reinterpret_cast<unsigned*>(lds)[i] = 0x2c002c00u + (i & 0xff);
    __syncthreads();
    const unsigned char* base = lds + (lane & 15) * 144 + (lane >> 4) * 2816;  // halo row q = lane / 16, pixel lane % 16: the kernels' lane-constant address
    unsigned char* wb = lds + 33 * 1024 + threadIdx.x * 8;
    h8 ad[3], as[2];
    int ix[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ad[i][j] = (_Float16)(j == (lane & 7) ? seed * 0.01f * (i + 1) : 0.f);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) as[i][j] = (_Float16)((j & 1) == 0 ? seed * 0.01f * (i + 1) : 0.f);
        ix[i] = (int)(0x44444444u + (unsigned)(lane & 3) * 0x11111111u * (unsigned)(seed > 0.f));
    }
    uint4 bq[3] = {uint4{0x2c002c00u, 0x2c012c00u, 0x2c022c00u, 0x2c032c00u}, uint4{0x2c042c00u, 0x2c052c00u, 0x2c062c00u, 0x2c072c00u}, uint4{0x2c082c00u, 0x2c092c00u, 0x2c0a2c00u, 0x2c0b2c00u}};
    float sum = 0.f;
    for (int it = 0; it < iters; ++it) {
        const unsigned char* b = base + (it & 7) * 2816;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        if (MODE == 1 || MODE == 2) {
#pragma unroll
            for (int i = 0; i < 3; ++i) bq[i] = *reinterpret_cast<const uint4*>(b + i * 144);
        } else if (MODE == 0) {
            asm volatile("" : "+v"(bq[0].x), "+v"(bq[1].x), "+v"(bq[2].x));  // opaque: nothing is hoisted out of the loop
        }
        if (MODE != 3) {
            const h8 b0 = __builtin_bit_cast(h8, bq[0]), b1 = __builtin_bit_cast(h8, bq[1]), b2 = __builtin_bit_cast(h8, bq[2]);
            if (UNIT == 0) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ad[0], b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ad[1], b1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ad[2], b2, acc, 0, 0, 0);
            } else if (UNIT == 1) {
                const h16 b01 = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(as[0], b01, acc, ix[0], 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ad[2], b2, acc, 0, 0, 0);
            } else if (UNIT == 3) {  // dense first: its C operand is the inline constant 0, while the sparse instruction accumulates in place (a zeroed accumulator costs 4 vector moves)
                const h16 b01 = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ad[2], b2, acc, 0, 0, 0);
                acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(as[0], b01, acc, ix[0], 0, 0);
            } else if (UNIT == 2) {
                const h16 b01 = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
                const h16 b2z = __builtin_shufflevector(b2, b2, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);  // the fourth K-octet of the pair is padding
                acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(as[0], b01, acc, ix[0], 0, 0);
                acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(as[1], b2z, acc, ix[1], 0, 0);
            }
        } else {
            acc = f4{(float)it * 1e-4f, sum, 0.25f, -0.5f};
        }
        if (MODE >= 2) {
            float2_t gp[2] = {float2_t{acc[0], acc[1]}, float2_t{acc[2], acc[3]}};
            gelu_mx<2>(gp);
            *reinterpret_cast<uint2*>(wb) = uint2{pack_f16(gp[0].x, gp[0].y), pack_f16(gp[1].x, gp[1].y)};
            if (MODE == 3) sum += gp[0].x;
        } else {
            sum += acc[0] + acc[1] + acc[2] + acc[3];
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = sum + (float)lds[33 * 1024 + threadIdx.x];
}

template <typename K>
static double cost_run(K kern, float* d) {
    const int w = 4, blocks = 256 * w, iters = 20000, lds = 36 * 1024;
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    double best = 1e30;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, 0, d, 200, 1.0f);
    for (int rep = 0; rep < 3; ++rep) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, 0, d, iters, 1.0f);
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double ns = ms * 1e6 / ((double)w * iters);
        best = ns < best ? ns : best;
    }
    return best;  // ns per unit per SIMD (a SIMD runs w waves, each `iters` units)
}

int main() {
    h8* dA; unsigned* dI; h16* dB; float* dD;
    CK(hipMalloc(&dA, (size_t)NCFG * 64 * 16)); CK(hipMalloc(&dI, (size_t)NCFG * 64 * 4)); CK(hipMalloc(&dB, 64 * 32)); CK(hipMalloc(&dD, (size_t)NCFG * 256 * 4));
    std::vector<_Float16> hB(64 * 16);
    for (int L = 0; L < 64; ++L)
        for (int j = 0; j < 16; ++j) hB[L * 16 + j] = (_Float16)(float)(1 + L * 16 + j);  // <= 1024: exact
    CK(hipMemcpy(dB, hB.data(), hB.size() * 2, hipMemcpyHostToDevice));
    printf("(a) v_smfmac_f32_16x16x64_f16 layout: %d one-hot runs per line, A = 1.0 at (lane La, element e), index t in its 2-bit field\n", NCFG);
    if (layout_run<0, 0>(0, dA, dI, dB, dD, true)) return 1;
    if (layout_run<0, 0>(16, dA, dI, dB, dD, false)) return 1;
    if (layout_run<0, 1>(0, dA, dI, dB, dD, false)) return 1;
    if (layout_run<0, 1>(16, dA, dI, dB, dD, true)) return 1;
    if (layout_run<0, 2>(0, dA, dI, dB, dD, false)) return 1;
    if (layout_run<0, 3>(16, dA, dI, dB, dD, false)) return 1;
    if (layout_run<1, 0>(0, dA, dI, dB, dD, false)) return 1;
    if (layout_run<1, 1>(16, dA, dI, dB, dD, false)) return 1;
    if (layout_run<1, 1>(0, dA, dI, dB, dD, false)) return 1;

    float* d;
    CK(hipMalloc(&d, 256 * 8 * 256 * 4));
    printf("(b) ns per unit (8 channels x 2 rows x 16 px) per SIMD, 4 waves per SIMD\n");
    printf("%-34s %8s %8s %8s %8s\n", "", "3 dense", "1 sp+1 d", "2 sparse", "1 d+1 sp");
    printf("%-34s %8.2f %8.2f %8.2f %8.2f\n", "MFMAs alone (registers)", cost_run(k_cost<0, 0>, d), cost_run(k_cost<1, 0>, d), cost_run(k_cost<2, 0>, d), cost_run(k_cost<3, 0>, d));
    printf("%-34s %8.2f %8.2f %8.2f %8.2f\n", "+ 3 ds_read_b128", cost_run(k_cost<0, 1>, d), cost_run(k_cost<1, 1>, d), cost_run(k_cost<2, 1>, d), cost_run(k_cost<3, 1>, d));
    printf("%-34s %8.2f %8.2f %8.2f %8.2f\n", "+ reads + gelu_mx<2> + store", cost_run(k_cost<0, 2>, d), cost_run(k_cost<1, 2>, d), cost_run(k_cost<2, 2>, d), cost_run(k_cost<3, 2>, d));
    printf("%-34s %8.2f\n", "gelu_mx<2> + store alone", cost_run(k_cost<9, 3>, d));
    CK(hipDeviceSynchronize());
    return 0;
}
