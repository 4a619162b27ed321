// Probe (gfx950): does it matter how many 128-byte lines one 16-byte-per-lane memory instruction of a wave addresses?  The decoder upsampling
// (csrc/mst_mfma.hip, k_mst_convt2x2 / k_mst_convt2x2_16) reads its skip rows and writes its output rows so that one instruction moves 1 KB as 16
// bytes out of every other 64-byte pixel: 32 lines touched per instruction, each line completed by four instructions.  A whole-line access
// touches 8.  Persistent waves (CUs x 4 workgroups of 4 waves) move a buffer far past the Infinity Cache, 4 KB runs (64 pixels x 32 channels), two
// runs per step (the two output rows of a wave-tile), in two shapes that move the same bytes with the same number of instructions:
//   (a) scattered   instruction (odd, s) of a run: lane (p, h) moves the 16 bytes at 128 p + 64 odd + 32 h + 16 s      (today's kernels)
//   (b) lines       instruction i of a run:        lane l      moves the 16 bytes at 1024 i + 16 l
// Load side alone, store side alone, and both (a copy).  hipcc --offload-arch=gfx950 -O3 -o line_touch_probe line_touch_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

template <bool LINES> __device__ __forceinline__ unsigned ofs16(int lane, int i /*0..3*/) {
    if (LINES) return 1024u * i + 16u * lane;
    return 128u * (lane & 31) + 64u * (i >> 1) + 32u * (lane >> 5) + 16u * (i & 1);
}

// MODE 0: loads only, 1: stores only, 2: copy.  `pairs` steps in all; step j takes the runs j and pairs + j (4 KB each) of src / dst.
template <bool LINES, int MODE>
__global__ __launch_bounds__(256, 4) void k_probe(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, long pairs, uint4* __restrict__ sink) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = ofs16<LINES>(lane, i);
    uint4 acc = uint4{(unsigned)lane, 1u, 2u, 3u};
    for (long j = w; j < pairs; j += nw) {
        uint4 v[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t run = (size_t)(r ? pairs + j : j) * 4096;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (MODE != 1) v[r][i] = *reinterpret_cast<const uint4*>(src + run + o[i]);
                else v[r][i] = acc;
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t run = (size_t)(r ? pairs + j : j) * 4096;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (MODE != 0) *reinterpret_cast<uint4*>(dst + run + o[i]) = v[r][i];
                else { acc.x ^= v[r][i].x; acc.y ^= v[r][i].y; acc.z ^= v[r][i].z; acc.w ^= v[r][i].w; }
            }
        }
    }
    if (MODE == 0 && acc.x == 0x9e3779b9u && acc.y == 0x7f4a7c15u) sink[0] = acc;  // keeps the loads alive; the buffer never holds this
}

template <bool LINES, int MODE>
static int run(const unsigned char* s, unsigned char* d, long pairs, uint4* sink, int grid, int reps, std::vector<float>& us) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int r = -1; r < reps; ++r) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((k_probe<LINES, MODE>), dim3(grid), dim3(256), 0, 0, s, d, pairs, sink);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) us.push_back(ms * 1000.f);
    }
    CK(hipGetLastError());
    return 0;
}

int main(int argc, char** argv) {
    const size_t bytes = (size_t)1 << 30;  // read this much, write this much: the C = 64 decoder step's volume at 4K
    const int rounds = argc > 1 ? atoi(argv[1]) : 5, reps = 5;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount * 4;
    unsigned char *s, *d;
    uint4* sink;
    CK(hipMalloc(&s, bytes));
    CK(hipMalloc(&d, bytes));
    CK(hipMalloc(&sink, 16));
    CK(hipMemset(s, 0x5a, bytes));
    CK(hipMemset(d, 0, bytes));
    const long pairs = (long)(bytes / 8192);
    printf("line_touch_probe: %s, %d CUs, grid %d x 256, %.2f GB read / %.2f GB written per launch, %d rounds x %d launches per form, forms alternating\n", prop.name,
           prop.multiProcessorCount, grid, bytes / 1e9, bytes / 1e9, rounds, reps);
    const char* names[3] = {"loads only ", "stores only", "copy       "};
    std::vector<float> t[3][2];
    for (int r = 0; r < rounds; ++r) {  // the two shapes alternate inside a round, so drift of the box hits both alike
        if (run<false, 0>(s, d, pairs, sink, grid, reps, t[0][0]) || run<true, 0>(s, d, pairs, sink, grid, reps, t[0][1])) return 2;
        if (run<false, 1>(s, d, pairs, sink, grid, reps, t[1][0]) || run<true, 1>(s, d, pairs, sink, grid, reps, t[1][1])) return 2;
        if (run<false, 2>(s, d, pairs, sink, grid, reps, t[2][0]) || run<true, 2>(s, d, pairs, sink, grid, reps, t[2][1])) return 2;
    }
    for (int m = 0; m < 3; ++m) {
        float med[2];
        for (int f = 0; f < 2; ++f) {
            std::vector<float>& v = t[m][f];
            std::sort(v.begin(), v.end());
            med[f] = v[v.size() / 2];
            const double moved = (m == 2 ? 2.0 : 1.0) * bytes;
            printf("%s  %s  %8.1f us (%8.1f - %8.1f)   %5.2f TB/s (%5.2f - %5.2f)\n", names[m], f ? "(b) lines    " : "(a) scattered", med[f], v.front(), v.back(),
                   moved / med[f] * 1e-6, moved / v.back() * 1e-6, moved / v.front() * 1e-6);
        }
        printf("%s  (b) against (a): %+.1f %%\n", names[m], 100.0 * (med[1] / med[0] - 1.0));
    }
    // the copy has to have copied: spot-check the last run of each half
    std::vector<unsigned char> chk(4096);
    CK(hipMemcpy(chk.data(), d + bytes - 4096, 4096, hipMemcpyDeviceToHost));
    int bad = 0;
    for (unsigned char c : chk) bad += c != 0x5a;
    printf("copy check: %d wrong bytes in the last run\n", bad);
    return bad != 0;
}
