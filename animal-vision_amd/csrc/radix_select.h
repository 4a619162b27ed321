// csrc/radix_select.h -- the core of the exact order statistic (np.percentile): a three-pass radix select on order-preserving keys.
//
// One launch per radix pass.  Every workgroup (kSelT threads) histograms its share of the values in LDS (sel_visit / sel_visit_run); sel_finish_pass
// then ends the pass: the non-empty bins go to the global histogram with atomics, and the LAST workgroup to arrive picks the bin that holds the rank,
// narrows the prefix, re-zeroes the histogram and the ticket, and -- on the last pass -- resolves the successor key and performs NumPy's float32 lerp.
// Pass 0 takes its state from the arguments: no init launch, no memset.  Who runs a pass: select.hip (k_sel_pass over arrays, k_sel_pass_up / k_sel_cand
// over a band stack read through its resize) and uv.hip (k_bee_tile, whose "array" is the honeybee tile pipeline).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dichromat_common.h"

constexpr int kSelT = 256;   // threads of a workgroup that runs a pass
constexpr int kSelMax = 4;   // order statistics resolved together by one set of passes

struct SelState {
    uint32_t prefix, mask;      // key bits fixed so far
    unsigned long long rank;    // remaining 0-based rank inside the selected prefix
    uint32_t key_lo, key_hi;    // results: key of x[k] and of x[k+1]
    uint32_t cnt_in_bin;        // size of the finally selected bin (duplicates of x[k])
    uint32_t next_key;          // smallest key > key_lo
    uint32_t next_above;        // smallest key above the selected 22-bit prefix range (last histogram pass)
};

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
// np.percentile(x, q) of n values, linear interpolation: x[rank0] + gamma (x[rank0 + 1] - x[rank0]).  NumPy (2.x) evaluates the virtual index in the
// array's dtype: float32(n - 1) * (float32(q) / float32(100)).
struct SelRank { unsigned long long rank0; float gamma; int has_next; };
inline SelRank sel_rank(size_t n, double q) {
    const float vi = (float)(n - 1) * ((float)q / 100.0f);
    float lo = floorf(vi);
    if (lo < 0) lo = 0;
    if (lo > (float)(n - 1)) lo = (float)(n - 1);
    return SelRank{(unsigned long long)lo, vi - lo, (size_t)lo + 1 < n ? 1 : 0};
}

// The three digits of a key, most significant first.
struct SelSplit { int shift[3], bits[3]; };
constexpr SelSplit kSelSplit = {{21, 10, 0}, {11, 11, 10}};
// Values in [0, 1]: every key starts with the bits 10 (positive, exponent < 128; prefix0 / mask0 below), so the digits are taken from bits 29..19,
// 18..8, 7..0 -- the first histogram then resolves 16 mantissa steps per binade instead of 4, and its LDS atomics collide a quarter as often (the
// plain split put an eighth of a uniform [0, 1] sample into ONE bin).
constexpr SelSplit kSelSplit01 = {{19, 8, 0}, {11, 11, 8}};
constexpr uint32_t kSelPrefix01 = 0x80000000u, kSelMask01 = 0xc0000000u;

// One pass over up to kSelMax arrays (k_sel_pass, select.hip).  blockIdx.y = frame: the arrays of a job are x_frame_stride floats apart, its results
// out_frame_stride doubles apart, and every frame has kSelMax states, kSelMax x 2048 bins and one ticket word of its own.
struct SelJob { const float* x; size_t n; SelRank r; double* out; };
struct SelPass { int n_jobs, pass, shift, bits; SelState* st; uint32_t* hist; uint32_t* ticket; SelJob job[kSelMax];
                 size_t x_frame_stride; int out_frame_stride; };
// launches pass a.pass of a.n_jobs jobs on g workgroups for each of F frames (the kernel is instantiated for 1, 2 and 4 jobs)
void sel_launch_pass(const SelPass& a, int g, int F, hipStream_t s);

// ---- device side ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// What a visit needs of the pass and the job: the prefix selected so far, the digit of this pass, and whether keys above the prefix range are
// candidates for the successor x[k + 1] (find_next).
struct SelDigit {
    uint32_t prefix, mask, above;  // above: the largest key with this prefix
    int shift, nb;
    bool find_next;
    __device__ __forceinline__ SelDigit(uint32_t prefix_, uint32_t mask_, int shift_, int bits, bool find_next_)
        : prefix(prefix_), mask(mask_), above(prefix_ | ~mask_), shift(shift_), nb(1 << bits), find_next(find_next_) {}
};

// The plain visit: one LDS atomic per value inside the prefix (count = false: none, the value was counted before); the smallest key above the prefix
// range is kept in best.  Returns whether the value lies inside the prefix.
__device__ __forceinline__ bool sel_visit(const SelDigit& d, float v, uint32_t* h, uint32_t& best, bool count = true) {
    const uint32_t k = f2key(v);
    if ((k & d.mask) == d.prefix) {
        if (count) atomicAdd(&h[(k >> d.shift) & (d.nb - 1)], 1u);
        return true;
    }
    if (d.find_next && k > d.above && k < best) best = k;
    return false;
}

// The visit with run-length combining: neighbouring samples of a frame usually share a bin (always, nearly, in the first pass, where a bin is a
// quarter of a binade), and 64 lanes adding 1 to the same LDS word serialise -- a thread keeps (bin, count) of its current run and issues one atomic
// per run instead of one per sample.  sel_run_flush after the last visit.
struct SelRun { uint32_t bin = 0xffffffffu, cnt = 0; };
__device__ __forceinline__ void sel_run_flush(const SelRun& run, uint32_t* h) {
    if (run.cnt) atomicAdd(&h[run.bin], run.cnt);
}
__device__ __forceinline__ void sel_visit_run(const SelDigit& d, float v, uint32_t* h, uint32_t& best, SelRun& run) {
    const uint32_t k = f2key(v);
    if ((k & d.mask) == d.prefix) {
        const uint32_t b = (k >> d.shift) & (d.nb - 1);
        if (b == run.bin) { ++run.cnt; }
        else {
            sel_run_flush(run, h);
            run.bin = b; run.cnt = 1;
        }
    } else if (d.find_next && k > d.above && k < best) best = k;
}

// The last workgroup of a pass, for one job: pick the bin holding the rank, narrow the prefix, on the last pass resolve x[k], x[k+1] and NumPy's
// float32 lerp; the histogram is left zero.  prefix0 / mask0: key bits every element is known to share before the first pass (0 / 0: none).
__device__ __forceinline__ void sel_pick(uint32_t* hist, SelState* st, int pass, int shift, int bits, SelRank rk, double* out, uint32_t prefix0, uint32_t mask0) {
    __shared__ unsigned long long csum[kSelT];
    __shared__ int first_after[kSelT / 64];
    __shared__ int sel_chunk, sel_bin;
    __shared__ unsigned long long sel_rem;
    __shared__ uint32_t sel_cnt;
    const int nb = 1 << bits, t = threadIdx.x, per = nb / kSelT;
    const bool last_pass = pass == 2;
    const uint32_t prefix = pass == 0 ? prefix0 : st->prefix, mask = pass == 0 ? mask0 : st->mask;
    uint32_t loc[8];
    unsigned long long sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) loc[i] = i < per ? __hip_atomic_load(&hist[t * per + (i < per ? i : 0)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) sum += loc[i];
    // inclusive scan of the 256 chunk sums: within a wave by shuffles, across the four waves through LDS (two barriers; the
    // Hillis-Steele form in LDS took sixteen, and the pick is pure latency on the critical path of every pass)
    unsigned long long incl = sum;
    {
        const int lane = t & 63, wave = t >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        __syncthreads();  // csum is free (a previous job's readers are done)
        if (lane == 63) csum[wave] = incl;
        if (t == 0) sel_chunk = kSelT - 1;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += csum[w];
    }
    const unsigned long long r = pass == 0 ? rk.rank0 : st->rank;
    const unsigned long long excl = incl - sum;
    if (excl <= r && r < incl) sel_chunk = t;
    __syncthreads();
    if (t == sel_chunk) {
        unsigned long long cum = excl;
        int i = 0;
        for (; i < per; ++i) {
            if (cum + loc[i] > r) break;
            cum += loc[i];
        }
        if (i == per) i = per - 1;
        const int b = t * per + i;
        st->prefix = prefix | ((uint32_t)b << shift);
        st->mask = mask | ((uint32_t)(nb - 1) << shift);
        st->rank = r - cum;
        if (pass == 0) st->next_above = 0xffffffffu;
        if (last_pass) { st->key_lo = prefix | (uint32_t)b; st->cnt_in_bin = loc[i]; sel_bin = b; sel_rem = r - cum; sel_cnt = loc[i]; }
    }
    if (last_pass) {
        __syncthreads();
        int f = 0x7fffffff;
        for (int i = per - 1; i >= 0; --i)
            if (loc[i] && t * per + i > sel_bin) f = t * per + i;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(f, o); f = v < f ? v : f; }
        if ((t & 63) == 0) first_after[t >> 6] = f;
        __syncthreads();
        if (t == 0) {
            int m = first_after[0];
            for (int w = 1; w < kSelT / 64; ++w) m = first_after[w] < m ? first_after[w] : m;
            const uint32_t next_above = __hip_atomic_load(&st->next_above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t next_key = m != 0x7fffffff ? (prefix | (uint32_t)m) : next_above;
            const uint32_t key_lo = prefix | (uint32_t)sel_bin;
            const float lo = key2f(key_lo);
            float hi = lo;
            if (rk.has_next && sel_rem + 1 >= sel_cnt) hi = next_key == 0xffffffffu ? lo : key2f(next_key);
            const float diff = hi - lo;
            float res = lo + diff * rk.gamma;
            if (rk.gamma >= 0.5f) res = hi - diff * (1.0f - rk.gamma);
            *out = (double)res;
        }
    }
    for (int i = 0; i < per; ++i) hist[t * per + i] = 0;
    __syncthreads();
}

// How the workgroups of a pass find the last one.  kSelTicketGrid: the grid owns the whole ticket block and arrives through the two-level
// ticket_is_last (single-frame grids of up to 1,024 workgroups), which leaves its counters zero.  kSelTicketFrame: one word per frame, counted up
// by the frame's gridDim.x workgroups and reset by the last (the batched grids, blockIdx.y = frame).
// ticket / frame: the ticket block and the frame's word in it (kSelTicketGrid: frame 0).  The block is taken by reference so that a kernel passes its argument
// itself and the pointer is read where the ticket is taken: computed at the call, it stays live across the whole tail, and k_bee_tile then keeps a stack slot.
enum SelTicket { kSelTicketGrid, kSelTicketFrame };
// One job as the end of a pass sees it.
struct SelTail { SelState* st; uint32_t* hist; SelRank r; double* out; bool find_next; };

// The end of a radix pass, called by every thread of every workgroup after its last visit.  h / best: the workgroup's LDS histograms and each thread's
// successor candidates, one per job; tail(j): SelTail of job j < n_jobs <= NJ.  In order: successor reduction (wave, workgroup, atomicMin into
// st->next_above), flush of the non-empty LDS bins, wait for the workgroup's own atomics, ticket, and in the last workgroup the pick of every job (which
// re-zeroes the histogram) and the ticket reset.  Returns whether this workgroup was the last.
// Everything the workgroups exchange travels in agent-scope atomics (histogram, successor key, ticket) and is read back with agent-scope atomic
// loads, so no cache write-back / invalidate (__threadfence: a whole-L2 flush per workgroup on this multi-XCD part) is needed: only this wave's
// atomics must have been performed before the ticket is taken.
template <int NJ, class Tail>
__device__ __forceinline__ bool sel_finish_pass(uint32_t (&h)[NJ][2048], const uint32_t (&best)[NJ], int n_jobs, int pass, int shift, int bits, uint32_t* const& ticket, int frame,
                                                SelTicket form, uint32_t prefix0, uint32_t mask0, Tail tail) {
    __shared__ uint32_t wmin[kSelT / 64];
    __shared__ int is_last;
    const int t = threadIdx.x, nb = 1 << bits;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j >= n_jobs) break;
        const SelTail tl = tail(j);
        if (!tl.find_next) continue;
        uint32_t b = best[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t v = __shfl_xor(b, o); b = v < b ? v : b; }
        __syncthreads();
        if ((t & 63) == 0) wmin[t >> 6] = b;
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < kSelT / 64; ++w) b = wmin[w] < b ? wmin[w] : b;
            if (b != 0xffffffffu) atomicMin(&tl.st->next_above, b);
        }
    }
    __syncthreads();
    for (int j = 0; j < n_jobs; ++j) {
        uint32_t* hist = tail(j).hist;
        for (int i = t; i < nb; i += kSelT)
            if (h[j][i]) atomicAdd(&hist[i], h[j][i]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) is_last = form == kSelTicketFrame ? atomicAdd(ticket + frame, 1u) == gridDim.x - 1 : avxk::ticket_is_last(ticket, blockIdx.x, gridDim.x);
    __syncthreads();
    if (!is_last) return false;
    for (int j = 0; j < n_jobs; ++j) {
        const SelTail tl = tail(j);
        sel_pick(tl.hist, tl.st, pass, shift, bits, tl.r, tl.out, prefix0, mask0);
    }
    if (t == 0 && form == kSelTicketFrame) ticket[frame] = 0;
    return true;
}
