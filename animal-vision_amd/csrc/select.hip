// csrc/select.hip -- np.percentile (linear interpolation) on the device: the kernels that run a radix pass of csrc/radix_select.h over arrays
// (k_sel_pass) and over a band stack that only exists at reduced size (k_sel_pass_up, k_sel_cand), and the entry points that chain three passes.
// uv_mappers.py:32,61-62,73,104,142 (a20, a21).  Exact order statistics; the lerp between them is NumPy's float32 one.
#include "radix_select.h"
#include "stack_up.h"

using namespace avxk;

namespace {

constexpr int kT = kSelT;

// NJ percentiles per launch: the data pass walks the NJ arrays one after the other into NJ LDS histograms, and the
// last workgroup picks for each in turn -- the per-launch fixed costs (LDS clear / flush, ticket, tail latency)
// are paid once, which is most of the time of a pass at 1080p.
// The frame offset (blockIdx.y) is applied where a job is read: a local, rewritten copy of the argument struct would live in scratch memory.
template <int NJ>
__global__ __launch_bounds__(kT) void k_sel_pass(const SelPass a) {
    __shared__ uint32_t h[NJ][2048];
    const int t = threadIdx.x, f = blockIdx.y;  // gridDim.y == 1: the plain single-array form
    const bool last_pass = a.pass == 2;
    SelState* const st = a.st + (size_t)f * kSelMax;
    // The first eight 16-byte vectors of a thread's share of job j (all of it for a 1080p plane at one workgroup per CU): fetched a
    // job AHEAD -- job 0's while the histograms are cleared, job j + 1's before job j is visited -- so the jobs' memory round trips
    // overlap instead of adding up (a pass over four planes was four dependent round trips).
    const size_t stride = (size_t)gridDim.x * kT, i0 = (size_t)blockIdx.x * kT + t;
    auto job_vec = [&](int j, const float*& x, const float4*& xv, size_t& nvec, size_t& head, size_t& tail0) {
        x = a.job[j].x + (size_t)f * a.x_frame_stride;
        const size_t n = a.job[j].n, mis = ((16 - ((uintptr_t)x & 15)) & 15) / 4;
        head = mis < n ? mis : n;
        nvec = (n - head) / 4; tail0 = head + nvec * 4;
        xv = reinterpret_cast<const float4*>(x + head);
    };
    auto fetch8 = [&](int j, float4 (&v)[8]) {
        const float* x; const float4* xv; size_t nvec, head, tail0;
        job_vec(j, x, xv, nvec, head, tail0);
        if (nvec == 0) return;
#pragma unroll
        for (int q = 0; q < 8; ++q) { const size_t idx = i0 + q * stride; v[q] = xv[idx < nvec ? idx : nvec - 1]; }
    };
    float4 cur[8], nxt[8];
    fetch8(0, cur);
    for (int i = t; i < NJ * 2048; i += kT) (&h[0][0])[i] = 0;
    __syncthreads();
    uint32_t best[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) best[j] = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j >= a.n_jobs) break;
        if (j + 1 < NJ && j + 1 < a.n_jobs) fetch8(j + 1 < NJ ? j + 1 : j, nxt);
        const SelDigit d(a.pass == 0 ? 0u : st[j].prefix, a.pass == 0 ? 0u : st[j].mask, a.shift, a.bits, last_pass && a.job[j].r.has_next);
        SelRun run;
        auto visit = [&](float v) { sel_visit_run(d, v, h[j], best[j], run); };
        // 16-byte loads over the aligned body; the (<= 3 + 3) head / tail elements go to the first threads of block 0
        const float* x; const float4* xv; size_t nvec, head, tail0;
        job_vec(j, x, xv, nvec, head, tail0);
        // first batch: already here (cur); further batches (frames beyond 8 vectors per thread): eight loads in flight each, the ragged
        // end included (clamped index, masked visit)
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i0 + q * stride < nvec) { visit(cur[q].x); visit(cur[q].y); visit(cur[q].z); visit(cur[q].w); }
        for (size_t i = i0 + 8 * stride; i < nvec; i += 8 * stride) {
            float4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const size_t idx = i + q * stride; v[q] = xv[idx < nvec ? idx : nvec - 1]; }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (i + q * stride < nvec) { visit(v[q].x); visit(v[q].y); visit(v[q].z); visit(v[q].w); }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
        if (blockIdx.x == 0) {
            if ((size_t)t < head) visit(x[t]);
            if (tail0 + t < a.job[j].n && t < 4) visit(x[tail0 + t]);
        }
        sel_run_flush(run, h[j]);
    }
    sel_finish_pass<NJ>(h, best, a.n_jobs, a.pass, a.shift, a.bits, a.ticket, f, gridDim.y > 1 ? kSelTicketFrame : kSelTicketGrid, 0u, 0u, [&](int j) {
        return SelTail{st + j, a.hist + ((size_t)f * kSelMax + j) * 2048, a.job[j].r, a.job[j].out + (size_t)f * a.out_frame_stride, last_pass && a.job[j].r.has_next};
    });
}

// One radix pass over the values of a band stack that only exists at reduced size (stack_up.h): every thread recomputes the K
// resized + normalised values of its pixels and histograms them (one job).
// cand / cand_cnt: the SECOND pass also copies every value of the bin the first pass selected into cand[] (count in *cand_cnt) and tracks the smallest key
// above that bin, so the THIRD pass scans those candidates (k_sel_cand) instead of recomputing the whole stack a third time.
struct SelUpArgs { StackUp u; size_t cap_floats; uint32_t prefix0, mask0; int pass, shift, bits; SelState* st; uint32_t* hist; uint32_t* ticket; SelRank r; double* out;
                   float* cand; uint32_t* cand_cnt; };
constexpr uint32_t kSelStage = 3072;  // staged candidates per tile (12 KB of LDS); denser tiles take a second sweep
template <int K>
__global__ __launch_bounds__(kT) void k_sel_pass_up(const SelUpArgs a) {
    __shared__ uint32_t h[1][2048];
    __shared__ uint32_t scnt, sbase;
    __shared__ int redo;  // collect: 1 during the second sweep of a tile whose candidates outgrew the staging area (values are then written straight to cand[])
    const int t = threadIdx.x;
    const bool collect = a.pass == 1 && a.cand != nullptr;
    const bool find_next = (a.pass == 2 || collect) && a.r.has_next;  // collect: the smallest key above the first pass's bin (the successor when the candidates hold none)
    for (int i = t; i < 2048; i += kT) h[0][i] = 0;
    if (t == 0) { scnt = 0; redo = 0; }
    const SelDigit d(a.pass == 0 ? a.prefix0 : a.st->prefix, a.pass == 0 ? a.mask0 : a.st->mask, a.shift, a.bits, find_next);
    uint32_t best[1] = {0xffffffffu};
    __syncthreads();
    extern __shared__ float tile_lds[];
    float* stage = tile_lds + a.cap_floats;  // collect: this tile's candidates, up to kSelStage of them
    stack_tiles<K, true>(a.u, tile_lds, a.cap_floats, [&](int, int, float (&v)[K]) {
        const bool second = collect && redo;  // uniform
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (sel_visit(d, v[k], h[0], best[0], !second) && collect) {
                const uint32_t idx = atomicAdd(&scnt, 1u);
                if (second) a.cand[(size_t)sbase + idx] = v[k];
                else if (idx < kSelStage) stage[idx] = v[k];
            }
        }
    }, [&]() -> bool {
        if (!collect) return false;  // uniform
        const uint32_t m = scnt;
        const bool was_second = redo != 0, dense = !was_second && m > kSelStage;
        __syncthreads();  // everyone has read scnt / redo
        if (was_second) {
            if (t == 0) { scnt = 0; redo = 0; }
            __syncthreads();
            return false;
        }
        if (t == 0) {
            if (m) sbase = atomicAdd(a.cand_cnt, m);  // one reservation per tile
            scnt = 0;
            redo = dense ? 1 : 0;
        }
        __syncthreads();
        if (dense) return true;  // too many for the staging area (a flat region: every value in the bin): the tile is swept again and writes straight to cand[sbase + ...]
        for (uint32_t i = t; i < m; i += kT) a.cand[(size_t)sbase + i] = stage[i];
        __syncthreads();  // the staging area is free again
        return false;
    });
    const bool last_wg = sel_finish_pass<1>(h, best, 1, a.pass, a.shift, a.bits, a.ticket, 0, kSelTicketGrid /*up to 1,024 workgroups arrive here*/, a.prefix0, a.mask0,
                                            [&](int) { return SelTail{a.st, a.hist, a.r, a.out, find_next}; });
    if (last_wg && a.pass == 0 && a.cand_cnt && t == 0) *a.cand_cnt = 0;  // the next launch collects from zero (the kernel boundary publishes it)
}

// The third radix pass over the candidates the second one collected (k_sel_pass_up): *cand_cnt values, all inside the first pass's bin.  The successor
// found among keys above that bin is already in st->next_above.
__global__ __launch_bounds__(kT) void k_sel_cand(const SelUpArgs a) {
    __shared__ uint32_t h[1][2048];
    const int t = threadIdx.x;
    const bool find_next = a.r.has_next != 0;
    for (int i = t; i < 2048; i += kT) h[0][i] = 0;
    const SelDigit d(a.st->prefix, a.st->mask, a.shift, a.bits, find_next);
    const size_t n = *a.cand_cnt;
    uint32_t best[1] = {0xffffffffu};
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kT + t; i < n; i += (size_t)gridDim.x * kT) sel_visit(d, a.cand[i], h[0], best[0]);
    sel_finish_pass<1>(h, best, 1, 2, a.shift, a.bits, a.ticket, 0, kSelTicketGrid, a.prefix0, a.mask0, [&](int) { return SelTail{a.st, a.hist, a.r, a.out, find_next}; });
}

}  // namespace

void sel_launch_pass(const SelPass& a, int g, int F, hipStream_t s) {
    if (a.n_jobs == 1) hipLaunchKernelGGL(k_sel_pass<1>, dim3(g, F), dim3(kT), 0, s, a);
    else if (a.n_jobs == 2) hipLaunchKernelGGL(k_sel_pass<2>, dim3(g, F), dim3(kT), 0, s, a);
    else hipLaunchKernelGGL(k_sel_pass<4>, dim3(g, F), dim3(kT), 0, s, a);
}

// exact np.percentile(x_j, q_j) (linear interpolation) of n_j device floats -> *out_j (device doubles), up to kSelMax
// order statistics resolved by the same three passes
int run_percentiles(avx_ctx* ctx, const UvScratch& u, const PctReq* req, int count, hipStream_t s) {
    for (int base = 0; base < count; base += kSelMax) {
        SelPass a{};
        a.n_jobs = count - base < kSelMax ? count - base : kSelMax; a.st = u.sel; a.hist = u.hist; a.ticket = u.ticket;
        size_t nmax = 0;
        for (int j = 0; j < a.n_jobs; ++j) {
            const PctReq& r = req[base + j];
            a.job[j] = SelJob{r.x, r.n, sel_rank(r.n, r.q), r.out_dev};
            nmax = r.n > nmax ? r.n : nmax;
        }
        // few, fat workgroups: every workgroup flushes its non-empty LDS bins with global atomics
        const size_t want = (nmax + (size_t)kT * 16 - 1) / ((size_t)kT * 16);
        static const int wg_per_cu = [] { const char* e = getenv("AVX_SEL_WG"); const int v = e ? atoi(e) : 1; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
        const size_t cap = (size_t)ctx->num_cus * wg_per_cu;  // measured again in round 2 (hummingbird 1080p: 3.24 / 3.02 / 2.49 / 2.07 GP/s at 1 / 2 / 4 / 8 per CU): every workgroup pays the histogram clear, flush and ticket
        const int g = (int)(want < cap ? (want ? want : 1) : cap);
        for (int p = 0; p < 3; ++p) {
            a.pass = p; a.shift = kSelSplit.shift[p]; a.bits = kSelSplit.bits[p];
            sel_launch_pass(a, g, 1, s);
        }
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

// ---- internal entry points for other translation units of the library (mantis.hip) ---------------------
int avx_uv_percentiles_device(avx_ctx* ctx, int count, const float* const* x, const size_t* n, const double* q, double* const* out_dev, hipStream_t s) {
    UvScratch u;
    int rc = uv_small_scratch(ctx, s, &u);
    if (rc) return rc;
    PctReq rq[16];
    if (count > 16) return avx_fail(ctx, AVX_ERR_INVALID, "at most 16 percentiles per call");
    for (int i = 0; i < count; ++i) rq[i] = PctReq{x[i], n[i], q[i], out_dev[i]};
    return run_percentiles(ctx, u, rq, count, s);
}

int avx_uv_percentile_device(avx_ctx* ctx, const float* x, size_t n, double q, double* out_dev, hipStream_t s) {
    return avx_uv_percentiles_device(ctx, 1, &x, &n, &q, &out_dev, s);
}

// np.percentile(q) over the H x W x K values of a reduced-size band stack read through its resize (+ safe_norm): stack_up.h
int avx_uv_percentile_up_device(avx_ctx* ctx, const StackUp& up, double q, double* out_dev, hipStream_t s, float* cand_buf /*H * W * K floats, or NULL: three full passes*/) {
    UvScratch u;
    int rc = uv_small_scratch(ctx, s, &u);
    if (rc) return rc;
    SelUpArgs a{};
    a.u = up; a.st = u.sel; a.hist = u.hist; a.ticket = u.ticket; a.r = sel_rank((size_t)up.H * up.W * up.K, q); a.out = out_dev;
    static_assert(kT == 256, "AVX_STACK_TILES assumes 256 threads");
    const size_t tiles = (size_t)((up.W + kUpTW - 1) / kUpTW) * ((up.H + kUpTH - 1) / kUpTH), cap = (size_t)ctx->num_cus * 4;
    const int g = (int)(tiles < cap ? (tiles ? tiles : 1) : cap);
    a.cap_floats = stack_tile_floats(up.hs, up.ws, up.H, up.W, up.K);
    const size_t lds_tile = a.cap_floats * sizeof(float);
    AVX_REQUIRE(ctx, lds_tile <= 96 * 1024, "percentile through a resized stack: the tile's source rectangle does not fit LDS (%zu bytes)", lds_tile);
    // candidates: the second pass stages a tile's matching values in LDS (kSelStage floats behind the source rectangle) and copies them out once per tile
    const size_t lds_stage = (size_t)kSelStage * sizeof(float);
    const char* cand_env = getenv("AVX_MANTIS_CAND");  // read per call: tests flip it (0: three full passes)
    const bool use_cand = cand_buf && !(cand_env && cand_env[0] == '0') && lds_tile + lds_stage <= 120 * 1024;
    const size_t lds = lds_tile + (use_cand ? lds_stage : 0);
    AVX_REQUIRE(ctx, stack_k_tiled(up.K) && up.mm, "percentile through a resized stack: K=%d is not instantiated / no min-max table", up.K);
    AVX_STACK_K_SWITCH(up.K, AVX_HIP(ctx, hipFuncSetAttribute((const void*)k_sel_pass_up<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)))
    a.prefix0 = kSelPrefix01; a.mask0 = kSelMask01;  // safe_norm's values lie in [0, 1]
    if (use_cand) { a.cand = cand_buf; a.cand_cnt = u.ticket + 56; }  // word 56 of the ticket block: zero at rest (uv_small_scratch), re-zeroed by the first pass
    for (int p = 0; p < 3; ++p) {
        a.pass = p; a.shift = kSelSplit01.shift[p]; a.bits = kSelSplit01.bits[p];
        if (p == 2 && use_cand) {  // the candidates of the first pass's bin instead of the whole stack
            const int gc = (int)((size_t)ctx->num_cus < (size_t)g ? (size_t)ctx->num_cus : (size_t)g);
            hipLaunchKernelGGL(k_sel_cand, dim3(gc), dim3(kT), 0, s, a);
            break;
        }
        const size_t lds_p = (p == 1 && use_cand) ? lds : lds_tile;  // only the collecting pass carries the staging area
        AVX_STACK_K_SWITCH(up.K, hipLaunchKernelGGL(k_sel_pass_up<KT>, dim3(g), dim3(kT), lds_p, s, a))
    }
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}

extern "C" int avx_percentile(avx_ctx* ctx, const float* data, size_t n, double q, double* out_host, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, data && out_host && n > 0 && q >= 0.0 && q <= 100.0, "avx_percentile: bad arguments");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    UvScratch u;
    int rc = uv_small_scratch(ctx, s, &u);
    if (rc) return rc;
    const PctReq r{data, n, q, u.pct};
    rc = run_percentiles(ctx, u, &r, 1, s);
    if (rc) return rc;
    AVX_HIP(ctx, hipMemcpyAsync(out_host, u.pct, sizeof(double), hipMemcpyDeviceToHost, s));
    AVX_HIP(ctx, hipStreamSynchronize(s));
    return AVX_OK;
}
