// csrc/wall.hip -- the species wall of the `wall` command: the labelled contact sheet of gallery.hip for a batch of video frames.
// All tiles of a wall are uint8 H x W x 3 sources of one size resized to one h x w, so everything but the source pointers is
// known before the first frame: avx_wall_layout_create chooses the resize mode, builds the axis tables and uploads them with the
// label segments once, and avx_wall_compose_u8 is one launch per batch whose source pointers travel as kernel arguments -- no
// upload, allocation or synchronisation per call.
//
// A workgroup owns one piece of one canvas row: up to `cw` pixels of one grid column.  It copies the band of source rows that
// piece's samples read into LDS with 16-byte loads (a row segment is contiguous in the source), every thread then computes one
// canvas pixel out of LDS with gallery.hip's statements (gallery_px.h: tile_sample; label_common.h), the bytes are collected in
// LDS and leave as 16-byte stores.  The mode is a template parameter; the row a workgroup works on tells it whether it is
// background, tile or label, so the label's distance loop runs in label rows only.  No workgroup waits for another.
#include <vector>

#include "avx_internal.h"
#include "gallery_px.h"

namespace {

constexpr int kWT = 256;
constexpr int kWallMaxTiles = 64;        // source pointers of one launch (kernel arguments)
constexpr size_t kWallLds = 48 << 10;    // LDS budget of a workgroup: three workgroups per CU
constexpr uint32_t kWallMagic = 0x77616c6cu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));  // a 16-byte load from any address (global_load_dwordx4)

struct WallSrcs { const uint8_t* p[kWallMaxTiles]; };

struct WallArgs {
    const float* seg; const uint32_t* tabs; const int* tile_seg;  // tile_seg [n][2]: {seg_offset, seg_count}
    int n, cols, rows, cell_h, cell_w, pad, strip_h;
    int H, W, h, w, isx, isy, xo, yo, xm, ym, ly0;
    int Hc, Wc;            // the canvas, both even
    int cw, nsub;          // pixels of a piece, pieces of a column
    int wp, mr;            // pixels of a staged source row (a multiple of 16: rows start 16-byte aligned in LDS), rows staged at most
    int obuf;              // bytes of the output staging in front of the staged rows
    size_t src_stride, canvas_stride;
    uint8_t bg[3];
    uint8_t* canvas;
};

// the source rows [r0, r0 + nr) and pixels [x0, x0 + nx) that the samples (tx0 .. tx1 - 1, ty) read
template <int MODE>
__device__ __forceinline__ void wall_band(const WallArgs& a, int tx0, int tx1, int ty, int& r0, int& nr, int& x0, int& nx) {
    if (MODE == M_COPY) { r0 = ty; nr = 1; x0 = tx0; nx = tx1 - tx0; }
    else if (MODE == M_AREA_FAST) { r0 = ty * a.isy; nr = a.isy; x0 = tx0 * a.isx; nx = (tx1 - tx0) * a.isx; }
    else if (MODE == M_AREA) {
        const AxisArea ax = area_axis(a.tabs, a.xo, a.w, a.xm), ay = area_axis(a.tabs, a.yo, a.h, a.ym);
        r0 = ay.start[ty]; nr = ay.cnt[ty];
        x0 = ax.start[tx0]; nx = ax.start[tx1 - 1] + ax.cnt[tx1 - 1] - x0;
    } else {
        const AxisLin ax = lin_axis(a.tabs, a.xo, a.w, a.xm), ay = lin_axis(a.tabs, a.yo, a.h, a.ym);
        r0 = ay.ofs[ty]; nr = 2;
        x0 = ax.ofs[tx0]; nx = ax.ofs[tx1 - 1] + 2 - x0;
    }
    // never past the source or the staging, whatever the tables say
    if (r0 < 0) r0 = 0;
    if (x0 < 0) x0 = 0;
    if (r0 > a.H - 1) r0 = a.H - 1;
    if (x0 > a.W - 1) x0 = a.W - 1;
    if (nr > a.H - r0) nr = a.H - r0;
    if (nx > a.W - x0) nx = a.W - x0;
    if (nx > a.wp) nx = a.wp;
    if (nr > a.mr) nr = a.mr;
}

template <int MODE, bool STAGE>
__global__ __launch_bounds__(kWT) void k_wall_compose(WallArgs a, WallSrcs srcs) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    // blockIdx.x = (canvas row, grid column, piece); blockIdx.y = frame
    const int s = (int)(blockIdx.x % (unsigned)a.nsub);
    const int col = (int)((blockIdx.x / (unsigned)a.nsub) % (unsigned)a.cols);
    const int Y = (int)(blockIdx.x / ((unsigned)a.nsub * (unsigned)a.cols));
    const size_t f = blockIdx.y;
    // The piece in the column's own coordinate u (canvas x = pad + col * cell_w + u; the tile is 0 <= u < w): the first piece of
    // the first column takes the left pad along, the last column runs to the canvas edge.
    const int u_end = col == a.cols - 1 ? a.Wc - a.pad - col * a.cell_w : a.cell_w;
    const int u0 = s * a.cw + (s == 0 && col == 0 ? -a.pad : 0);
    const int u1 = (s + 1) * a.cw < u_end ? (s + 1) * a.cw : u_end;
    const int npx = u1 - u0;
    if (npx <= 0) return;
    const int yy = Y - a.pad;
    const int row = yy >= 0 ? yy / a.cell_h : 0, ty = yy - row * a.cell_h;
    const int i = row * a.cols + col;
    const int tx0 = s * a.cw, tx1 = u1 < a.w ? u1 : a.w;  // the tile's samples in this piece
    const bool tile_row = yy >= 0 && row < a.rows && i < a.n && ty < a.h + a.strip_h && tx1 > tx0;  // workgroup-uniform

    GalTile t{};
    t.H = a.H; t.W = a.W; t.h = a.h; t.w = a.w; t.isx = a.isx; t.isy = a.isy;
    t.xo = a.xo; t.yo = a.yo; t.xm = a.xm; t.ym = a.ym; t.ly0 = a.ly0; t.mode = MODE;
    const uint8_t* src = nullptr;
    int r0 = 0, nr = 0, x0 = 0, nx = 0;
    if (tile_row) {
        src = srcs.p[i] + f * a.src_stride;
        t.seg_off = a.tile_seg[2 * i]; t.nseg = a.tile_seg[2 * i + 1];
        if (STAGE && ty < a.h) {
            wall_band<MODE>(a, tx0, tx1, ty, r0, nr, x0, nx);
            uint8_t* stage = smem + a.obuf;
            const int rs = a.wp * 3, nb = nx * 3, nv = nb >> 4, tail = nb & 15;
            for (int q = tid; q < nr * nv; q += kWT) {
                const int j = q / nv, v = q - j * nv;
                *(u32x4*)(stage + j * rs + 16 * v) = *(const u32x4_u*)(src + ((size_t)(r0 + j) * a.W + x0) * 3 + 16 * v);
            }
            for (int q = tid; q < nr * tail; q += kWT) {
                const int j = q / tail, b = 16 * nv + (q - j * tail);
                stage[j * rs + b] = src[((size_t)(r0 + j) * a.W + x0) * 3 + b];
            }
            __syncthreads();
        }
    }
    // the statements index the source by (row, pixel): staged, they get the band in LDS under the source's own coordinates
    if (STAGE) { t.src = smem + a.obuf - ((size_t)r0 * a.wp + x0) * 3; t.W = a.wp; }
    else t.src = src;

    // one canvas pixel per thread, into LDS at the canvas address's own phase so that 16-byte stores line up
    uint8_t* crow = a.canvas + f * a.canvas_stride + ((size_t)Y * a.Wc + (a.pad + col * a.cell_w + u0)) * 3;
    const int ph = (int)((uintptr_t)crow & 15);
    for (int k = tid; k < npx; k += kWT) {
        const int tx = u0 + k;
        uint8_t o[3] = {a.bg[0], a.bg[1], a.bg[2]};
        if (tile_row && tx >= 0 && tx < t.w) {
            o[0] = o[1] = o[2] = 0;  // strip black
            if (ty < t.h) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)tile_sample<uint8_t, MODE>(t, a.tabs, c, tx, ty);
            }
            if (ty >= t.ly0 && t.nseg > 0) {  // the label, as k_draw_label draws it on the tile-plus-strip image (no segments: it changes nothing)
                const float d = label_dist(a.seg + 6 * (size_t)t.seg_off, t.nseg, (float)tx, (float)ty);
                const float co = cover(d, kHalfOutline), ct = cover(d, kHalfText);
                const bool inbox = ty >= t.h;  // the box is the strip: (0, h, w - 1, h + strip_h - 1)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = label_blend(o[c], inbox, co, ct);
            }
        }
        smem[ph + 3 * k] = o[0]; smem[ph + 3 * k + 1] = o[1]; smem[ph + 3 * k + 2] = o[2];
    }
    __syncthreads();
    const int nbytes = npx * 3;
    int head = (16 - ph) & 15;
    head = head < nbytes ? head : nbytes;
    const int nv = (nbytes - head) >> 4, tail0 = head + 16 * nv;
    for (int v = tid; v < nv; v += kWT) *(u32x4*)(crow + head + 16 * v) = *(const u32x4*)(smem + ph + head + 16 * v);
    for (int b = tid; b < head; b += kWT) crow[b] = smem[ph + b];
    for (int b = tail0 + tid; b < nbytes; b += kWT) crow[b] = smem[ph + b];
}

}  // namespace

struct avx_wall_layout {
    uint32_t magic;
    avx_ctx* ctx;
    int mode, stage;
    size_t lds;
    void* dev;  // [segments][tables][tile_seg], 256-byte aligned sections
    WallArgs a;
};

namespace {

// source rows and pixels one piece's band can take at most (wall_band's extents, over every row and piece)
void wall_band_max(const GalTile& g, const GalTables& gt, int cw, int* rows, int* px) {
    const uint32_t* tb = gt.tabs.data();
    int mr = 1, mp = 1;
    for (int tx0 = 0; tx0 < g.w; tx0 += cw) {
        const int tx1 = tx0 + cw < g.w ? tx0 + cw : g.w;
        int nx;
        if (g.mode == M_COPY) nx = tx1 - tx0;
        else if (g.mode == M_AREA_FAST) nx = (tx1 - tx0) * g.isx;
        else if (g.mode == M_AREA) nx = (int)tb[g.xo + tx1 - 1] + (int)tb[g.xo + g.w + tx1 - 1] - (int)tb[g.xo + tx0];
        else nx = (int)tb[g.xo + tx1 - 1] + 2 - (int)tb[g.xo + tx0];
        nx = nx < g.W ? nx : g.W;
        mp = nx > mp ? nx : mp;
    }
    if (g.mode == M_AREA_FAST) mr = g.isy;
    else if (g.mode == M_AREA) { for (int y = 0; y < g.h; ++y) mr = (int)tb[g.yo + g.h + y] > mr ? (int)tb[g.yo + g.h + y] : mr; }
    else if (g.mode == M_LINEAR) mr = 2;
    *rows = mr < g.H ? mr : g.H; *px = mp;
}

// Copy takes one source row per piece and linear two: they always fit the budget, so only the area modes have an unstaged form.
void wall_launch(int mode, bool stage, dim3 grid, size_t lds, hipStream_t s, const WallArgs& a, const WallSrcs& p) {
    switch (mode) {
        case M_COPY: hipLaunchKernelGGL((k_wall_compose<M_COPY, true>), grid, dim3(kWT), lds, s, a, p); break;
        case M_AREA_FAST:
            if (stage) hipLaunchKernelGGL((k_wall_compose<M_AREA_FAST, true>), grid, dim3(kWT), lds, s, a, p);
            else hipLaunchKernelGGL((k_wall_compose<M_AREA_FAST, false>), grid, dim3(kWT), lds, s, a, p);
            break;
        case M_AREA:
            if (stage) hipLaunchKernelGGL((k_wall_compose<M_AREA, true>), grid, dim3(kWT), lds, s, a, p);
            else hipLaunchKernelGGL((k_wall_compose<M_AREA, false>), grid, dim3(kWT), lds, s, a, p);
            break;
        default: hipLaunchKernelGGL((k_wall_compose<M_LINEAR, true>), grid, dim3(kWT), lds, s, a, p); break;
    }
}

}  // namespace

extern "C" int avx_wall_max_tiles(void) { return kWallMaxTiles; }

extern "C" int avx_wall_layout_create(avx_ctx* ctx, int H, int W, int h, int w, int n_tiles, const int* seg_offset, const int* seg_count,
                                      const float* segments_host, int n_segments, int strip_h, int pad, int cols, const int bg_rgb[3],
                                      avx_wall_layout** out_layout) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, out_layout, "avx_wall_layout_create: out_layout is NULL");
    *out_layout = nullptr;
    AVX_REQUIRE(ctx, n_tiles >= 1 && n_tiles <= kWallMaxTiles, "avx_wall_layout_create: need 1..%d tiles (got %d)", kWallMaxTiles, n_tiles);
    AVX_REQUIRE(ctx, H > 0 && W > 0 && h > 0 && w > 0 && h <= (1 << 16) && w <= (1 << 16) && (size_t)H * W < ((size_t)1 << 29),
                "avx_wall_layout_create: bad size %d x %d -> %d x %d", H, W, h, w);
    AVX_REQUIRE(ctx, cols >= 1 && cols <= 4096 && pad >= 0 && pad <= 4096 && strip_h >= 0 && strip_h <= 4096,
                "avx_wall_layout_create: bad layout (cols %d, pad %d, strip %d)", cols, pad, strip_h);
    AVX_REQUIRE(ctx, bg_rgb, "avx_wall_layout_create: bg is NULL");
    for (int c = 0; c < 3; ++c) AVX_REQUIRE(ctx, bg_rgb[c] >= 0 && bg_rgb[c] <= 255, "avx_wall_layout_create: bg[%d] = %d is not in 0..255", c, bg_rgb[c]);
    AVX_REQUIRE(ctx, n_segments >= 0 && n_segments <= (1 << 20) && (n_segments == 0 || segments_host), "avx_wall_layout_create: bad segment table");
    AVX_REQUIRE(ctx, n_segments == 0 || (seg_offset && seg_count), "avx_wall_layout_create: segments without seg_offset / seg_count");
    std::vector<int> tile_seg(2 * (size_t)n_tiles, 0);
    for (int i = 0; i < n_tiles && seg_offset && seg_count; ++i) {
        AVX_REQUIRE(ctx, seg_offset[i] >= 0 && seg_count[i] >= 0 && (int64_t)seg_offset[i] + seg_count[i] <= n_segments,
                    "avx_wall_layout_create: tile %d: segments [%d, %d + %d) past the table of %d", i, seg_offset[i], seg_offset[i], seg_count[i], n_segments);
        tile_seg[2 * i] = seg_offset[i]; tile_seg[2 * i + 1] = seg_count[i];
    }
    const int64_t cell_h = (int64_t)h + strip_h + pad, cell_w = (int64_t)w + pad, rows = (n_tiles + cols - 1) / cols;
    const int64_t Hg = rows * cell_h + pad, Wg = cols * cell_w + pad;  // the gallery's canvas
    const int64_t Hc = Hg + (Hg & 1), Wc = Wg + (Wg & 1);
    AVX_REQUIRE(ctx, Hc * Wc < ((int64_t)1 << 29), "avx_wall_layout_create: the %lld x %lld canvas is too large", (long long)Hc, (long long)Wc);

    GalTile g{};
    g.H = H; g.W = W; g.h = h; g.w = w;
    GalTables gt;
    gt.place(g);  // the mode and tables avx_gallery_compose_u8 gives such a tile

    // the widest piece whose band of source rows fits the LDS budget; none: the samples read the source itself
    int cw = 256, stage = 0, wp = 16, mrows = 1;
    size_t lds = 0;
    auto obuf_of = [&](int c) { return (size_t)(((c + pad + 1) * 3 + 16 + 15) & ~15); };
    for (int c = 256; c >= 32 && !stage; c >>= 1) {
        int mr, mp;
        wall_band_max(g, gt, c, &mr, &mp);
        const int p16 = (mp + 15) & ~15;
        const size_t need = obuf_of(c) + (size_t)mr * p16 * 3;
        if (need <= kWallLds) { cw = c; stage = 1; wp = p16; mrows = mr; lds = need; }
    }
    if (!stage) { cw = 256; lds = obuf_of(cw); }
    if (!stage && (g.mode == M_COPY || g.mode == M_LINEAR))
        return avx_fail(ctx, AVX_ERR_UNSUPPORTED, "avx_wall_layout_create: pad %d leaves no room for a source row in a workgroup's LDS", pad);
    const int64_t u_max = cell_w + (Wc - Wg);
    const int64_t nsub = (u_max + cw - 1) / cw;
    AVX_REQUIRE(ctx, Hc * cols * nsub < ((int64_t)1 << 31), "avx_wall_layout_create: too many pieces");

    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_seg = up(sizeof(float) * 6 * (size_t)n_segments), b_tab = up(4 * gt.tabs.size()), b_ts = up(4 * tile_seg.size());
    std::vector<uint8_t> blob(b_seg + b_tab + b_ts + 256, 0);
    if (n_segments) memcpy(blob.data(), segments_host, sizeof(float) * 6 * (size_t)n_segments);
    if (!gt.tabs.empty()) memcpy(blob.data() + b_seg, gt.tabs.data(), 4 * gt.tabs.size());
    memcpy(blob.data() + b_seg + b_tab, tile_seg.data(), 4 * tile_seg.size());

    AVX_HIP(ctx, hipSetDevice(ctx->device));
    void* dev = nullptr;
    if (hipMalloc(&dev, blob.size()) != hipSuccess) return avx_fail(ctx, AVX_ERR_NOMEM, "avx_wall_layout_create: hipMalloc(%zu) failed", blob.size());
    hipError_t e = hipMemcpy(dev, blob.data(), blob.size(), hipMemcpyHostToDevice);  // synchronous: the blob is a local
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return avx_fail(ctx, AVX_ERR_HIP, "avx_wall_layout_create: upload failed: %s", hipGetErrorString(e));
    }
    avx_wall_layout* L = new avx_wall_layout{};
    L->magic = kWallMagic; L->ctx = ctx; L->mode = g.mode; L->stage = stage; L->lds = lds; L->dev = dev;
    WallArgs& a = L->a;
    a.seg = (const float*)dev;
    a.tabs = (const uint32_t*)((uint8_t*)dev + b_seg);
    a.tile_seg = (const int*)((uint8_t*)dev + b_seg + b_tab);
    a.n = n_tiles; a.cols = cols; a.rows = (int)rows; a.cell_h = (int)cell_h; a.cell_w = (int)cell_w; a.pad = pad; a.strip_h = strip_h;
    a.H = H; a.W = W; a.h = h; a.w = w; a.isx = g.isx; a.isy = g.isy; a.xo = g.xo; a.yo = g.yo; a.xm = g.xm; a.ym = g.ym;
    a.ly0 = gal_label_row0(h);
    a.Hc = (int)Hc; a.Wc = (int)Wc; a.cw = cw; a.nsub = (int)nsub; a.wp = wp; a.mr = mrows; a.obuf = (int)obuf_of(cw);
    for (int c = 0; c < 3; ++c) a.bg[c] = (uint8_t)bg_rgb[c];
    *out_layout = L;
    return AVX_OK;
}

extern "C" int avx_wall_layout_destroy(avx_ctx* ctx, avx_wall_layout* layout) {
    if (!ctx) return AVX_ERR_INVALID;
    if (!layout) return AVX_OK;
    AVX_REQUIRE(ctx, layout->magic == kWallMagic && layout->ctx == ctx, "avx_wall_layout_destroy: not a layout of this context");
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    layout->magic = 0;
    hipError_t e = hipFree(layout->dev);
    delete layout;
    AVX_HIP(ctx, e);
    return AVX_OK;
}

extern "C" int avx_wall_canvas_size(const avx_wall_layout* layout, int* Hc, int* Wc) {
    if (!layout || layout->magic != kWallMagic || !Hc || !Wc) return AVX_ERR_INVALID;
    *Hc = layout->a.Hc; *Wc = layout->a.Wc;
    return AVX_OK;
}

extern "C" int avx_wall_layout_info(const avx_wall_layout* layout, int* mode, int* staged, int* piece_px, size_t* lds_bytes) {
    if (!layout || layout->magic != kWallMagic) return AVX_ERR_INVALID;
    if (mode) *mode = layout->mode;
    if (staged) *staged = layout->stage;
    if (piece_px) *piece_px = layout->a.cw;
    if (lds_bytes) *lds_bytes = layout->lds;
    return AVX_OK;
}

extern "C" int avx_wall_compose_u8(avx_ctx* ctx, const avx_wall_layout* layout, const uint8_t* const* src, size_t src_frame_stride, int n_frames,
                                   uint8_t* canvas, size_t canvas_frame_stride, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, layout && layout->magic == kWallMagic, "avx_wall_compose_u8: layout is NULL or destroyed");
    AVX_REQUIRE(ctx, layout->ctx == ctx, "avx_wall_compose_u8: the layout belongs to another context");
    AVX_REQUIRE(ctx, src && canvas, "avx_wall_compose_u8: NULL pointer");
    AVX_REQUIRE(ctx, n_frames >= 0 && n_frames <= AVX_EW_MAX_FRAMES, "avx_wall_compose_u8: n_frames %d (0..%d)", n_frames, (int)AVX_EW_MAX_FRAMES);
    WallArgs a = layout->a;
    const size_t sframe = (size_t)a.H * a.W * 3, cframe = (size_t)a.Hc * a.Wc * 3;
    AVX_REQUIRE(ctx, src_frame_stride >= sframe && canvas_frame_stride >= cframe,
                "avx_wall_compose_u8: frame strides %zu / %zu are smaller than a frame (%zu / %zu)", src_frame_stride, canvas_frame_stride, sframe, cframe);
    AVX_REQUIRE(ctx, src_frame_stride < ((size_t)1 << 40) && canvas_frame_stride < ((size_t)1 << 40), "avx_wall_compose_u8: frame strides too large");
    const int nf = n_frames > 0 ? n_frames : 1;
    const uintptr_t c0 = (uintptr_t)canvas, c1 = c0 + (size_t)(nf - 1) * canvas_frame_stride + cframe;
    WallSrcs p{};
    for (int i = 0; i < a.n; ++i) {
        AVX_REQUIRE(ctx, src[i], "avx_wall_compose_u8: source %d is NULL", i);
        const uintptr_t s0 = (uintptr_t)src[i], s1 = s0 + (size_t)(nf - 1) * src_frame_stride + sframe;
        AVX_REQUIRE(ctx, s1 <= c0 || c1 <= s0, "avx_wall_compose_u8: source %d overlaps the canvas", i);
        p.p[i] = src[i];
    }
    if (n_frames == 0) return AVX_OK;
    a.src_stride = src_frame_stride; a.canvas_stride = canvas_frame_stride; a.canvas = canvas;
    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    const dim3 grid((unsigned)((size_t)a.Hc * a.cols * a.nsub), (unsigned)n_frames);
    wall_launch(layout->mode, layout->stage != 0, grid, layout->lds, s, a, p);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
