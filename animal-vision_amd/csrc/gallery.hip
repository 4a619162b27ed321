// csrc/gallery.hip -- gallery_grid.build_labeled_grid (reference: gallery_grid.py:8-106) in one launch: the labelled contact
// sheet of the `gallery` command (main.py:203-278).
//
// The reference resizes every tile to tile_height (cv2.resize INTER_AREA, aspect kept), converts it to uint8, stacks a 40-row
// black strip under it, draws the label on that with cv2.putText (black outline at thickness 3, white text at 1), pads it to
// the largest tile with bg and places it in a row-major grid on a bg canvas.  Here the host lays all of that out
// (gallery_grid.py) and one thread per canvas pixel decides which of four things the pixel is -- background, a resized tile
// sample, strip black, or one of those under label coverage -- so each canvas byte is written once and no tile is
// materialised.  The arithmetic is the existing kernels': resize_common.h (avx_resize_hwc's INTER_AREA / INTER_LINEAR
// samples) and label_common.h (avx_draw_label_u8's coverage and blend).
#include <vector>

#include "avx_internal.h"
#include "gallery_px.h"

namespace {

constexpr int kGT = 256;
constexpr int kSlot = 10;            // avx_ws::consts slot of the uploaded descriptors, segments and tables

struct GalArgs {
    const GalTile* tiles; const float* seg; const uint32_t* tabs;
    int n, cols, cell_h, cell_w, pad, strip_h;
    int Hc, Wc;
    uint8_t bg[3];
    uint8_t* canvas;
};

__global__ __launch_bounds__(kGT) void k_gallery_compose(GalArgs a) {
    const unsigned npx = (unsigned)a.Hc * (unsigned)a.Wc;  // the host checks Hc * Wc < 2^31
    for (unsigned p = blockIdx.x * kGT + threadIdx.x; p < npx; p += gridDim.x * kGT) {
        const int y = (int)(p / (unsigned)a.Wc), x = (int)(p - (unsigned)y * (unsigned)a.Wc);
        uint8_t o[3] = {a.bg[0], a.bg[1], a.bg[2]};
        const int xx = x - a.pad, yy = y - a.pad;
        if (xx >= 0 && yy >= 0) {
            const int col = xx / a.cell_w, row = yy / a.cell_h;
            const int tx = xx - col * a.cell_w, ty = yy - row * a.cell_h;
            const int i = row * a.cols + col;
            if (col < a.cols && i < a.n) {
                const GalTile& t = a.tiles[i];
                if (tx < t.w && ty < t.h + a.strip_h) {
                    o[0] = o[1] = o[2] = 0;  // strip black
                    if (ty < t.h) {
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            o[c] = t.f32 ? to_u8(tile_sample<float>(t, a.tabs, c, tx, ty)) : (uint8_t)tile_sample<uint8_t>(t, a.tabs, c, tx, ty);
                    }
                    if (ty >= t.ly0) {  // the label, as k_draw_label draws it on the tile-plus-strip image
                        const float d = label_dist(a.seg + 6 * (size_t)t.seg_off, t.nseg, (float)tx, (float)ty);
                        const float co = cover(d, kHalfOutline), ct = cover(d, kHalfText);
                        const bool inbox = ty >= t.h;  // the box is the strip: (0, h, w - 1, h + strip_h - 1)
#pragma unroll
                        for (int c = 0; c < 3; ++c) o[c] = label_blend(o[c], inbox, co, ct);
                    }
                }
            }
        }
        uint8_t* D = a.canvas + (size_t)p * 3;
        D[0] = o[0]; D[1] = o[1]; D[2] = o[2];
    }
}

}  // namespace

extern "C" int avx_gallery_compose_u8(avx_ctx* ctx, const avx_gallery_tile* tiles_host, int n_tiles, const float* segments_host, int n_segments,
                                      int strip_h, int pad, int cols, const int bg_rgb[3], uint8_t* canvas_hwc, int Hc, int Wc, void* stream) {
    if (!ctx) return AVX_ERR_INVALID;
    AVX_REQUIRE(ctx, tiles_host && n_tiles >= 1 && n_tiles <= 4096, "avx_gallery_compose_u8: need 1..4096 tiles (got %d)", n_tiles);
    AVX_REQUIRE(ctx, canvas_hwc && Hc > 0 && Wc > 0 && (size_t)Hc * Wc < ((size_t)1 << 31), "avx_gallery_compose_u8: bad canvas (%d x %d)", Hc, Wc);
    AVX_REQUIRE(ctx, cols >= 1 && pad >= 0 && strip_h >= 0 && strip_h <= 4096, "avx_gallery_compose_u8: bad layout (cols %d, pad %d, strip %d)", cols, pad, strip_h);
    AVX_REQUIRE(ctx, bg_rgb, "avx_gallery_compose_u8: bg is NULL");
    for (int c = 0; c < 3; ++c) AVX_REQUIRE(ctx, bg_rgb[c] >= 0 && bg_rgb[c] <= 255, "avx_gallery_compose_u8: bg[%d] = %d is not in 0..255", c, bg_rgb[c]);
    AVX_REQUIRE(ctx, n_segments >= 0 && n_segments <= (1 << 20) && (n_segments == 0 || segments_host), "avx_gallery_compose_u8: bad segment table");

    // descriptors; cell = largest tile plus strip, plus pad (build_labeled_grid's padding)
    std::vector<GalTile> td(n_tiles);
    int max_h = 0, max_w = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const avx_gallery_tile& t = tiles_host[i];
        AVX_REQUIRE(ctx, t.src && t.src != canvas_hwc, "avx_gallery_compose_u8: tile %d: no source, or the source is the canvas", i);
        AVX_REQUIRE(ctx, t.dtype == 0 || t.dtype == 2, "avx_gallery_compose_u8: tile %d: dtype %d (0 float32 or 2 uint8)", i, t.dtype);
        AVX_REQUIRE(ctx, t.H > 0 && t.W > 0 && t.h > 0 && t.w > 0 && t.h <= (1 << 16) && t.w <= (1 << 16),
                    "avx_gallery_compose_u8: tile %d: bad size %d x %d -> %d x %d", i, t.H, t.W, t.h, t.w);
        AVX_REQUIRE(ctx, t.seg_offset >= 0 && t.seg_count >= 0 && (int64_t)t.seg_offset + t.seg_count <= n_segments,
                    "avx_gallery_compose_u8: tile %d: segments [%d, %d + %d) past the table of %d", i, t.seg_offset, t.seg_offset, t.seg_count, n_segments);
        GalTile& g = td[i];
        g = GalTile{};
        g.src = t.src; g.f32 = t.dtype == 0;
        g.H = t.H; g.W = t.W; g.h = t.h; g.w = t.w;
        g.seg_off = t.seg_offset; g.nseg = t.seg_count;
        g.ly0 = gal_label_row0(t.h);
        max_h = t.h + strip_h > max_h ? t.h + strip_h : max_h;
        max_w = t.w > max_w ? t.w : max_w;
    }
    const int64_t cell_h = (int64_t)max_h + pad, cell_w = (int64_t)max_w + pad;
    const int64_t used_cols = cols < n_tiles ? cols : n_tiles, rows = (n_tiles + cols - 1) / cols;
    AVX_REQUIRE(ctx, rows * cell_h + pad <= Hc && used_cols * cell_w + pad <= Wc,
                "avx_gallery_compose_u8: the %lld x %lld grid of %lld x %lld cells does not fit the %d x %d canvas", (long long)rows, (long long)used_cols,
                (long long)cell_h, (long long)cell_w, Hc, Wc);

    // resize mode per tile (avx_resize_hwc's choice) and one table per distinct (kind, source, destination) axis
    GalTables gt;
    for (GalTile& g : td) gt.place(g);
    const std::vector<uint32_t>& tabs = gt.tabs;

    // one upload: [tiles][segments][tables], 256-byte aligned sections; re-sent only when its bytes change (avx_const_upload)
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_tiles = up(sizeof(GalTile) * n_tiles), b_seg = up(sizeof(float) * 6 * (size_t)n_segments), b_tab = up(4 * tabs.size());
    std::vector<uint8_t> blob(b_tiles + b_seg + b_tab + 256, 0);
    memcpy(blob.data(), td.data(), sizeof(GalTile) * n_tiles);
    if (n_segments) memcpy(blob.data() + b_tiles, segments_host, sizeof(float) * 6 * (size_t)n_segments);
    if (!tabs.empty()) memcpy(blob.data() + b_tiles + b_seg, tabs.data(), 4 * tabs.size());

    AVX_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = avx_pick_stream(ctx, stream);
    avx_ws* ws = avx_workspace(ctx, s);
    if (!ws) return AVX_ERR_NOMEM;
    uint8_t* dev = nullptr;
    const int rc = avx_const_upload(ctx, ws, kSlot, blob.data(), blob.size(), s, (void**)&dev);
    if (rc) return rc;
    GalArgs a{};
    a.tiles = (const GalTile*)dev;
    a.seg = (const float*)(dev + b_tiles);
    a.tabs = (const uint32_t*)(dev + b_tiles + b_seg);
    a.n = n_tiles; a.cols = cols; a.cell_h = (int)cell_h; a.cell_w = (int)cell_w; a.pad = pad; a.strip_h = strip_h;
    a.Hc = Hc; a.Wc = Wc;
    for (int c = 0; c < 3; ++c) a.bg[c] = (uint8_t)bg_rgb[c];
    a.canvas = canvas_hwc;
    const size_t npx = (size_t)Hc * Wc, want = (npx + kGT - 1) / kGT, cap = (size_t)ctx->num_cus * 16;
    hipLaunchKernelGGL(k_gallery_compose, dim3((unsigned)(want < cap ? want : cap)), dim3(kGT), 0, s, a);
    AVX_HIP(ctx, hipGetLastError());
    return AVX_OK;
}
