// csrc/gallery_px.h -- what a labelled contact sheet's tile is to its kernels, shared by gallery.hip (avx_gallery_compose_u8: one
// sheet of mixed tiles) and wall.hip (avx_wall_compose_u8: a batch of sheets of equal tiles) so that both compile one copy: the
// tile descriptor, the resized sample of a tile (resize_common.h's statements, chosen by the tile's mode), _to_uint8, and the
// host's choice of resize mode and construction of the axis tables.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "label_common.h"
#include "resize_common.h"

namespace {

constexpr float kHalfOutline = 1.5f;  // _label_strip: outline thickness 3 ...
constexpr float kHalfText = 0.5f;     // ... and text thickness 1, halved as avx_draw_label_u8 halves them
enum { M_COPY = 0, M_AREA_FAST = 1, M_AREA = 2, M_LINEAR = 3 };

// A tile as the kernel reads it: the caller's descriptor plus what the entry point derived from it.  Axis tables are word
// offsets into the table section of the upload (INTER_AREA: start[d], cnt[d], alpha[d][m]; INTER_LINEAR: ofs[d], f[d]).
struct GalTile {
    const void* src;
    int f32, mode;
    int H, W, h, w;
    int isx, isy;          // M_AREA_FAST: the integer ratio
    int seg_off, nseg;
    int ly0;               // first row the label visits: the strip grown by the outline's reach, clipped to the tile
    int xo, yo, xm, ym;    // x / y tables: offset, and maxcnt (area) or dmax (linear)
};

__device__ __forceinline__ AxisArea area_axis(const uint32_t* tabs, int o, int d, int m) {
    return AxisArea{(int*)(tabs + o), (int*)(tabs + o + d), (float*)(tabs + o + 2 * d), m};
}
__device__ __forceinline__ AxisLin lin_axis(const uint32_t* tabs, int o, int d, int dmax) { return AxisLin{(int*)(tabs + o), (float*)(tabs + o + d), dmax}; }

// the resized sample (x, y) of a tile's channel c, before the uint8 conversion: T = source type.  MODE: the tile's mode where a
// launch knows it (wall.hip instantiates per mode), or -1 to read it from the descriptor.
template <typename T, int MODE = -1>
__device__ __forceinline__ float tile_sample(const GalTile& t, const uint32_t* tabs, int c, int x, int y) {
    const T* src = (const T*)t.src;
    const int mode = MODE < 0 ? t.mode : MODE;
    if (mode == M_COPY) return (float)src[((size_t)y * t.W + x) * 3 + c];
    if (mode == M_AREA_FAST) {
        T v;
        const int area = t.isx * t.isy;
        const float scale = 1.f / area;
        AVX_AREA_FAST(T, &v, src, t.W, 3, c, x, y, t.isx, t.isy, area, scale);
        return (float)v;
    }
    if (mode == M_AREA) {
        T v;
        put_area(&v, area_sum(src, t.W, 3, c, x, y, area_axis(tabs, t.xo, t.w, t.xm), area_axis(tabs, t.yo, t.h, t.ym)));
        return (float)v;
    }
    const AxisLin ax = lin_axis(tabs, t.xo, t.w, t.xm), ay = lin_axis(tabs, t.yo, t.h, t.ym);
    if (sizeof(T) == 1) {
        uint8_t out8;  // (not `v`: the macro's own locals would shadow it)
        AVX_LINEAR_U8(out8, (const uint8_t*)src, t.H, t.W, 3, c, x, y, ax, ay);
        return (float)out8;
    }
    return linear_f32_px((const float*)src, t.H, t.W, 3, c, x, y, ax, ay);
}

// _to_uint8 of a float tile: clip to [0, 1] (NaN -> 0), * 255 + 0.5 in float32, truncate
__device__ __forceinline__ uint8_t to_u8(float v) {
    const float cl = v > 0.f ? (v < 1.f ? v : 1.f) : 0.f;
    return (uint8_t)(cl * 255.f + 0.5f);
}

// first row of a tile-plus-strip image that its label visits: avx_draw_label_u8's region, the box grown by the outline's reach
inline int gal_label_row0(int h) {
    const int grow = (int)(kHalfOutline + 2.f);
    return h - grow < 0 ? 0 : h - grow;
}

// ---- host: resize mode per tile (avx_resize_hwc's choice) and one table per distinct (kind, source, destination) axis ----
struct GalTables {
    std::vector<uint32_t> tabs;
    struct Seen { int kind, s, d, off, m; };
    std::vector<Seen> seen;

    void axis(int kind, int ssize, int dsize, int* off, int* m) {
        for (const Seen& e : seen)
            if (e.kind == kind && e.s == ssize && e.d == dsize) { *off = e.off; *m = e.m; return; }
        const int o = (int)tabs.size();
        auto put = [&](const void* p, size_t words) { tabs.resize(tabs.size() + words); memcpy(tabs.data() + tabs.size() - words, p, words * 4); };
        if (kind == M_AREA) {
            std::vector<int> sv, cv; std::vector<float> av; int mc = 1;
            host_area(ssize, dsize, sv, cv, av, mc);
            put(sv.data(), sv.size()); put(cv.data(), cv.size()); put(av.data(), av.size());
            *m = mc;
        } else {
            HostLin hl = host_lin(ssize, dsize);
            put(hl.ofs.data(), hl.ofs.size()); put(hl.f.data(), hl.f.size());
            *m = hl.dmax;
        }
        *off = o;
        seen.push_back({kind, ssize, dsize, o, *m});
    }

    // sets g.mode (and isx / isy, or the table offsets) from g.H, g.W, g.h, g.w
    void place(GalTile& g) {
        if (g.H == g.h && g.W == g.w) { g.mode = M_COPY; return; }
        if (g.w > g.W || g.h > g.H) g.mode = M_LINEAR;  // cv::resize: INTER_AREA when enlarging is INTER_LINEAR
        else {
            const double sx = (double)g.W / g.w, sy = (double)g.H / g.h;
            const int isx = (int)std::lrint(sx), isy = (int)std::lrint(sy);
            if (std::fabs(sx - isx) < DBL_EPSILON && std::fabs(sy - isy) < DBL_EPSILON) { g.mode = M_AREA_FAST; g.isx = isx; g.isy = isy; return; }
            g.mode = M_AREA;
        }
        axis(g.mode, g.W, g.w, &g.xo, &g.xm);
        axis(g.mode, g.H, g.h, &g.yo, &g.ym);
    }
};

}  // namespace
