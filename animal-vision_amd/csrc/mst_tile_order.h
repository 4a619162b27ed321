// csrc/mst_tile_order.h -- which tiles of a (frames x ty x tx) grid a persistent workgroup visits, and in which order.
//
// RASTER (round 2): workgroup w takes tiles w, w + nwg, w + 2 nwg, ... of the raster (frame, row, column).  Workgroups are dealt round-robin
// over the 8 XCDs, so a tile and its right neighbour -- and, the row length being what it is, the tile below -- run on different XCDs, each
// behind its own 4 MiB L2: every halo pixel is fetched past L2 once per tile that touches it.
//
// XCD (round 4): the workgroups with the same blockIdx.x % 8 (the observed dispatch puts them on one XCD; nothing but speed depends on it)
// walk ONE contiguous stretch of the BAND-MAJOR order together.  The band-major order cuts the grid into min(8, tx) bands of tile columns
// and runs through a band frame by frame, row by row, before it enters the next band.  Class g of the workgroups owns the positions
// [T cum(g) / nwg, T cum(g + 1) / nwg) of that order (T tiles, cum(g) workgroups in the classes below g: a bijection by construction, for any
// T and nwg, and balanced to one tile), and its n members take the positions first + m, + n, + 2n, ...: at any moment the n tiles in flight
// on an XCD are n consecutive tiles of a band -- a patch a few rows tall whose upper neighbours left the same L2 a moment ago.  Where tx is
// a multiple of 8 a class's stretch IS a band; otherwise it laps a little into the next band.
//
// Either way the coordinates advance with carries (scalar adds and compares): divisions run when the walk starts and when it crosses into
// another band (at most a few times per workgroup), never per tile: there is no scalar divide, and a division per tile on the vector unit
// (~150 instructions per wave as a 64-bit one) was a fifth of the attention tail's instruction stream.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define AVX_TW_UNI32(v) __builtin_amdgcn_readfirstlane((int)(v))
#else
#define AVX_TW_UNI32(v) ((int)(v))
#endif

enum { AVX_TILE_ORDER_RASTER = 0, AVX_TILE_ORDER_XCD = 1 };
constexpr int kTileXcds = 8;

// All counts are 32-bit (the launchers refuse grids of 2^31 tiles or more): the walk lives in scalar registers, which the tile kernels are short of too.
struct TileWalk {
    int xi, yi, b;     // this tile's column, row and frame
    bool live;         // false: past this workgroup's last tile (the coordinates mean nothing)
    int x1, w;         // this band's last column + 1 and its width
    int dx, dy, db;    // the stride as (columns, rows, frames) of this band
    int tx, ty, nb;    // the grid; its bands
    unsigned per;      // tiles of one tile column over all rows and frames
    unsigned pos, end, step, stop;  // band-major position, this walk's last + 1, stride; first position past this band or the walk, whichever comes first

    // coordinates and carries of band-major position `pos` (< total): the divisions run on the vector unit, their results go back to scalar registers
    __host__ __device__ __forceinline__ void locate() {
        const unsigned qb = (unsigned)tx / (unsigned)nb, rb = (unsigned)tx % (unsigned)nb;  // the first rb bands are qb + 1 columns wide, the others qb
        const unsigned wide = rb * (qb + 1) * per;
        unsigned bstart, wv, x0v;
        if (pos < wide) {
            const unsigned band = pos / ((qb + 1) * per);
            wv = qb + 1; x0v = band * (qb + 1); bstart = band * (qb + 1) * per;
        } else {
            const unsigned band = (pos - wide) / (qb * per);
            wv = qb; x0v = rb * (qb + 1) + band * qb; bstart = wide + band * qb * per;
        }
        const unsigned idx = pos - bstart, row = idx / wv, srow = step / wv;
        xi = AVX_TW_UNI32(x0v + idx - row * wv); yi = AVX_TW_UNI32(row % (unsigned)ty); b = AVX_TW_UNI32(row / (unsigned)ty);
        dx = AVX_TW_UNI32(step - srow * wv); dy = AVX_TW_UNI32(srow % (unsigned)ty); db = AVX_TW_UNI32(srow / (unsigned)ty);
        w = AVX_TW_UNI32(wv); x1 = AVX_TW_UNI32(x0v + wv);
        const unsigned band_end = (unsigned)AVX_TW_UNI32(bstart + wv * per);
        stop = band_end < end ? band_end : end;
    }
    __host__ __device__ __forceinline__ void init(unsigned wg, unsigned nwg, int frames, int ty_, int tx_, int order) {
        tx = tx_; ty = ty_; per = (unsigned)frames * (unsigned)ty_;
        const unsigned total = per * (unsigned)tx_;
        if (order == AVX_TILE_ORDER_XCD) {
            const unsigned g = wg % kTileXcds, m = wg / kTileXcds, base = nwg / kTileXcds, rem = nwg % kTileXcds;
            const unsigned cum = g * base + (g < rem ? g : rem), n = base + (g < rem ? 1u : 0u);  // workgroups in the classes below g; in class g (>= 1: wg is one)
            nb = tx_ < kTileXcds ? tx_ : kTileXcds;
            pos = (unsigned)AVX_TW_UNI32((unsigned long long)total * cum / nwg) + m;
            end = (unsigned)AVX_TW_UNI32((unsigned long long)total * (cum + n) / nwg);
            step = n;
        } else {
            nb = 1;  // one band: the band-major order is the raster
            pos = wg; end = total; step = nwg;
        }
        live = pos < end;
        stop = 0;  // a walk that never lived stays dead
        if (live) locate();
    }
    __host__ __device__ __forceinline__ void advance() {
        pos += step;  // < 2^32: pos < 2^31 while the walk is live, and a dead walk is advanced a few times at most
        if (pos >= stop) {  // into the next band (rare), or past the end
            live = live && pos < end;
            if (live) locate();
            return;
        }
        xi += dx;
        const int cx = xi >= x1 ? 1 : 0;
        xi -= cx ? w : 0;
        yi += dy + cx;
        const int cy = yi >= ty ? 1 : 0;
        yi -= cy ? ty : 0;
        b += db + cy;
    }
};

// COLUMN (round 10): the marching FeedForward kernel carries the two bottom halo rows of a tile on chip into the tile below, so a workgroup owns one contiguous
// RUN of the column-major order (frame, tile column, tile row) and walks it a tile at a time.  Run r of nwg is the positions [T r / nwg, T (r + 1) / nwg): a
// bijection for any T and nwg, balanced to one tile.  The workgroups of one class (blockIdx.x % 8, see above) own neighbouring runs -- neighbouring tile columns
// meet in one L2 -- and nothing but speed depends on that.  A SEGMENT starts at a walk's first tile and at the top of every column: there the rows above are not
// on chip.  The divisions run when the walk starts; a step is an increment and two carries.
struct ColumnWalk {
    int xi, yi, b;      // this tile's column, row and frame
    bool live;          // false: past this workgroup's last tile (the coordinates mean nothing)
    bool seg;           // this tile starts a segment
    int tx, ty;         // the grid
    unsigned pos, end;  // column-major position, this walk's last + 1

    __host__ __device__ __forceinline__ void init(unsigned wg, unsigned nwg, int frames, int ty_, int tx_) {
        tx = tx_; ty = ty_;
        const unsigned total = (unsigned)frames * (unsigned)ty_ * (unsigned)tx_;
        const unsigned g = wg % kTileXcds, m = wg / kTileXcds, base = nwg / kTileXcds, rem = nwg % kTileXcds;
        const unsigned run = g * base + (g < rem ? g : rem) + m;  // the workgroups in the classes below g, then this one's place in its class
        pos = (unsigned)AVX_TW_UNI32((unsigned long long)total * run / nwg);
        end = (unsigned)AVX_TW_UNI32((unsigned long long)total * (run + 1) / nwg);
        live = pos < end;
        seg = true;
        const unsigned col = pos / (unsigned)ty_;
        yi = AVX_TW_UNI32(pos - col * (unsigned)ty_); xi = AVX_TW_UNI32(col % (unsigned)tx_); b = AVX_TW_UNI32(col / (unsigned)tx_);
    }
    __host__ __device__ __forceinline__ void advance() {
        ++pos;  // < 2^32: pos < 2^31 while the walk is live, and a dead walk is advanced a few times at most
        live = live && pos < end;
        ++yi;
        seg = yi >= ty;
        yi = seg ? 0 : yi;
        xi += seg ? 1 : 0;
        const int cx = xi >= tx ? 1 : 0;
        xi = cx ? 0 : xi;
        b += cx;
    }
};

// COLUMN STEPS (round 11): the marching attention tail carries v rows, a mid row pair and stash rows from the tile above.  At a segment start they are not on chip,
// and the kernel gets them by running an ordinary step on the tile ABOVE (row index yi - 1, which is -1 at the top of a column) with its stores masked: a PRIMING
// step.  This is the ColumnWalk with those steps put in: next() yields the step to run (false: the walk is over), and the walk itself stays a step ahead, so the
// kernel can prefetch the step after the one it works on.
struct ColumnSteps {
    ColumnWalk wk;
    bool primed;     // the last step yielded was the priming step of wk's tile
    int xi, yi, b;   // the step's tile (yi = -1: the tile above the frame's first row)
    bool prime;      // a priming step: nothing is stored

    __host__ __device__ __forceinline__ void init(unsigned wg, unsigned nwg, int frames, int ty_, int tx_) {
        wk.init(wg, nwg, frames, ty_, tx_);
        primed = false;
    }
    __host__ __device__ __forceinline__ bool next() {
        if (!wk.live) return false;
        prime = wk.seg && !primed;
        xi = wk.xi; b = wk.b; yi = wk.yi - (prime ? 1 : 0);
        primed = prime;
        if (!prime) wk.advance();
        return true;
    }
};
