// csrc/mst_convt_lines.h -- where the bytes of a wave-tile's skip row and output row sit in the wave's LDS area (csrc/mst_mfma.hip,
// k_mst_convt2x2_16_ln), as functions the kernel and the host (avx_mst_convt_lines_map, tests/test_mst_convt_lines.py) share.
//
// A wave-tile's output row is one run of 64 pixels x C bytes (C = 64: 32 channels, C = 128: 64), the same run in `skip` and in `out`.  Counted in
// 16-byte chunks a pixel has cpp = C / 16 of them (4 or 8) and the run is cpp pieces of 64 chunks = 1 KB; chunk g of the run is pixel g / cpp,
// channels 8 (g % cpp) ... + 7.
//
// Skip row in: one global_load_lds_dwordx4 per piece; the instruction puts lane l's 16 bytes in slot l of the piece, which leaves the chunk the
// lane FETCHES free: lane l of piece i fetches chunk convt_ln_skip_chunk(cpp, i, l) of the piece (a bijection, so the access is the whole 1 KB).
// The B operand of tap dx, step s in lane (p, h) is the chunk of pixel 2 p + dx, channels h C/4 + 8 s.  ds_read_b128 serves 16 lanes a cycle
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, the same + 32), and the 16 slots it wants then must differ mod 16 (the 256-byte bank row).  Such a
// group holds four lanes with consecutive p out of each of four pieces, so: slot = 16 U + 4 V + (p & 3), where (U, V) enumerate the 16 chunks a
// lane quartet's pixels offer for (dx, channel chunk c) and V carries the piece index: V = (i ^ 3 hi ^ dx) & 3 at cpp = 4 (16 pixels a piece,
// hi = the upper half of them; the groups' pieces come with (i, hi) = (0,0) (1,1) (2,1) (3,0) or (0,1) (1,0) (2,0) (3,1)), V = (i & 3) ^ (2 (c & 1) + dx)
// at cpp = 8 (8 pixels a piece; the groups' pieces are {0, 3, 5, 6} and {1, 2, 4, 7}).
//
// Output row out: lane (p, h) writes, per tap dx and 32-channel tile t, chunks (2 p + dx) cpp + 4 t + 2 h + b, b = 0, 1 (ds_write_b128: 8 consecutive
// lanes a cycle, 128-byte bank row), and the wave reads the run back as chunk 64 i + l in lane l (ds_read_b128, groups as above) for one 1 KB store
// per piece.  Chunk k of piece i sits in slot k ^ (k >> 3) (cpp = 4) or k ^ (((k >> 4) & 3) | (i & 1) << 2) (cpp = 8): the eight writers of a cycle
// -- pixels two apart -- and the sixteen readers of a cycle each cover their bank row once.
#pragma once

__host__ __device__ constexpr int convt_ln_skip_slot(int cpp, int i, int k) {  // slot (0 .. 63) of chunk k of piece i
    if (cpp == 4) {
        const int ql = k >> 2, c = k & 3, hi = ql >> 3, pl = (ql >> 1) & 3, dx = ql & 1;
        return 16 * c + 4 * ((i ^ (3 * hi) ^ dx) & 3) + pl;
    }
    const int ql = k >> 3, c = k & 7, pl = ql >> 1, dx = ql & 1;
    return 16 * (c >> 1) + 4 * ((i & 3) ^ (2 * (c & 1) + dx)) + pl;
}
__host__ __device__ constexpr int convt_ln_skip_chunk(int cpp, int i, int l) {  // the inverse: the chunk of piece i that lane l fetches
    const int u = l >> 4, v = ((l >> 2) ^ i) & 3, pl = l & 3;
    if (cpp == 4) {
        const int hi = v >> 1, dx = (v & 1) ^ hi;
        return 4 * (8 * hi + 2 * pl + dx) + u;
    }
    return 8 * (2 * pl + (v & 1)) + 2 * u + (v >> 1);
}
// byte in the row area of the operand of lane (p, h), tap dx, step s
__host__ __device__ constexpr int convt_ln_operand_byte(int cpp, int p, int h, int dx, int s) {
    const int g = (2 * p + dx) * cpp + h * (cpp / 2) + s;
    return 1024 * (g >> 6) + 16 * convt_ln_skip_slot(cpp, g >> 6, g & 63);
}
// byte in the row area of chunk g of the output run
__host__ __device__ constexpr int convt_ln_out_byte(int cpp, int g) {
    const int i = g >> 6, k = g & 63;
    return 1024 * i + 16 * (k ^ (cpp == 4 ? k >> 3 : ((k >> 4) & 3) | (i & 1) << 2));
}
