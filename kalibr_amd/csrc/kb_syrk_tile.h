// LDS image of k_buildp's 64 x 16 Jacobian-row tile during the 4x4x4 SYRK, as plain integer arithmetic (host and
// device), so the bank test includes the very function the kernel uses.
//
// Element (row, col) sits at double col * 66 + row: the tile is stored by columns, 66 doubles apart (16 * 66 = 1056
// of the 64 * 17 = 1088 doubles the launch layout allots to a view wave).  With the LDS rules of gfx950 for 8-byte
// accesses (ds_write_b64: four 16-lane groups over 32 banks of 4 bytes; ds_read_b64: two 32-lane groups over 64
// banks) both accesses of the SYRK are conflict-free, and each needs one address register and immediate offsets:
//   store of column q, lane = row:  the 64 lanes write 64 consecutive doubles;
//   operand read, lane = 16 mrow + mcol -> (r0 + mrow, mcol), r0 a multiple of 4:  a 32-lane group holds two
//     consecutive rows of 16 columns, bank pair (2 mcol + r0 + mrow) mod 32 as 66 = 2 mod 32: all 32 distinct.
// (The row-major tile at a 17-double row stride serves the store, but row 1 of a read group starts 34 banks in and
// wraps onto row 0's first pair: 2-way.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KB_TILE_HD __host__ __device__
#else
#define KB_TILE_HD
#endif

namespace kb_tile {

constexpr int kRows = 64, kCols = 16;
constexpr int kColStride = 66;  // doubles between columns: >= kRows, and = 2 mod 32

// double index of tile element (row, col), 0 <= row < 64, 0 <= col < 16
KB_TILE_HD constexpr int idx(int row, int col) { return col * kColStride + row; }

// the two operand reads of pair p (rows 8p .. 8p + 7) by lane: quad 0 / 1 = rows 8p + mrow / 8p + 4 + mrow, column
// mcol (lane = 16 mrow + mcol: the 16x16x4 A-operand layout); the other SYRK operands are lane rotations of these
KB_TILE_HD constexpr int read_idx(int p, int quad, int lane) { return idx(8 * p + 4 * quad + (lane >> 4), lane & 15); }

// the store of column q by lane: row = lane
KB_TILE_HD constexpr int store_idx(int lane, int q) { return idx(lane, q); }

// the kernel addresses pair p's reads as pair 0's plus 8 p doubles (an immediate offset)
static_assert(read_idx(5, 1, 37) == read_idx(0, 1, 37) + 8 * 5 && read_idx(0, 1, 9) == read_idx(0, 0, 9) + 4, "");
static_assert(kColStride >= kRows && kColStride % 32 == 2 && kCols * kColStride <= 64 * 17, "fits the 64 x 17 tile");

}  // namespace kb_tile
