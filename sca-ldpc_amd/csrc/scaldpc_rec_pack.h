// Row words of the min-sum record form's variable pass (d_var_rows / d_csc_row): the row of an edge and, in the high
// bits, the edge's index IN that row -- what the variable pass compares the row's arg-min byte against.  24 bits of row,
// 8 bits of index (rows of the record form have at most 64 edges).  The row bound also keeps the byte distance between
// a row's first and second magnitudes (rows * 256) in the 32-bit lane offset the variable pass adds it to.  rec_form()
// refuses a graph that does not fit (message form) instead of letting the index run into the row.
// And the layout of a tile's block of records (d_rec): where a row's records and its arg-min bytes lie.
// Plain C++, no HIP: tests/rec_pack_main.cc and tests/rec_layout_main.cc build it with a host compiler
// (tests/test_rec_pack.py, tests/test_rec_layout.py).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define SCALDPC_REC_HD __host__ __device__
#else
#define SCALDPC_REC_HD
#endif

namespace scaldpc {

constexpr int REC_ROW_BITS = 24;
constexpr int REC_MAX_ROWS = (1 << REC_ROW_BITS) - 1;      // most rows a packed graph has: (rows + 1) * 256 B < 2^32
constexpr int REC_MAX_ROW_DEG = 1 << (32 - REC_ROW_BITS);  // in-row indices 0 ... 255

// can every row of an m-row graph whose widest row has max_row_deg edges be packed?
SCALDPC_REC_HD inline bool rec_rows_fit(long m, int max_row_deg) { return m <= (long)REC_MAX_ROWS && max_row_deg <= REC_MAX_ROW_DEG; }
SCALDPC_REC_HD inline int rec_pack_row(int row, int k_in_row) { return (int)((unsigned)row | ((unsigned)k_in_row << REC_ROW_BITS)); }
SCALDPC_REC_HD inline int rec_row_of(int word) { return (int)((unsigned)word & ((1u << REC_ROW_BITS) - 1u)); }
SCALDPC_REC_HD inline int rec_index_of(int word) { return (int)((unsigned)word >> REC_ROW_BITS); }

// One tile's block of d_rec for a graph of m rows, offsets in FLOATS from the block's start:
//     m1  [row][64] float   first magnitudes (* alpha, the row's parity in the sign bit), 256 B per row
//     m2  [row][64] float   second magnitudes, m rows behind the first (rec_m2_off; in bytes the 32-bit lane offset
//                           the variable pass adds: (rows + 1) * 256 B < 2^32, REC_MAX_ROWS)
//     arg [row][64] u8      behind both
// padded to whole 256-B lines.
constexpr int REC_TW = 64;  // codewords per tile (the kernels' TW)
SCALDPC_REC_HD inline size_t rec_row_off(long row) { return (size_t)row * REC_TW; }  // a row's first magnitudes
SCALDPC_REC_HD inline size_t rec_m2_off(long m) { return (size_t)m * REC_TW; }       // from a row's first magnitudes to its second
SCALDPC_REC_HD inline size_t rec_arg_off(long m) { return (size_t)m * (2 * REC_TW); }
SCALDPC_REC_HD inline size_t rec_arg_row_bytes() { return (size_t)REC_TW; }
SCALDPC_REC_HD inline size_t rec_tile_floats(long m) { return ((size_t)m * (2 * REC_TW + REC_TW / 4) + 63) / 64 * 64; }

}  // namespace scaldpc
