// Host-side decisions of the min-sum record form's trimmed passes: which rows end in a CONSTANT edge.
// An edge into a column of degree 1 carries that column's prior in every pass (the column has no other check to hear
// from), so the record check pass need not load it: where it is the row's LAST edge -- the identity block of an HQC
// graph [Hin | I] -- the row's descriptor is marked (REC_CONST_LAST in its fourth word, beside the bucket's unroll bound)
// and k_check_minsum_rec takes the value from the shared priors with one scalar load.  A constant edge elsewhere in a
// row, or a second one before the last, changes nothing: those edges are loaded as ever.
// Plain C++, no HIP: tests/rec_trim_main.cc builds it with a host compiler (tests/test_rec_trim.py).
#pragma once

#include <algorithm>
#include <cstddef>

#include "scaldpc_rec_pack.h"

namespace scaldpc {

// A row descriptor's fourth word: bits 0-6 the bucket's unroll bound (at most 64; 0 = any-degree row, which is never
// marked: the tanh kernel tests the word against 0), bit 30 the mark, bits 7-29 the COLUMN of the marked row's last
// edge -- the check pass reads the prior without a look into col_idx (a 64-B line per row).  A column the field cannot
// hold leaves its row unmarked.
constexpr int REC_CONST_LAST = 1 << 30;
constexpr int REC_CONST_COL_SHIFT = 7, REC_CONST_COL_BITS = 23;
constexpr int REC_CONST_MAX_COL = (1 << REC_CONST_COL_BITS) - 1;
SCALDPC_REC_HD inline int rec_desc_col(int word) { return (word >> REC_CONST_COL_SHIFT) & REC_CONST_MAX_COL; }
SCALDPC_REC_HD inline int rec_desc_bound(int word) { return word & ((1 << REC_CONST_COL_SHIFT) - 1); }

// mark[r] = 1 + that column where row r's last edge (CSR position row_ptr[r + 1] - 1) goes into a column of degree 1, else 0.
// The graph comes as the table builder holds it: CSR row pointers (m + 1) and the CSC mirror (col_ptr: n + 1;
// csc_edge: the CSR position of every edge, grouped by column).  Returns how many rows are marked.
inline long rec_mark_const_last(int m, int n, const int *row_ptr, const int *col_ptr, const int *csc_edge, int *mark)
{
    std::fill(mark, mark + m, 0);
    long marked = 0;
    for (int j = 0; j < n; j++) {
        if (col_ptr[j + 1] - col_ptr[j] != 1) continue;
        const int e = csc_edge[col_ptr[j]];
        // the row that holds CSR position e: the last one that starts at or before it (empty rows share a start)
        const int r = (int)(std::upper_bound(row_ptr, row_ptr + m + 1, e) - row_ptr) - 1;
        if (r < 0 || r >= m || e != row_ptr[r + 1] - 1) continue;
        mark[r] = 1 + j;
        marked++;
    }
    return marked;
}

// a row descriptor's fourth word; mark = rec_mark_const_last's entry of the row
inline int rec_desc_word(int unroll_bound, int mark)
{
    const int col = mark - 1;
    if (unroll_bound <= 0 || unroll_bound >= (1 << REC_CONST_COL_SHIFT) || col < 0 || col > REC_CONST_MAX_COL) return unroll_bound;
    return unroll_bound | REC_CONST_LAST | (col << REC_CONST_COL_SHIFT);
}

}  // namespace scaldpc
