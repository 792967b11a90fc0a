// Host driver for csrc/scaldpc_rec_trim.h (tests/test_rec_trim.py):
//   rec_trim_main mark M N ROWDEGS... -- COLS...   -> marked=K mark=0101... cols=C,C,...   (rec_mark_const_last; C = -1: not marked; on the graph whose
//                                                      row r has the next ROWDEGS[r] entries of COLS as its columns)
//   rec_trim_main word BOUND MARK                   -> word=W flag=0|1 bound=B col=C (rec_desc_word of a row's mark, 0 or 1 + column, and what the kernels read back)
// The CSC mirror is built as the library builds it: edges grouped by column, ascending CSR position.
#include "../sca-ldpc_amd/csrc/scaldpc_rec_trim.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
    using namespace scaldpc;
    if (argc == 4 && !strcmp(argv[1], "word")) {
        const int w = rec_desc_word(atoi(argv[2]), atoi(argv[3]));
        printf("word=%d flag=%d bound=%d col=%d\n", w, (w & REC_CONST_LAST) ? 1 : 0, rec_desc_bound(w), rec_desc_col(w));
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "mark")) {
        const int m = atoi(argv[2]), n = atoi(argv[3]);
        if (m < 0 || n < 0 || argc < 4 + m + 1 || strcmp(argv[4 + m], "--")) {
            fprintf(stderr, "rec_trim_main mark: expected M row degrees, then --\n");
            return 2;
        }
        std::vector<int> row_ptr((size_t)m + 1, 0);
        for (int r = 0; r < m; r++) row_ptr[r + 1] = row_ptr[r] + atoi(argv[4 + r]);
        const int nnz = row_ptr[m];
        if (argc != 4 + m + 1 + nnz) {
            fprintf(stderr, "rec_trim_main mark: %d column ids expected\n", nnz);
            return 2;
        }
        std::vector<int> col_idx((size_t)nnz), col_ptr((size_t)n + 1, 0), csc_edge((size_t)nnz);
        for (int e = 0; e < nnz; e++) {
            col_idx[e] = atoi(argv[4 + m + 1 + e]);
            if (col_idx[e] < 0 || col_idx[e] >= n) {
                fprintf(stderr, "rec_trim_main mark: column %d out of range\n", col_idx[e]);
                return 2;
            }
            col_ptr[col_idx[e] + 1]++;
        }
        for (int j = 0; j < n; j++) col_ptr[j + 1] += col_ptr[j];
        std::vector<int> cursor(col_ptr.begin(), col_ptr.end() - 1);
        for (int e = 0; e < nnz; e++) csc_edge[cursor[col_idx[e]]++] = e;
        std::vector<int> mark((size_t)m + 1, 7);  // (one byte beyond: must stay as it is)
        const long k = rec_mark_const_last(m, n, row_ptr.data(), col_ptr.data(), csc_edge.data(), mark.data());
        if (mark[m] != 7) {
            fprintf(stderr, "rec_trim_main mark: wrote beyond row %d\n", m);
            return 3;
        }
        printf("marked=%ld mark=", k);
        for (int r = 0; r < m; r++) putchar(mark[r] ? '1' : '0');
        if (m == 0) putchar('-');
        printf(" cols=");
        for (int r = 0; r < m; r++) printf("%d,", mark[r] - 1);
        if (m == 0) putchar('-');
        putchar('\n');
        return 0;
    }
    fprintf(stderr, "usage: rec_trim_main mark M N ROWDEGS... -- COLS... | word BOUND MARK\n");
    return 2;
}
