// Host driver for csrc/scaldpc_rec_pack.h (tests/test_rec_pack.py):
//   rec_pack_main fit M MAXDEG          -> fit=0|1                       (rec_rows_fit: may the record form take the graph?)
//   rec_pack_main pack ROW K            -> word=W row=R index=I          (rec_pack_row and the two extractors)
//   rec_pack_main limits                -> row_bits=.. max_rows=.. max_row_deg=.. rec2_bytes_max=..
#include "../sca-ldpc_amd/csrc/scaldpc_rec_pack.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    using namespace scaldpc;
    if (argc == 4 && !strcmp(argv[1], "fit")) {
        printf("fit=%d\n", rec_rows_fit(atol(argv[2]), atoi(argv[3])) ? 1 : 0);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "pack")) {
        const int w = rec_pack_row(atoi(argv[2]), atoi(argv[3]));
        printf("word=%u row=%d index=%d\n", (unsigned)w, rec_row_of(w), rec_index_of(w));
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        // the variable pass adds (rows * 256) bytes to a lane offset of at most 252 in 32 bits
        printf("row_bits=%d max_rows=%d max_row_deg=%d rec2_bytes_max=%llu\n", REC_ROW_BITS, REC_MAX_ROWS, REC_MAX_ROW_DEG,
               (unsigned long long)REC_MAX_ROWS * 256ull + 252ull);
        return 0;
    }
    fprintf(stderr, "usage: rec_pack_main fit M MAXDEG | pack ROW K | limits\n");
    return 2;
}
