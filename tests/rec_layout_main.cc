// Host driver for the tile-block layout of the min-sum record form in csrc/scaldpc_rec_pack.h (tests/test_rec_layout.py):
//   rec_layout_main layout M  -> tw=.. tile_floats=.. row_floats=.. row_last=.. m2_off=.. arg_off=.. arg_row_bytes=..
//   rec_layout_main limits    -> max_rows=..
// All offsets are in floats from the start of a tile's block unless the name says bytes; m2_off is the distance from a
// row's first magnitudes to its second ones.
#include "../sca-ldpc_amd/csrc/scaldpc_rec_pack.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    using namespace scaldpc;
    if (argc == 3 && !strcmp(argv[1], "layout")) {
        const long m = atol(argv[2]);
        printf("tw=%d tile_floats=%zu row_floats=%zu row_last=%zu m2_off=%zu arg_off=%zu arg_row_bytes=%zu\n", REC_TW, rec_tile_floats(m),
               rec_row_off(1) - rec_row_off(0), rec_row_off(m - 1), rec_m2_off(m), rec_arg_off(m), rec_arg_row_bytes());
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        printf("max_rows=%d\n", REC_MAX_ROWS);
        return 0;
    }
    fprintf(stderr, "usage: rec_layout_main layout M | limits\n");
    return 2;
}
