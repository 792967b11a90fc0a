// Walks rec_var_slices of csrc/scaldpc_bp_sched.h on the host (tests/test_rec_slices.py builds this with the address and
// undefined-behaviour sanitizers): which blocks of the column records a record-form variable pass launches.  Cases come on
// stdin, one per line, whitespace-separated integers:
//
//   slices nb  maxd[0] .. maxd[nb-1]  blk[0] .. blk[nb]  var_reversed light write_out G max_col_deg
//       -> `slices narrow0 narrow_n narrow_deg narrow_grid wide0 wide_n wide_grid xmap`
//
// The two arrays are heap blocks of exactly nb and nb + 1 ints: a read past the bucket table is a sanitizer report.
#include "../sca-ldpc_amd/csrc/scaldpc_bp_sched.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace scaldpc;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        int nb = 0;
        bool ok = cmd == "slices" && (in >> nb) && nb >= 0 && nb <= 64;
        std::vector<int> maxd((size_t)(ok ? nb : 0)), blk((size_t)(ok ? nb + 1 : 0));
        for (int &x : maxd) ok = ok && (in >> x);
        for (int &x : blk) ok = ok && (in >> x);
        int rev = 0, light = 0, wo = 0, G = 0, maxcol = 0;
        ok = ok && (in >> rev >> light >> wo >> G >> maxcol);
        if (!ok) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 1;
        }
        const RecVarSlices r = rec_var_slices(nb, maxd.data(), blk.data(), rev != 0, light != 0, wo != 0, G, maxcol);
        printf("slices %d %d %d %d %d %d %d %d\n", r.narrow0, r.narrow_n, r.narrow_deg, r.narrow_grid, r.wide0, r.wide_n, r.wide_grid,
               r.xmap ? 1 : 0);
    }
    return 0;
}
