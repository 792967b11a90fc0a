// Walks the sparse-gate rules of csrc/scaldpc_bp_sched.h on the host (tests/test_settle_sparse.py builds this with the
// address and undefined-behaviour sanitizers).  Scenarios come on stdin, one per line, whitespace-separated integers:
//
//   gates  first_test last_test max_iter start -> per iteration 2 .. max_iter `it check_writes check_gates var_writes var_gates`
//                                            (the variable pass of an iteration >= last_test is the closing pass or is not
//                                            enqueued: 0 0)
//   mode   knob settle identity_block     -> the `settle_sparse` mode in force
//   start  min_frozen_at first_test       -> the start the next call gates from (0 = the first test)
#include "../sca-ldpc_amd/csrc/scaldpc_bp_sched.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace scaldpc;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "gates") {
            int ft, lt, max_iter, start;
            if (!(in >> ft >> lt >> max_iter >> start) || max_iter < 1) return 1;
            for (int it = 2; it <= max_iter; it++) {
                const bool var = it < lt;
                printf("it %d %d %d %d %d\n", it, settle_check_mark(it, ft, lt) != 0, settle_sparse_check_gate(it, ft, lt, start),
                       var ? settle_var_mark(it, ft, lt) != 0 : 0, var ? settle_sparse_var_gate(it, ft, lt, start) : 0);
            }
        } else if (cmd == "start") {
            int at, ft;
            if (!(in >> at >> ft)) return 1;
            printf("start %d\n", settle_sparse_next_start(at, ft));
        } else if (cmd == "mode") {
            int knob, settle, ident;
            if (!(in >> knob >> settle >> ident)) return 1;
            printf("mode %d\n", settle_sparse_mode(knob, settle, ident != 0));
        } else {
            fprintf(stderr, "bad scenario: %s\n", line.c_str());
            return 1;
        }
    }
    return 0;
}
