// Walks the lane-offset rule of csrc/scaldpc_bp_sched.h on the host (tests/test_phase_schedule.py builds this with the
// address and undefined-behaviour sanitizers).  Scenarios come on stdin, one per line, whitespace-separated integers:
//
//   phase  chain horizon max_iter          -> `phase 0|1`: does a group with these chain bits (re-)establish the offset
//   level  groups full_last horizon max_iter -> a fixed-iteration level of `groups` tile groups on two lanes (the last one
//                                              full or not): per group `group chain phase`, chain from chain_bits
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
        if (cmd == "phase") {
            int chain, horizon, max_iter;
            if (!(in >> chain >> horizon >> max_iter)) return 1;
            printf("phase %d\n", phase_reestablished(chain, horizon, max_iter) ? 1 : 0);
        } else if (cmd == "level") {
            int groups, full_last, horizon, max_iter;
            if (!(in >> groups >> full_last >> horizon >> max_iter) || groups < 1) return 1;
            const PollState ps{};
            const RemRing ring{};
            bool open = false;
            for (int g = 0; g < groups; g++) {
                const bool full = g + 1 < groups || full_last != 0;
                const bool next_full = g + 1 < groups && (g + 2 < groups || full_last != 0);
                const int chain = chain_bits(false, true, full, g == 0, next_full, open, 0, max_iter, ps, ring);
                open = (chain & 2) != 0;
                printf("group %d %d\n", chain, phase_reestablished(chain, horizon, max_iter) ? 1 : 0);
            }
        } else {
            fprintf(stderr, "bad scenario: %s\n", line.c_str());
            return 1;
        }
    }
    return 0;
}
