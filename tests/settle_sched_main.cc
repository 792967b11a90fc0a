// Walks the settle rules of csrc/scaldpc_bp_sched.h on the host (tests/test_settle_schedule.py builds this with the address
// and undefined-behaviour sanitizers).  Scenarios come on stdin, one per line, whitespace-separated integers:
//
//   plan   alpha_from max_iter K            -> first_test usable, then per iteration 1 .. max_iter that a group enqueues
//                                              `it check_done check_mark var_done var_mark` (-1 -1 = the pass is not
//                                              enqueued; the last variable pass is never tracked: 0 0), then `saved n`
//   frozen first_test last_test n  then n numbers `latest`     -> the frozen-at number of each
//   calls  max_iter forced first_test tiles ncalls  then per call `tiles` true frozen-at numbers (0 = never)
//                                              a handle's calls one after the other: per call `call K rerun frozen max next`
//   mode   knob identity_block              -> the `settle` mode in force
//   consts                                  -> the header's constants
#include "../sca-ldpc_amd/csrc/scaldpc_bp_sched.h"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace scaldpc;

static int walk_plan(std::istringstream &in)
{
    int alpha_from, max_iter, K;
    if (!(in >> alpha_from >> max_iter >> K) || max_iter < 1 || alpha_from < 1) return 1;
    const int ft = settle_first_test(alpha_from);
    const bool usable = settle_horizon_usable(K, ft, max_iter);
    if (!usable) K = 0;
    const int last_test = K ? K : max_iter;
    printf("plan %d %d\n", ft, usable ? 1 : 0);
    for (int it = 1; it <= max_iter; it++) {
        const bool last = it == max_iter;
        if (!settle_enqueued(it, K, max_iter)) continue;
        const bool check = it >= 2 && settle_has_check(it, K, max_iter);  // (iteration 1 has no record-form check pass)
        const bool boot = it == 2;
        const bool var = settle_has_var(it, K);
        printf("it %d %d %d %d %d\n", it, check ? settle_check_done(it, ft) : -1,
               check ? (boot ? 0 : settle_check_mark(it, ft, last_test)) : -1,
               var ? (last || it < 2 ? 0 : settle_var_done(it, ft, last_test)) : -1,
               var ? (last || it < 2 ? 0 : settle_var_mark(it, ft, last_test)) : -1);
    }
    printf("saved %d\n", K ? settle_launches_saved(K, max_iter) : 0);
    return 0;
}

static int walk_calls(std::istringstream &in)
{
    int max_iter, forced, ft, tiles, ncalls;
    if (!(in >> max_iter >> forced >> ft >> tiles >> ncalls) || tiles < 1 || ncalls < 0) return 1;
    int next = 0;
    std::vector<int> at((size_t)tiles);
    for (int c = 0; c < ncalls; c++) {
        for (int &x : at)
            if (!(in >> x)) return 1;
        int K = forced > 0 ? forced : next;
        if (!settle_horizon_usable(K, ft, max_iter)) K = 0;
        int rerun = 0, frozen = 0, mx = 0;
        for (int x : at) {
            // what the device reports for a tile whose true number is x: tests run from ft to K (or max_iter)
            const int seen = x >= ft && x <= (K ? K : max_iter) ? x : 0;
            if (K && !seen) rerun++;  // decoded again with all iterations: the true number
            const int fin = K && !seen ? (x >= ft && x <= max_iter ? x : 0) : seen;
            frozen += fin > 0;
            mx = std::max(mx, fin);
        }
        next = settle_next_horizon(tiles, frozen, mx, rerun, max_iter);
        printf("call %d %d %d %d %d\n", K, rerun, frozen, mx, next);
    }
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        int rc = 0;
        if (cmd == "plan") {
            rc = walk_plan(in);
        } else if (cmd == "calls") {
            rc = walk_calls(in);
        } else if (cmd == "frozen") {
            int ft, lt, n;
            if (!(in >> ft >> lt >> n) || n < 0) return 1;
            printf("frozen");
            for (int i = 0; i < n; i++) {
                int latest;
                if (!(in >> latest)) return 1;
                printf(" %d", settle_frozen_at(latest, ft, lt));
            }
            printf("\n");
        } else if (cmd == "consts") {
            printf("consts %d\n", SETTLE_FIRST);
        } else if (cmd == "mode") {
            int knob, ident;
            if (!(in >> knob >> ident)) return 1;
            printf("mode %d\n", settle_mode(knob, ident != 0));
        } else {
            rc = 1;
        }
        if (rc) {
            fprintf(stderr, "bad scenario: %s\n", line.c_str());
            return 1;
        }
    }
    return 0;
}
