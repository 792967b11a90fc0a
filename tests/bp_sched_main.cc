// Walks the scheduler decisions of csrc/scaldpc_bp_sched.h on the host (tests/test_bp_schedule.py builds this with the
// address and undefined-behaviour sanitizers).  Scenarios come on stdin, one per line, whitespace-separated integers:
//
//   level  early lvl T G batch split compact_after max_iter el_lim ring_slot ring_rows cleared L  then per group L numbers
//          one compaction level of T tiles / `batch` codewords in groups of G tiles; per group the codewords still
//          running after iteration 1 .. L (after later iterations: the last of them).  Prints per group
//              group <i> chain row cleared open_before kind it npolls polls...
//          (kind 0 = a poll found nobody running, 1 = handed over at a poll, 2 = stopped unseen, 3 = ran all iterations)
//          then `counters <SCHED_WORDS numbers>` and `ring <slot> <cleared>`.
//   pred   hint streak since_poll defer_after max_iter      -> stops runs, then the poll points up to max_iter
//   hand   early lvl compact_after max_iter                  -> the level's hand-over point
//   deal   g split                                           -> lanes, then tiles and first tile of every lane
//   rows   T G                                               -> rows of the ring a call of that shape asks for
//   consts                                                   -> the header's constants
//   elpoll max_ip                                            -> the row-parallel loop's poll points up to max_ip
#include "../sca-ldpc_amd/csrc/scaldpc_bp_sched.h"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace scaldpc;

static int walk_level(std::istringstream &in)
{
    int early, lvl, T, G, batch, split, compact_after, max_iter, el_lim, cleared, L;
    RemRing ring;
    if (!(in >> early >> lvl >> T >> G >> batch >> split >> compact_after >> max_iter >> el_lim >> ring.slot >> ring.rows >> cleared >> L))
        return 1;
    if (lvl < 0 || lvl > SCHED_MAX_LEVELS || T < 1 || G < 1 || L < 1 || max_iter < 1 || ring.rows < 2) return 1;
    const int Gl = std::min(G, T);
    const int groups = (T + Gl - 1) / Gl;
    std::vector<int> left((size_t)groups * L);
    for (int &x : left)
        if (!(in >> x)) return 1;
    const int defer_after = defer_after_of(early != 0, lvl, compact_after, max_iter);
    const bool lanes2 = lanes_of(split, Gl) > 1;
    SchedCounters cnt;
    cnt.ring_cleared = cleared != 0;
    cnt.w[SCHED_RING_ROWS] = ring.rows;
    PollState ps;
    bool lanes_open = false;
    int gi = 0;
    for (int g0 = 0; g0 < T; g0 += Gl, gi++) {
        const int g = std::min(Gl, T - g0);
        const int real = std::min(batch - g0 * SCHED_TW, g * SCHED_TW);
        const bool next_full = g0 + Gl < T && std::min(Gl, T - (g0 + Gl)) == Gl;
        const int chain = chain_bits(early != 0, lanes2, g == Gl, g0 == 0, next_full, lanes_open, defer_after, max_iter, ps, ring);
        cnt.note_group(lvl, early != 0, chain);
        const bool open_before = lanes_open;
        bool clears = false;
        int row = 0;
        if (early) {
            row = ring_take(ring, &clears);
            cnt.note_take(clears, lanes_open);
        }
        int kind = 3, stop = max_iter;
        std::vector<int> polls;
        for (int it = 1; it <= max_iter; it++) {
            const bool last = it == max_iter;
            if (!early || last || !poll_point(it, defer_after, ps)) continue;
            if (it == defer_after && stops_unseen(defer_after, max_iter, ps)) {
                note_unseen(ps);
                cnt.w[SCHED_UNSEEN]++;
                kind = 2;
                stop = it;
                break;
            }
            polls.push_back(it);
            cnt.w[SCHED_POLLS]++;
            const PollVerdict v =
                after_poll(ps, it, defer_after, max_iter, left[(size_t)gi * L + std::min(it, L) - 1], real, g, el_lim);
            if (v != POLL_GO_ON) {
                kind = v == POLL_DONE ? 0 : 1;
                stop = it;
                break;
            }
        }
        // a group that polled joined its lanes there; one that never met the host leaves them as its chain bit says
        lanes_open = (chain & 2) != 0;
        if (!polls.empty() && (chain & 2)) return 2;  // (a group left open for its successor never polls)
        printf("group %d %d %d %d %d %d %d %zu", gi, chain, row, clears ? 1 : 0, open_before ? 1 : 0, kind, stop, polls.size());
        for (int p : polls) printf(" %d", p);
        printf("\n");
    }
    printf("counters");
    for (int i = 0; i < SCHED_WORDS; i++) printf(" %lld", (long long)cnt.w[i]);
    printf("\nring %d %d\n", ring.slot, cnt.ring_cleared ? 1 : 0);
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "level") {
            if (const int rc = walk_level(in)) {
                fprintf(stderr, "bad level scenario (%d): %s\n", rc, line.c_str());
                return 1;
            }
        } else if (cmd == "pred") {
            PollState ps;
            int defer_after, max_iter;
            if (!(in >> ps.hint >> ps.streak >> ps.since_poll >> defer_after >> max_iter)) return 1;
            printf("pred %d %d", stops_unseen(defer_after, max_iter, ps) ? 1 : 0, runs_unseen(defer_after, max_iter, ps) ? 1 : 0);
            for (int it = 1; it <= max_iter; it++)
                if (poll_point(it, defer_after, ps)) printf(" %d", it);
            printf("\n");
        } else if (cmd == "hand") {
            int early, lvl, compact_after, max_iter;
            if (!(in >> early >> lvl >> compact_after >> max_iter)) return 1;
            printf("hand %d\n", defer_after_of(early != 0, lvl, compact_after, max_iter));
        } else if (cmd == "deal") {
            int g, split, gs[SCHED_MAX_LANES], t0[SCHED_MAX_LANES];
            if (!(in >> g >> split) || g < 1) return 1;
            const int nl = lanes_of(split, g);
            deal_tiles(g, nl, gs, t0);
            printf("deal %d", nl);
            for (int k = 0; k < nl; k++) printf(" %d %d", gs[k], t0[k]);
            printf("\n");
        } else if (cmd == "rows") {
            int T, G;
            if (!(in >> T >> G)) return 1;
            printf("rows %d\n", ring_rows_wanted(T, G));
        } else if (cmd == "consts") {
            printf("consts %d %d %d %d %d %d %d\n", SCHED_TW, SCHED_MAX_LANES, SCHED_MAX_LEVELS, REM_SLOTS, SPEC_PERIOD, POLL_EVERY,
                   (int)SCHED_WORDS);
        } else if (cmd == "elpoll") {
            int max_ip;
            if (!(in >> max_ip)) return 1;
            printf("elpoll");
            for (int ip = 0; ip <= max_ip; ip++)
                if (el_poll_point(ip)) printf(" %d", ip);
            printf("\n");
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
