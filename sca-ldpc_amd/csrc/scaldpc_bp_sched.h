// The decisions of the early-exit tile scheduler (decode_level / iterate_tiles in scaldpc_bp.hip), and the counters
// scaldpc_bp_last_schedule reports about them.  Every function here is a pure function of integers: which iterations the
// host polls at, when a tile group hands its stragglers one level down, when it stops at the hand-over point UNSEEN, when
// such groups are chained lane to lane, and which row of "still running" counters a group takes.
// Plain C++, no HIP: tests/bp_sched_main.cc walks these functions with a host compiler under the address and
// undefined-behaviour sanitizers, and tests/test_bp_schedule.py holds them to tests/sched_model.py, a restatement of the
// same rules in Python.
#pragma once

#include <cstdint>

namespace scaldpc {

constexpr int SCHED_TW = 64;          // codewords per tile (the kernels' TW)
constexpr int SCHED_MAX_LANES = 4;    // stream lanes of a tile group
constexpr int SCHED_MAX_LEVELS = 3;   // compaction levels below the call's own arrays
constexpr int REM_SLOTS = 512;        // most rows of "still running" counters a handle keeps

// What the groups of one call learn from each other about polling (a poll drains the queue: the GPU idles
// while the host turns around, ~4 % of a group's time on the config-5 sweep):
//   hint   poll points before this iteration saw no codeword finish in earlier groups: skip them
//   streak consecutive groups that handed a small remainder (<= 1/8) to the compact pass at `defer_after`:
//          after two of them the next groups stop there WITHOUT polling (their stragglers are found from the
//          done masks afterwards, as always), with a real poll every 16th group to keep the assumption honest.
//          A group stopped on a wrong guess only sends more codewords to the compact pass, which decodes
//          them from their inputs: results cannot change.
//   since_poll  groups stopped unseen since the last real hand-over poll
constexpr int SPEC_PERIOD = 16;  // (64 and 4096 measured the same to 0.5 % on the config-5 sweep: the polls are not where its time goes)
constexpr int POLL_EVERY = 4;
struct PollState {
    int hint = 1, streak = 0, since_poll = 0;
};
// Is iteration `it` a poll point of an early-exit tile group?  Every POLL_EVERY-th iteration, the first and the hand-over
// point, from the hint on.  (Decided before anything of the iteration is enqueued: these are the host's own sync points.)
inline bool poll_point(int it, int defer_after, const PollState &ps)
{
    return (it % POLL_EVERY == 0 || it == 1 || it == defer_after) && it >= ps.hint;
}
// Does a group stop at the hand-over point `defer_after` UNSEEN, as the last groups did?
inline bool stops_unseen(int defer_after, int max_iter, const PollState &ps)
{
    return defer_after > 0 && 2 * defer_after < max_iter && ps.streak >= 2 && ps.since_poll < SPEC_PERIOD - 1 &&
           poll_point(defer_after, defer_after, ps);
}
// ... and does it get there without the host: no poll point before it is live?  (decode_level chains such groups)
inline bool runs_unseen(int defer_after, int max_iter, const PollState &ps)
{
    if (!stops_unseen(defer_after, max_iter, ps)) return false;
    for (int it = 1; it < defer_after; it++)
        if (poll_point(it, defer_after, ps)) return false;
    return true;
}
// a group that stopped unseen: one more since the last real poll
inline void note_unseen(PollState &ps) { ps.since_poll++; }

// stream lanes of a group of g tiles under the `split` knob: at most one per tile, at most SCHED_MAX_LANES
inline int lanes_of(int split, int g)
{
    const int nl = split < g ? split : g;
    return nl < 1 ? 1 : nl > SCHED_MAX_LANES ? SCHED_MAX_LANES : nl;
}
// a group of g tiles dealt to nl lanes: lane k takes the gs[k] tiles from t0[k] on, the first g % nl lanes one more
inline void deal_tiles(int g, int nl, int *gs, int *t0)
{
    for (int k = 0, t = 0; k < nl; k++) {
        gs[k] = g / nl + (k < g % nl ? 1 : 0);
        t0[k] = t;
        t += gs[k];
    }
}

// The hand-over point of compaction level lvl (0 = none: the level runs every group to its end).  compact_after < 0 = the
// default.
inline int defer_after_of(bool early, int lvl, int compact_after, int max_iter)
{
    int defer_after = 0;
    if (early && lvl < SCHED_MAX_LEVELS) {
        defer_after = 4;  // measured on the config-5 sweep: 4-5 best (177k trials/s), 8: 156k, 12: 136k
        if (compact_after >= 0) defer_after = compact_after;
        if (max_iter <= 2 * defer_after) defer_after = 0;  // nothing to gain
    }
    return defer_after;
}

// What the host does after it has read `left` = codewords of the group still running after iteration `it`, at a poll
// point that is not the group's last iteration.  g = tiles of the group, real = its codewords, el_lim = codewords the
// row-parallel kernels take (0 = none).
enum PollVerdict { POLL_DONE = 0, POLL_HAND_OVER = 1, POLL_GO_ON = 2 };
inline PollVerdict after_poll(PollState &ps, int it, int defer_after, int max_iter, int left, int real, int g, int el_lim)
{
    if (left == 0) return POLL_DONE;
    if (left >= real) ps.hint = ps.hint > it + 1 ? ps.hint : it + 1;
    // from `defer_after` on, any poll point may hand the stragglers over, provided the
    // restart (it iterations redone) is cheap next to what is still ahead
    // ... and the stragglers really get cheaper: fewer tiles, or few enough for the
    // row-parallel kernels
    const bool shrinks = (left + SCHED_TW - 1) / SCHED_TW < g || left <= el_lim;
    if (defer_after > 0 && it >= defer_after && 2 * it < max_iter && 2 * left <= real && shrinks) {
        ps.streak = (it == defer_after && 8 * left <= real) ? ps.streak + 1 : 0;
        ps.since_poll = 0;
        return POLL_HAND_OVER;
    }
    if (it >= defer_after) ps.streak = 0;
    return POLL_GO_ON;
}

// The ring of "still running" counter rows: every early-exit tile group of a call takes the next row; row 0 belongs to
// the row-parallel and small-call paths.  A call starts with slot = rows ("nothing zeroed yet"), and a taker that finds
// the ring used up clears ALL rows and starts again at row 1.
inline int ring_rows_wanted(int T, int G)
{
    const int gg = G > 1 ? G : 1;
    const int groups = (T + gg - 1) / gg;
    const int want = 2 * groups + 8;  // one per tile group of the call, the compact levels' groups (fewer tiles each) included, + row 0
    return want < REM_SLOTS ? want : REM_SLOTS;
}
struct RemRing {
    int slot = 0, rows = 0;
};
// the row the next group takes; *clears = the whole ring is zeroed first
inline int ring_take(RemRing &r, bool *clears)
{
    *clears = r.slot >= r.rows;
    if (*clears) r.slot = 1;  // (row 0 is the other paths')
    return r.slot++;
}

// chain bits of a group (iterate_tiles): bit 0 = it CONTINUES the lanes of the group before it, bit 1 = it leaves them
// un-joined for the group after it.
//   early       the call runs with early exit
//   lanes2      the level's groups run on more than one lane, without an initialisation pass
//   full        this group has the level's full tile count; next_full: there is a next group and it has, too
//   first       this is the level's first group
//   lanes_open  the group before it left its lanes un-joined
//   ps          the poll state BEFORE this group; ring: the counter rows BEFORE this group takes its own
inline int chain_bits(bool early, bool lanes2, bool full, bool first, bool next_full, bool lanes_open, int defer_after,
                      int max_iter, const PollState &ps, const RemRing &ring)
{
    int chain = 0;
    if (!lanes2 || !full) return 0;
    if (!early) {
        // fixed-iteration runs chain consecutive groups of the same geometry lane by lane: no host interaction
        if (!first) chain |= 1;     // (the group before it was a full one too)
        if (next_full) chain |= 2;  // ... and so is the next
    } else if (runs_unseen(defer_after, max_iter, ps)) {
        // a group that will stop at the hand-over point UNSEEN and polls nowhere before enqueues its launches without
        // ever synchronising
        PollState nxt = ps;
        note_unseen(nxt);
        if (lanes_open) chain |= 1;  // (the group before it left them un-joined)
        // (the next group takes the next row of "still running" counters: no chaining across the wrap, which clears them all)
        if (next_full && runs_unseen(defer_after, max_iter, nxt) && ring.slot + 2 < ring.rows) chain |= 2;
    }
    return chain;
}

// Does a group (re-)establish the one-kernel offset between neighbouring lanes -- lane k + 1 waits, once, for lane k's first
// check pass -- when it starts (iterate_tiles)?  A group that continues nobody's lanes has to: its lanes start together.
// A chained group finds whatever offset its predecessor's lanes ended with.
//   chain     the group's chain bits (chain_bits)
//   horizon   the settle horizon in force (0 = none): the group enqueues iterations 1 ... horizon and its closing sequence
//   max_iter  the call's iteration count
// The rule in force: always.  Carrying the offset over in chained groups was measured twice: with groups of 50 iterations
// (3.7 ms; profiles/r04/ab_chain_unseen_groups.log: + 0.5 % on the config-5 sweep, - 2 % on the fixed-iteration bench) and
// with groups cut to a settle horizon of 12 (0.6 ms; profiles/minsum_settle_passes/README.md: 0.03 ms of 10.0 on HQC-128,
// 0.13 of 19.7 on HQC-192, both inside the run-to-run spread; the tanh rule unchanged).  Neither the horizon nor the
// iteration count moves the verdict, so neither enters the rule; they stay inputs, for whoever measures it next.
// tests/test_phase_schedule.py holds the rule to a restatement, tests/phase_sched_main.cc walks it under the sanitizers.
inline bool phase_reestablished(int chain, int horizon, int max_iter)
{
    (void)chain;
    (void)horizon;
    (void)max_iter;
    return true;
}

// Counters of the schedule a call ran (scaldpc_bp_last_schedule), host integers only.
enum SchedWord {
    SCHED_GROUPS = 0,         // [4] tile groups run at compaction level 0 .. 3
    SCHED_HANDED = 4,         // [3] codewords handed down FROM level 0 .. 2
    SCHED_POLLS = 7,          // host polls of the tile loop (a synchronise plus a read of a counter)
    SCHED_UNSEEN = 8,         // groups that stopped at the hand-over point unseen
    SCHED_CONTINUED = 9,      // early-exit groups that continued their predecessor's lanes (chain bit 0)
    SCHED_LEFT_OPEN = 10,     // early-exit groups left un-joined for their successor (chain bit 1)
    SCHED_FIXED_CHAINED = 11, // fixed-iteration groups that continued their predecessor's lanes
    SCHED_CLEARS = 12,        // clears of the counter ring after the call's first
    SCHED_OPEN_AT_CLEAR = 13, // clears that found the lanes of the group before un-joined (must stay 0)
    SCHED_RING_ROWS = 14,     // rows of the counter ring during the call
    SCHED_EL_POLLS = 15,      // host polls of the row-parallel loop
    SCHED_RING_TAKES = 16,    // rows of the ring handed out
    SCHED_WORDS = 17
};
struct SchedCounters {
    int64_t w[SCHED_WORDS] = {};
    bool ring_cleared = false;  // the call's first clear has happened
    void reset() { *this = SchedCounters{}; }
    void note_take(bool clears, bool lanes_open)
    {
        w[SCHED_RING_TAKES]++;
        if (!clears) return;
        if (ring_cleared) w[SCHED_CLEARS]++;
        if (lanes_open) w[SCHED_OPEN_AT_CLEAR]++;
        ring_cleared = true;
    }
    void note_group(int lvl, bool early, int chain)
    {
        w[SCHED_GROUPS + lvl]++;
        if (early) {
            if (chain & 1) w[SCHED_CONTINUED]++;
            if (chain & 2) w[SCHED_LEFT_OPEN]++;
        } else if (chain & 1)
            w[SCHED_FIXED_CHAINED]++;
    }
};

// ---------------------------------------------------------------------------
// Settled codewords (fixed-iteration calls on the record-form kernels; the device side is `Settle`,
// scaldpc_bp_kernels.h).  Test t (t >= SETTLE_FIRST) has two halves -- variable pass t - 1 compares the sign masks it
// stores with the ones it overwrites, check pass t its records and arg-min bytes -- and a tile in which neither saw a
// difference is frozen at t.  tests/settle_sched_main.cc walks the rules below under the sanitizers and
// tests/test_settle_schedule.py holds them to a restatement in Python.
// ---------------------------------------------------------------------------
constexpr int SETTLE_FIRST = 3;  // check pass 2 is the bootstrap pass: it has nothing to compare with
// The first test a call can track.  Tracking is valid only across passes with the same alpha: alpha_from = the first
// iteration from which alpha_for() is one float to the call's end (1 with a given alpha; with the 1 - 2^-it schedule the
// iteration at which the float becomes 1.0f).  Test t needs check passes t - 1 and t to share it.
inline int settle_first_test(int alpha_from)
{
    const int t = alpha_from + 1;
    return t < SETTLE_FIRST ? SETTLE_FIRST : t;
}
// What the passes of iteration `it` are told: `done` = the latest test completed before the pass on its stream (0 = none),
// `mark` = the test it is a half of (0 = the pass is not tracked).  last_test = the last test of the group: its last
// check pass that is not the bootstrap one, i.e. max_iter, or the horizon.
inline int settle_check_done(int it, int first_test) { return it - 1 >= first_test ? it - 1 : 0; }
inline int settle_check_mark(int it, int first_test, int last_test) { return it >= first_test && it <= last_test ? it : 0; }
inline int settle_var_done(int it, int first_test, int last_test) { return it >= first_test && it <= last_test ? it : 0; }
inline int settle_var_mark(int it, int first_test, int last_test) { return settle_check_mark(it + 1, first_test, last_test); }
// The frozen-at number of a tile after a group whose tests ran from first_test to last_test: latest = the maximum of its
// words = the last test in which something of it changed (0 = none did).  0 = the tile never froze.
inline int settle_frozen_at(int latest, int first_test, int last_test)
{
    if (last_test < first_test || latest >= last_test) return 0;
    return latest + 1 > first_test ? latest + 1 : first_test;
}
// Can a group stop at horizon K -- iterations 1 ... K, then the closing sequence (the last variable pass and the final
// test, as iteration max_iter)?  Test K must exist, and something must be left out.  (The closing variable pass takes
// the place of variable pass K: on a tile frozen by K that one would have returned at once, and any other tile is decoded
// again.)
inline bool settle_horizon_usable(int K, int first_test, int max_iter) { return K >= first_test && K + 1 < max_iter; }
// Which passes a group with horizon K (0 = none) enqueues: iteration `it` at all; its check pass (where the iteration has
// one anyway); its variable pass.
inline bool settle_enqueued(int it, int K, int max_iter) { return !(K && it > K && it < max_iter); }
inline bool settle_has_check(int it, int K, int max_iter) { return !(K && it == max_iter); }
inline bool settle_has_var(int it, int K) { return !(K && it == K); }
// launches of one lane that a group with horizon K does not enqueue: variable pass K, the pairs of K + 1 ... max_iter - 1
// and the check pass of max_iter
inline int settle_launches_saved(int K, int max_iter) { return 2 * (max_iter - K); }
// The horizon the NEXT call runs with, learned from the last one (0 = none: the call runs with device-side skipping alone
// and is learned from again).  tiles = tiles of the call, frozen = those with a frozen-at number (re-run ones with the
// number their re-run found), max_frozen_at = the largest of them, rerun = tiles the call had to decode again because
// they were not frozen by its horizon.
inline int settle_next_horizon(int tiles, int frozen, int max_frozen_at, int rerun, int max_iter)
{
    if (tiles <= 0 || max_frozen_at <= 0) return 0;
    if (8 * rerun > tiles) return 0;  // more than 1/8 re-run: the horizon costs more than it saves
    const int K = max_frozen_at + 2;
    if (8 * frozen < 7 * tiles) return 0;  // at least 7/8 of the tiles froze by K
    if (2 * K >= max_iter) return 0;
    return K;
}

// The `settle` knob in force: 0 / 1 / 2 as given; -1 (the default) = 2 on a graph [Hin | I], where every row has an edge
// into a column of degree 1 and the message state is bounded, and 0 on any other graph, which has no reason to settle and
// would only pay for the tracking.
inline int settle_mode(int knob, bool identity_block) { return knob >= 0 ? knob : identity_block ? 2 : 0; }

// The sparse gate of a tracked level (knob settle_sparse; the device side: `Settle`'s row_flag / col_flag tables).  The
// tracked passes write flags -- a pass with a mark, settle_check_mark / settle_var_mark -- and a pass GATES, i.e. its waves
// return for nodes none of whose inputs changed, only when the pass before it on the same tiles wrote flags and it is
// tracked itself: with start = first_test, check passes first_test + 1 ... last_test (variable pass t - 1 stamped the columns that ran; at
// first_test every column ran, so gating that pass would skip nothing), variable passes first_test ... last_test - 1
// (check pass t stamped its rows).  The bootstrap pass, passes under a moving alpha (before first_test), the closing pass
// and early-exit calls (never tracked) do not gate.  tests/settle_sparse_main.cc walks these under the sanitizers,
// tests/test_settle_sparse.py holds them to tests/settle_sparse_ref.py.
// `start` (>= first_test) = the variable pass from which the call gates at all; its check passes gate one later.  Every
// tracked pass writes its flags whether it gates or not, so any start from first_test on finds them.
inline int settle_sparse_check_gate(int it, int first_test, int last_test, int start)
{
    const int from = start > first_test ? start : first_test;
    return settle_check_mark(it, first_test, last_test) != 0 && settle_var_mark(it - 1, first_test, last_test) != 0 && it > from;
}
inline int settle_sparse_var_gate(int it, int first_test, int last_test, int start)
{
    const int from = start > first_test ? start : first_test;
    return settle_var_mark(it, first_test, last_test) != 0 && settle_check_mark(it, first_test, last_test) != 0 && it >= from;
}
// The start the NEXT call gates from, learned like the horizon (settle_next_horizon) from the last call: the gate's two
// dependent loads stand in front of a wave's own, which a dense pass -- one in which nearly every node still has a changed
// input -- pays for and gets nothing back (variable passes 3 and 4 of the HQC-128 bench: + 8 ... 10 us of 53 per launch,
// profiles/settle_sparse/README.md).  Nodes go quiet shortly before their tile freezes: on the bench batch, whose first
// tiles freeze at test 8, variable pass 5 still runs 70 % of its columns and saves 3 us, variable pass 6 runs 3 ... 5 %.
// So the next call gates from SETTLE_SPARSE_LEAD passes before the smallest frozen-at number of the last one.
//   min_frozen_at  the smallest frozen-at number > 0 among the last call's tiles, 0 = no tile froze or nothing learned yet
// 0 = gate from the first test on: a call that learns, and a call after one in which nothing froze -- there the tiles
// cycle with part of their nodes quiet all the way, which the gate skips from the start.
constexpr int SETTLE_SPARSE_LEAD = 2;
inline int settle_sparse_next_start(int min_frozen_at, int first_test)
{
    if (min_frozen_at <= 0) return 0;
    const int s = min_frozen_at - SETTLE_SPARSE_LEAD;
    return s > first_test ? s : first_test;
}
// (Both functions lean on the bootstrap check pass coming before the first test: it is the first record-form check pass of
// a group, iteration 2 at the latest, it carries no mark and stamps no row, and first_test >= SETTLE_FIRST = 3 -- so the
// check pass of a gating variable pass is never the bootstrap one.  iterate_tiles passes gate = 0 with a bootstrap pass
// all the same.)
// The `settle_sparse` knob in force on a tracked level (settle = the settle mode in force, > 0): 0 / 1 as given; -1 (the
// default) = on where the settle mode is 2 AND the graph is [Hin | I] -- the graphs on which `settle` turns itself on.  On
// a graph where nothing freezes the gate only costs (+ 18 % on a tracked call, profiles/settle_sparse/README.md), so a
// caller who forces `settle` there gets the gate only by asking for it.
inline int settle_sparse_mode(int knob, int settle, bool identity_block)
{
    return settle <= 0 ? 0 : knob >= 0 ? knob : (settle >= 2 && identity_block) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// The record-form variable pass (launch_var, scaldpc_bp.hip): which blocks of the column records a pass runs.  The
// records are laid out bucket by bucket -- bucket b = blocks [blk[b], blk[b + 1]), unroll bound maxd[b], ascending;
// var_reversed: the whole order mirrored, heaviest first -- and a slice is a first block and a count.
//   slim   a pass without output after iteration 1 (light && !write_out) leaves the degree-1 bucket out.  A column of
//          degree <= 1 always sends its prior; iteration 1 has written that into the message array and the record check
//          pass never overwrites it (its sign mask is the bootstrap check pass's, and stays true), so such a pass has
//          nothing to do there (the identity block of an HQC graph: 4000 of 21669 column waves per tile).  Not when the
//          bucket is all there is.
//   wide   the blocks of the (32, 64] bucket (minsum_rec = 2, rec_form; the last bucket, no any-degree one behind it) get
//          a launch of their own -- k_var<64, ..>, the kernel that already keeps 64 edges in registers, in its record mode
//          (RecWide) -- so that the exact-degree code of the columns up to 32 stays what it is; the narrow launch runs over
//          the other buckets' blocks, compiled for the widest of THEM (narrow_deg).
//   xmap   XCD-aware tile placement where the launch's G tiles divide the 8 XCDs (fetch 38.0 -> 29.5 MB per launch,
//          profiles/r03/ab_rec_xmap.log): grid.x is then rounded up to a multiple of 8.
// tests/rec_slices_main.cc walks this under the sanitizers, tests/test_rec_slices.py holds it to a restatement in Python.
// ---------------------------------------------------------------------------
struct RecVarSlices {
    int narrow0 = 0, narrow_n = 0, narrow_deg = 0, narrow_grid = 0;  // first block, blocks, the degree that picks the cap, grid.x
    int wide0 = 0, wide_n = 0, wide_grid = 0;
    bool xmap = false;
};
inline RecVarSlices rec_var_slices(int nb, const int *maxd, const int *blk, bool var_reversed, bool light, bool write_out, int G,
                                   int max_col_deg)
{
    RecVarSlices r;
    const int nblk = blk[nb];
    const int n1 = (nb > 0 && maxd[0] == 1) ? blk[1] : 0;
    const bool slim = light && !write_out && n1 > 0 && n1 < nblk;
    r.wide_n = (nb > 0 && maxd[nb - 1] > 32) ? nblk - blk[nb - 1] : 0;
    r.narrow_deg = r.wide_n ? (nb > 1 ? maxd[nb - 2] : 0) : max_col_deg;
    r.narrow_n = (slim ? nblk - n1 : nblk) - r.wide_n;
    // (heaviest first: the wide blocks lead the records and the degree-1 bucket ends them)
    r.narrow0 = var_reversed ? r.wide_n : (slim ? n1 : 0);
    r.wide0 = var_reversed ? 0 : nblk - r.wide_n;
    r.xmap = G == 2 || G == 4 || G == 8;
    r.narrow_grid = r.xmap ? (r.narrow_n + 7) / 8 * 8 : r.narrow_n;
    r.wide_grid = r.xmap ? (r.wide_n + 7) / 8 * 8 : r.wide_n;
    return r;
}

// Poll points of the row-parallel loop: `ip` = the iteration whose verdict the host may look at.  Poll densely where
// convergence is likely, sparsely afterwards.
inline bool el_poll_point(int ip) { return (ip >= 3 && ip <= 6) || (ip > 6 && ip <= 16 && ip % 2 == 0) || (ip > 16 && ip % 16 == 0); }

}  // namespace scaldpc
