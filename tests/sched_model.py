"""A model of the early-exit tile scheduler of the binary BP path, restated from DESIGN.md ("Cache-resident tile groups,
two stream lanes", "Early exit and straggler compaction") and the comments of csrc/scaldpc_bp_sched.h -- not a port of
its code: the rules are written here the way the documents state them, and tests/test_bp_schedule.py holds the two to
each other decision for decision (tests/bp_sched_main.cc walks the header's functions).

The rules, in the documents' words:

  * Codewords travel in tiles of 64; a level's tiles are decoded in groups of at most G tiles, all iterations of a group
    back to back, on `lanes` stream lanes (at most 4, at most one per tile).
  * An early-exit group takes the next row of a ring of "still running" counters.  Row 0 is not handed out.  A call's
    first taker clears the ring and gets row 1; a taker that finds all rows used clears the ring again and gets row 1.
  * The host may poll after iteration 1, after every 4th iteration and after the level's hand-over point -- but not
    before `hint`: a poll that found every codeword of its group still running moves the hint past that iteration for
    the groups after it.  The group's last iteration is never polled.
  * A poll that finds nobody running ends the group.  From the hand-over point on, a poll hands the stragglers one
    level down when redoing `it` iterations is cheap (2 it < max_iter), at most half of the group's codewords are left,
    and they fill fewer tiles than the group has (or are few enough for the row-parallel kernels).
  * `streak` counts consecutive groups that handed over AT the hand-over point with at most 1/8 left; any other poll
    from the hand-over point on that does not end the group resets it.  With a streak of two the next groups stop at
    the hand-over point UNSEEN -- no poll; their stragglers are found afterwards from the done masks -- until 15 groups
    in a row have done so: the 16th polls for real.
  * A group that will stop unseen and has no live poll point before the hand-over point never meets the host.  Such a
    group continues the lanes its predecessor left open, and leaves its own open when the next group is a full one
    that will run unseen too -- unless the next group's counter row would come within one row of the ring's end: a
    clear never meets open lanes.
  * Fixed-iteration runs chain every full group to the next full group.
  * Levels 0, 1 and 2 have a hand-over point (`compact_after`, default 4; none if max_iter <= 2 * compact_after);
    level 3 has none.  A level of one tile with at most `el_limit` codewords runs on the row-parallel kernels, which
    poll after iterations 3 .. 6, every second iteration up to 16 and every 16th afterwards, one iteration late.
"""
import math

TW = 64
POLL_EVERY = 4
SPEC_PERIOD = 16
MAX_LEVELS = 3
REM_SLOTS = 512
MAX_LANES = 4


class Poll:
    """What the groups of one level learn from each other."""

    def __init__(self, hint=1, streak=0, since_poll=0):
        self.hint, self.streak, self.since_poll = hint, streak, since_poll

    def copy(self):
        return Poll(self.hint, self.streak, self.since_poll)


def is_poll_point(it, hand, p):
    return (it == 1 or it == hand or it % POLL_EVERY == 0) and it >= p.hint


def stops_unseen(hand, max_iter, p):
    if hand <= 0 or 2 * hand >= max_iter:
        return False
    if p.streak < 2 or p.since_poll > SPEC_PERIOD - 2:
        return False
    return is_poll_point(hand, hand, p)


def runs_unseen(hand, max_iter, p):
    return stops_unseen(hand, max_iter, p) and not any(is_poll_point(it, hand, p) for it in range(1, hand))


def hand_over_point(early, lvl, compact_after, max_iter):
    if not early or lvl >= MAX_LEVELS:
        return 0
    hand = 4 if compact_after < 0 else compact_after
    return 0 if max_iter <= 2 * hand else hand


def ring_rows_wanted(T, G):
    return min(REM_SLOTS, 2 * math.ceil(T / max(1, G)) + 8)


class Ring:
    """The rows of "still running" counters of a handle: `slot` = next free row."""

    def __init__(self, rows, slot=None):
        self.rows = rows
        self.slot = rows if slot is None else slot  # a new call: nothing cleared yet

    def take(self):
        cleared = self.slot >= self.rows
        if cleared:
            self.slot = 1
        row = self.slot
        self.slot += 1
        return row, cleared


def lanes_of(split, g):
    return max(1, min(split, g, MAX_LANES))


def deal(g, nl):
    """Tiles per lane and first tile of each lane."""
    sizes = [g // nl + (1 if k < g % nl else 0) for k in range(nl)]
    return sizes, [sum(sizes[:k]) for k in range(nl)]


def new_counters(ring_rows=0):
    return {"groups": [0, 0, 0, 0], "handed_down": [0, 0, 0], "polls": 0, "unseen": 0, "continued": 0, "left_open": 0,
            "fixed_chained": 0, "clears": 0, "open_at_clear": 0, "ring_rows": ring_rows, "row_parallel_polls": 0,
            "ring_takes": 0}  # fmt: skip


def walk_level(*, early, lvl, T, G, batch, lanes, compact_after, max_iter, el_limit, ring, left_of, counters=None,
               cleared_before=False):
    """One compaction level: T tiles holding `batch` codewords.  left_of(group index, it) = codewords of that group still
    running after iteration it (asked only where the host polls).  Returns the groups' records -- dict(tiles, real, chain,
    row, cleared, open_before, polls, stop = (kind, it)), kind one of "done" (a poll found nobody running), "hand" (a
    poll handed the stragglers down), "unseen" (stopped at the hand-over point without a poll), "end" (ran all
    iterations) -- and whether the ring has been cleared by now."""
    c = counters if counters is not None else new_counters(ring.rows)
    Gl = min(G, T)
    hand = hand_over_point(early, lvl, compact_after, max_iter)
    chaining = lanes_of(lanes, Gl) > 1
    p = Poll()
    out = []
    open_before = False
    starts = list(range(0, T, Gl))
    for gi, g0 in enumerate(starts):
        g = min(Gl, T - g0)
        real = min(batch - g0 * TW, g * TW)
        next_full = gi + 1 < len(starts) and min(Gl, T - starts[gi + 1]) == Gl
        chain = 0
        if chaining and g == Gl:
            if not early:
                chain = (1 if gi > 0 else 0) | (2 if next_full else 0)
            elif runs_unseen(hand, max_iter, p):
                after = p.copy()
                after.since_poll += 1
                if open_before:
                    chain |= 1
                # this group takes row `slot` (or row 1 after a clear), the next one the row behind it
                if next_full and runs_unseen(hand, max_iter, after) and ring.slot + 2 < ring.rows:
                    chain |= 2
        c["groups"][lvl] += 1
        if early:
            c["continued"] += chain & 1
            c["left_open"] += (chain >> 1) & 1
        else:
            c["fixed_chained"] += chain & 1
        rec = {"tiles": g, "real": real, "chain": chain, "row": 0, "cleared": False, "open_before": open_before,
               "polls": [], "stop": ("end", max_iter)}  # fmt: skip
        if early:
            rec["row"], rec["cleared"] = ring.take()
            c["ring_takes"] += 1
            if rec["cleared"]:
                c["clears"] += 1 if cleared_before else 0
                c["open_at_clear"] += 1 if open_before else 0
                cleared_before = True
            for it in range(1, max_iter):  # (the last iteration is never polled)
                if not is_poll_point(it, hand, p):
                    continue
                if it == hand and stops_unseen(hand, max_iter, p):
                    p.since_poll += 1
                    c["unseen"] += 1
                    rec["stop"] = ("unseen", it)
                    break
                left = left_of(gi, it)
                rec["polls"].append(it)
                c["polls"] += 1
                if left == 0:
                    rec["stop"] = ("done", it)
                    break
                if left >= real:
                    p.hint = max(p.hint, it + 1)
                fewer = math.ceil(left / TW) < g or left <= el_limit
                if hand > 0 and it >= hand and 2 * it < max_iter and 2 * left <= real and fewer:
                    p.streak = p.streak + 1 if (it == hand and 8 * left <= real) else 0
                    p.since_poll = 0
                    rec["stop"] = ("hand", it)
                    break
                if it >= hand:
                    p.streak = 0
        open_before = bool(chain & 2)
        out.append(rec)
    return out, cleared_before


def row_parallel_polls(finish, max_iter):
    """Polls of the row-parallel loop on codewords that finish after iteration finish[i] (max_iter + 1: never)."""
    n = 0
    for it in range(1, max_iter):
        ip = it - 1  # the iteration whose verdict the host looks at, one iteration late
        if (3 <= ip <= 6) or (6 < ip <= 16 and ip % 2 == 0) or (ip > 16 and ip % 16 == 0):
            n += 1
            if not any(f > ip for f in finish):
                break
    return n


def predict(iters, converged, *, G, lanes, compact_after, max_iter, el_limit, ring_rows, early=True):
    """The schedule of one call from the oracle's per-codeword results.  G = tiles per group (already cut to the call's
    tile count), ring_rows = rows of the handle's counter ring during the call.
    Returns dict(counters, levels, compacted, row_parallel, sets = [codeword ids of level 0, 1, ...], records)."""
    batch = len(iters)
    finish = [int(iters[i]) if converged[i] else max_iter + 1 for i in range(batch)]  # done after this iteration
    c = new_counters(ring_rows)
    ring = Ring(ring_rows)
    sets, records = [], []
    ids = list(range(batch))
    lvl, row_parallel, cleared = 0, 0, False
    while True:
        sets.append(ids)
        n = len(ids)
        T = math.ceil(n / TW)
        if T == 1 and n <= el_limit:
            row_parallel = n
            if early:
                c["row_parallel_polls"] += row_parallel_polls([finish[i] for i in ids], max_iter)
            records.append([])
            break
        Gl = min(G, T)

        def left_of(gi, it, ids=ids, Gl=Gl):
            return sum(1 for i in ids[gi * Gl * TW:(gi + 1) * Gl * TW] if finish[i] > it)

        recs, cleared = walk_level(early=early, lvl=lvl, T=T, G=G, batch=n, lanes=lanes, compact_after=compact_after,
                                   max_iter=max_iter, el_limit=el_limit, ring=ring, left_of=left_of, counters=c,
                                   cleared_before=cleared)
        records.append(recs)
        down = []
        for gi, r in enumerate(recs):
            if r["stop"][0] in ("hand", "unseen"):
                down += [i for i in ids[gi * Gl * TW:(gi + 1) * Gl * TW] if finish[i] > r["stop"][1]]
        if not down:
            break
        c["handed_down"][lvl] = len(down)
        ids = down
        lvl += 1
    return {"counters": c, "levels": lvl, "compacted": len(sets[1]) if len(sets) > 1 else 0, "row_parallel": row_parallel,
            "sets": sets, "records": records}
