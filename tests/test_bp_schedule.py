"""The early-exit tile scheduler of the binary BP path decides from integers alone: where the host polls, when a group's
stragglers go one level down, when a group stops at the hand-over point unseen, when such groups are chained lane to
lane, when a real poll is forced again, and which row of the counter ring a group takes (csrc/scaldpc_bp_sched.h, which
scaldpc_bp.hip calls).  Here the header -- compiled for the HOST with the address and undefined-behaviour sanitizers
(tests/bp_sched_main.cc) -- and tests/sched_model.py, a restatement of the rules from DESIGN.md and the header's
comments, are held to each other: on hand-worked scenarios, one per branch, whose expected decisions are written out
below, and on a few thousand seeded random ones; the invariants of the schedule are checked on every one of them.
tests/test_bp_schedule_gpu.py then holds the library's own counters (scaldpc_bp_last_schedule) to the model."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import sched_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
KINDS = ("done", "hand", "unseen", "end")
WORDS = ("groups", "handed_down", "polls", "unseen", "continued", "left_open", "fixed_chained", "clears", "open_at_clear",
         "ring_rows", "row_parallel_polls", "ring_takes")  # fmt: skip


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bp_sched") / "bp_sched_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "bp_sched_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: bp_sched_main is built without them")
        subprocess.check_call(cmd)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return [[w if i == 0 else int(w) for i, w in enumerate(ln.split())] for ln in out.stdout.splitlines()]

    return run


def scenario(groups_left, *, T, G, batch=None, early=1, lvl=0, split=2, compact_after=-1, max_iter=40, el_limit=0,
             ring_slot=None, ring_rows=None, cleared=0):
    """One level: groups_left[i] = codewords of group i still running after iteration 1, 2, ... (then: the last)."""
    L = max(len(x) for x in groups_left)
    left = [list(x) + [x[-1]] * (L - len(x)) for x in groups_left]
    rows = M.ring_rows_wanted(T, G) if ring_rows is None else ring_rows
    return dict(early=early, lvl=lvl, T=T, G=G, batch=T * M.TW if batch is None else batch, split=split,
                compact_after=compact_after, max_iter=max_iter, el_limit=el_limit, ring_slot=rows if ring_slot is None else ring_slot,
                ring_rows=rows, cleared=cleared, L=L, left=left)  # fmt: skip


def as_line(sc):
    head = [sc[k] for k in ("early", "lvl", "T", "G", "batch", "split", "compact_after", "max_iter", "el_limit", "ring_slot",
                            "ring_rows", "cleared", "L")]  # fmt: skip
    return "level " + " ".join(str(v) for v in head + [x for g in sc["left"] for x in g])


def by_header(tool, scs):
    """The header's walk of every scenario: (group records, counters, ring slot afterwards)."""
    res, it = [], iter(tool([as_line(sc) for sc in scs]))
    for sc in scs:
        groups = -(-sc["T"] // min(sc["G"], sc["T"]))
        recs = []
        for gi in range(groups):
            w = next(it)
            assert w[0] == "group" and w[1] == gi and len(w) == 9 + w[8]
            recs.append({"chain": w[2], "row": w[3], "cleared": bool(w[4]), "open_before": bool(w[5]), "stop": (KINDS[w[6]], w[7]),
                         "polls": w[9:]})  # fmt: skip
        w = next(it)
        assert w[0] == "counters"
        c = w[1:]
        counters = {"groups": c[0:4], "handed_down": c[4:7], "polls": c[7], "unseen": c[8], "continued": c[9], "left_open": c[10],
                    "fixed_chained": c[11], "clears": c[12], "open_at_clear": c[13], "ring_rows": c[14],
                    "row_parallel_polls": c[15], "ring_takes": c[16]}  # fmt: skip
        w = next(it)
        assert w[0] == "ring"
        res.append((recs, counters, w[1]))
    return res


def by_model(sc):
    ring = M.Ring(sc["ring_rows"], sc["ring_slot"])
    c = M.new_counters(sc["ring_rows"])
    recs, _ = M.walk_level(early=bool(sc["early"]), lvl=sc["lvl"], T=sc["T"], G=sc["G"], batch=sc["batch"], lanes=sc["split"],
                           compact_after=sc["compact_after"], max_iter=sc["max_iter"], el_limit=sc["el_limit"], ring=ring,
                           left_of=lambda gi, it: sc["left"][gi][min(it, sc["L"]) - 1], counters=c,
                           cleared_before=bool(sc["cleared"]))  # fmt: skip
    keep = ("chain", "row", "cleared", "open_before", "stop", "polls")
    return [{k: r[k] for k in keep} for r in recs], c, ring.slot


def both(tool, sc):
    (h, hc, hs), (m, mc, ms) = by_header(tool, [sc])[0], by_model(sc)
    assert h == m and hc == mc and hs == ms
    return m, mc


def check_invariants(sc, recs, c):
    """What must hold of any schedule, whatever the remainders were."""
    hand = M.hand_over_point(bool(sc["early"]), sc["lvl"], sc["compact_after"], sc["max_iter"])
    since = 0
    for i, r in enumerate(recs):
        # a group continues lanes only if the group before it left them open -- and if it was left open lanes, it continues them
        if sc["early"]:
            assert bool(r["chain"] & 1) == (i > 0 and bool(recs[i - 1]["chain"] & 2))
        assert r["open_before"] == (i > 0 and bool(recs[i - 1]["chain"] & 2))
        # no group is left open across a clear of the ring
        if r["cleared"]:
            assert not r["open_before"] and not (r["chain"] & 1)
        if sc["early"] and r["chain"] & 2:
            assert i + 1 < len(recs) and not recs[i + 1]["cleared"]
            # ... and only a group that never meets the host is left open: it stops unseen without a poll before
            assert r["stop"] == ("unseen", hand) and not r["polls"]
        # between two real polls at the hand-over point there are at most SPEC_PERIOD - 1 unseen groups
        if r["stop"][0] == "unseen":
            since += 1
            assert r["stop"][1] == hand and hand > 0
        elif hand in r["polls"]:
            since = 0
        assert since <= M.SPEC_PERIOD - 1
        # a level without a hand-over point hands nothing over
        if hand == 0:
            assert r["stop"][0] in ("done", "end")
        if r["stop"][0] == "hand":
            assert r["stop"][1] >= hand and 2 * r["stop"][1] < sc["max_iter"]
    assert c["open_at_clear"] == 0
    assert c["continued"] == c["left_open"] if sc["early"] else c["continued"] == c["left_open"] == 0
    if sc["early"]:
        rows = [r["row"] for r in recs]
        assert all(1 <= x < sc["ring_rows"] for x in rows)  # row 0 is never handed out
        assert c["ring_takes"] == len(recs)


# ---- the header's small decisions, value for value -----------------------------------------------------------------


def test_constants_agree(tool):
    assert tool(["consts"])[0][1:] == [M.TW, M.MAX_LANES, M.MAX_LEVELS, M.REM_SLOTS, M.SPEC_PERIOD, M.POLL_EVERY, 17]


def test_poll_points_and_the_hint(tool):
    """Iteration 1, every 4th and the hand-over point, from the hint on."""
    got = tool(["pred 1 0 0 4 20", "pred 1 0 0 2 20", "pred 2 0 0 6 20", "pred 5 0 0 4 20", "pred 7 0 0 6 20", "pred 1 0 0 0 9"])
    assert got[0] == ["pred", 0, 0, 1, 4, 8, 12, 16, 20]
    assert got[1] == ["pred", 0, 0, 1, 2, 4, 8, 12, 16, 20]
    assert got[2] == ["pred", 0, 0, 4, 6, 8, 12, 16, 20]
    assert got[3] == ["pred", 0, 0, 8, 12, 16, 20]  # (a hint past the hand-over point: it is no poll point any more)
    assert got[4] == ["pred", 0, 0, 8, 12, 16, 20]
    assert got[5] == ["pred", 0, 0, 1, 4, 8]
    for hint in range(1, 12):
        for hand in (0, 2, 3, 4, 5, 8):
            p = M.Poll(hint, 0, 0)
            want = [it for it in range(1, 31) if M.is_poll_point(it, hand, p)]
            assert tool([f"pred {hint} 0 0 {hand} 30"])[0][3:] == want


def test_unseen_predicates(tool):
    """stops_unseen: a streak of two, fewer than SPEC_PERIOD - 1 unseen groups since the last real poll, a hand-over point
    that is worth it and still live; runs_unseen: and no live poll point before it.  runs_unseen implies stops_unseen."""
    lines, want = [], []
    for hint in (1, 2, 3, 4, 5, 6):
        for streak in (0, 1, 2, 3, 9):
            for since in (0, 1, 13, 14, 15, 16):
                for hand in (0, 2, 4, 5, 8):
                    for max_iter in (8, 9, 16, 17, 40):
                        p = M.Poll(hint, streak, since)
                        lines.append(f"pred {hint} {streak} {since} {hand} {max_iter}")
                        want.append((int(M.stops_unseen(hand, max_iter, p)), int(M.runs_unseen(hand, max_iter, p))))
    got = [(w[1], w[2]) for w in tool(lines)]
    assert got == want
    assert all(s >= r for s, r in got) and any(s > r for s, r in got) and any(r for s, r in got)
    # by hand: hand-over point 4 of 40 iterations
    assert tool(["pred 2 2 0 4 40"])[0][1:3] == [1, 1]  # hint 2: iteration 1 is skipped, nothing live before 4
    assert tool(["pred 1 2 0 4 40"])[0][1:3] == [1, 0]  # iteration 1 still polls: stops unseen at 4, but meets the host
    assert tool(["pred 2 1 0 4 40"])[0][1:3] == [0, 0]  # one small remainder is no streak
    assert tool(["pred 2 2 14 4 40"])[0][1:3] == [1, 1]  # the 15th unseen group in a row
    assert tool(["pred 2 2 15 4 40"])[0][1:3] == [0, 0]  # the 16th polls for real
    assert tool(["pred 5 2 0 4 40"])[0][1:3] == [0, 0]  # the hint is past the hand-over point
    assert tool(["pred 2 2 0 4 8"])[0][1:3] == [0, 0]  # 2 * 4 is not below max_iter


def test_hand_over_point_per_level(tool):
    """Levels 0 .. 2 hand over (default after 4 iterations; not where max_iter <= twice that), level 3 never does."""
    for early in (0, 1):
        for lvl in range(4):
            for ca in (-1, 0, 1, 2, 4, 7, 20):
                for mi in (1, 4, 8, 9, 14, 15, 40, 41):
                    want = M.hand_over_point(bool(early), lvl, ca, mi)
                    assert tool([f"hand {early} {lvl} {ca} {mi}"])[0][1] == want
    assert [tool([f"hand 1 {lvl} -1 40"])[0][1] for lvl in range(4)] == [4, 4, 4, 0]
    assert tool(["hand 1 0 2 40"])[0][1] == 2 and tool(["hand 1 0 4 8"])[0][1] == 0 and tool(["hand 1 0 4 9"])[0][1] == 4
    assert tool(["hand 0 0 -1 40"])[0][1] == 0


def test_deal_and_ring_size(tool):
    for g in range(1, 12):
        for split in (0, 1, 2, 3, 4, 7):
            w = tool([f"deal {g} {split}"])[0]
            nl = M.lanes_of(split, g)
            sizes, firsts = M.deal(g, nl)
            assert w[1] == nl and w[2::2] == sizes and w[3::2] == firsts and sum(sizes) == g and max(sizes) - min(sizes) <= 1
    assert tool(["deal 5 2"])[0][1:] == [2, 3, 0, 2, 3]
    for T, G in ((1, 1), (6, 6), (22, 1), (44, 2), (503, 1), (504, 1), (505, 1), (1040, 2), (520, 1), (65535, 1), (7, 0)):
        assert tool([f"rows {T} {G}"])[0][1] == M.ring_rows_wanted(T, G)
    assert tool(["rows 44 2"])[0][1] == 52 and tool(["rows 1040 2"])[0][1] == 512 and tool(["rows 6 6"])[0][1] == 10
    assert tool(["elpoll 40"])[0][1:] == [3, 4, 5, 6, 8, 10, 12, 14, 16, 32]
    assert M.row_parallel_polls([41] * 20, 40) == 10 and M.row_parallel_polls([3, 5], 40) == 3  # (after 3, 4 and 5)


# ---- hand-worked scenarios, one per branch ---------------------------------------------------------------------------

SMALL = [128, 128, 128, 6]  # 128 codewords: nobody done after 1 .. 3, six left after iteration 4 (<= 1/8)


def test_stragglers_go_one_level_down(tool):
    """One group of 6 tiles, hand-over point 2 (`compact_after=2`): the poll after iteration 1 finds all 384 running and
    moves the hint, the poll after 2 finds 140 (at most half, 3 tiles < 6) and hands them down.  140 > 384 / 8: no streak.
    The level below (3 tiles): 140 after 1 and 2 -- no hand-over, more than half -- then 70 after 4."""
    recs, c = both(tool, scenario([[384, 140]], T=6, G=6, compact_after=2))
    assert recs[0]["polls"] == [1, 2] and recs[0]["stop"] == ("hand", 2) and c["polls"] == 2 and c["groups"] == [1, 0, 0, 0]
    recs, c = both(tool, scenario([[140, 140, 140, 70]], T=3, G=6, batch=140, lvl=1, compact_after=2, ring_slot=2, ring_rows=10, cleared=1))
    assert recs[0]["polls"] == [1, 2, 4] and recs[0]["stop"] == ("hand", 4) and recs[0]["row"] == 2 and c["groups"] == [0, 1, 0, 0]
    # level 3 has no hand-over point: 20 codewords that never converge are polled after 1 (hint), 4, 8, .. 36 and run to the end
    recs, c = both(tool, scenario([[20]], T=1, G=6, batch=20, lvl=3, compact_after=2, ring_slot=4, ring_rows=10, cleared=1))
    assert recs[0]["polls"] == [1, 4, 8, 12, 16, 20, 24, 28, 32, 36] and recs[0]["stop"] == ("end", 40) and c["groups"] == [0, 0, 0, 1]
    # ... while level 2 would have handed over HALF of a 2-tile group (64 of 128 fill fewer tiles) but not 65
    recs, _ = both(tool, scenario([[128, 128, 128, 64]], T=2, G=2, lvl=2))
    assert recs[0]["stop"] == ("hand", 4)
    recs, _ = both(tool, scenario([[128, 128, 128, 65, 65, 65, 65, 64]], T=2, G=2, lvl=2))
    assert recs[0]["polls"] == [1, 4, 8] and recs[0]["stop"] == ("hand", 8)
    # the restart must be cheap: after iteration 20 of 40 nothing is handed over any more
    recs, _ = both(tool, scenario([[128] * 19 + [10]], T=2, G=2))
    assert recs[0]["stop"] == ("end", 40) and recs[0]["polls"] == [1, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    # stragglers that fill as many tiles as the group has are kept -- unless the row-parallel kernels take them
    recs, _ = both(tool, scenario([[40, 40, 40, 20]], T=1, G=1, batch=40))
    assert recs[0]["stop"] == ("end", 40)
    recs, _ = both(tool, scenario([[40, 40, 40, 20]], T=1, G=1, batch=40, el_limit=20))
    assert recs[0]["stop"] == ("hand", 4)


def test_unseen_chained_and_repolled(tool):
    """22 groups of 2 tiles on 2 lanes, six stragglers each after iteration 4 (the last group holds 70 codewords): groups
    1 and 2 poll (group 1 after iteration 1 as well, which moves the hint), groups 3 .. 17 stop unseen -- 15 of them --
    group 18 polls for real, groups 19 .. 22 stop unseen again.  Every unseen group runs without the host, so 3 .. 16 and
    19 .. 21 leave their lanes open and 4 .. 17 and 20 .. 22 continue them."""
    sc = scenario([SMALL] * 21 + [[70, 70, 70, 6]], T=44, G=2, batch=21 * 128 + 70)
    recs, c = both(tool, sc)
    assert [r["polls"] for r in recs[:2]] == [[1, 4], [4]] and recs[17]["polls"] == [4]
    assert [i + 1 for i, r in enumerate(recs) if r["stop"][0] == "unseen"] == list(range(3, 18)) + [19, 20, 21, 22]
    assert [i + 1 for i, r in enumerate(recs) if r["chain"] & 2] == list(range(3, 17)) + [19, 20, 21]
    assert [i + 1 for i, r in enumerate(recs) if r["chain"] & 1] == list(range(4, 18)) + [20, 21, 22]
    assert c["polls"] == 4 and c["unseen"] == 19 and c["continued"] == 17 and c["left_open"] == 17 and c["clears"] == 0
    assert [r["row"] for r in recs] == list(range(1, 23)) and c["ring_rows"] == 52
    check_invariants(sc, recs, c)
    # one lane: the same polls, nothing chained
    recs1, c1 = both(tool, dict(sc, split=1))
    assert [r["stop"] for r in recs1] == [r["stop"] for r in recs] and c1["continued"] == c1["left_open"] == 0 and c1["unseen"] == 19
    # a ragged last group of ONE tile is no full group: group 21 is not left open for it
    sc = scenario([SMALL] * 21 + [[6, 6, 6, 1]], T=43, G=2, batch=21 * 128 + 6)
    recs, c = both(tool, sc)
    assert recs[20]["chain"] == 1 and recs[21]["chain"] == 0 and recs[21]["stop"] == ("unseen", 4)
    check_invariants(sc, recs, c)


def test_a_wrong_guess_is_stopped_all_the_same(tool):
    """Group 7 of the batch above holds 128 stragglers: it is stopped unseen like its neighbours (nobody looks), and the
    schedule of the other groups does not change."""
    sc = scenario([SMALL] * 6 + [[128]] + [SMALL] * 14 + [[70, 70, 70, 6]], T=44, G=2, batch=21 * 128 + 70)
    recs, c = both(tool, sc)
    assert recs[6]["stop"] == ("unseen", 4) and recs[6]["chain"] == 3 and recs[6]["polls"] == []
    assert c["polls"] == 4 and c["unseen"] == 19 and c["continued"] == 17
    # seen at a real poll, the same group ends the streak: group 18 is the 16th, finds 128 running at every poll point and
    # moves the hint past each of them -- to 37 in the end, so the groups after it are not polled at all and run through
    sc = scenario([SMALL] * 17 + [[128]] + [SMALL] * 4, T=44, G=2)
    recs, c = both(tool, sc)
    assert recs[17]["polls"] == [4, 8, 12, 16, 20, 24, 28, 32, 36] and recs[17]["stop"] == ("end", 40)
    assert [r["polls"] for r in recs[18:]] == [[], [], [], []] and [r["stop"] for r in recs[18:]] == [("end", 40)] * 4
    assert c["unseen"] == 15 and c["polls"] == 3 + 9
    check_invariants(sc, recs, c)


def test_ring_wraps_and_nothing_is_open_at_the_clear(tool):
    """520 groups of 2 tiles take rows 1 .. 511 of a 512-row ring, the 512th group clears it and starts again at row 1.
    The group two before the clear is the last one left open: its successor's row is the ring's last but one."""
    sc = scenario([SMALL] * 520, T=1040, G=2)
    recs, c = both(tool, sc)
    assert c["ring_rows"] == 512 and c["clears"] == 1 and c["open_at_clear"] == 0 and c["ring_takes"] == 520
    assert [r["row"] for r in recs] == list(range(1, 512)) + list(range(1, 10))
    assert [i + 1 for i, r in enumerate(recs) if r["cleared"]] == [1, 512]
    assert not recs[511]["open_before"] and recs[511]["chain"] & 1 == 0 and recs[510]["chain"] & 2 == 0
    assert recs[510]["stop"][0] == "unseen" and recs[511]["stop"][0] == "unseen"
    check_invariants(sc, recs, c)
    # one tile per group has one lane: the ring wraps all the same, nothing is ever open
    sc = scenario([[64, 64, 64, 3]] * 520, T=520, G=1)
    recs, c = both(tool, sc)
    assert c["clears"] == 1 and c["continued"] == 0 and [i + 1 for i, r in enumerate(recs) if r["cleared"]] == [1, 512]
    # a small ring wraps often: every clear finds the lanes joined
    sc = scenario([SMALL] * 60, T=120, G=2, ring_rows=7)
    recs, c = both(tool, sc)
    assert c["clears"] == 9 and c["open_at_clear"] == 0 and c["left_open"] > 0
    check_invariants(sc, recs, c)
    # a level that starts in the middle of the ring (the levels of one call share it)
    sc = scenario([SMALL] * 12, T=24, G=2, ring_rows=12, ring_slot=9, cleared=1, lvl=1)
    recs, c = both(tool, sc)
    assert [r["row"] for r in recs] == [9, 10, 11, 1, 2, 3, 4, 5, 6, 7, 8, 9] and c["clears"] == 1
    check_invariants(sc, recs, c)


def test_fixed_iteration_groups_chain(tool):
    """Without early exit every full group continues the full group before it; no polls, no counter rows."""
    sc = scenario([[128]] * 5 + [[64]], T=11, G=2, batch=11 * 64, early=0)
    recs, c = both(tool, sc)
    assert [r["chain"] for r in recs] == [2, 3, 3, 3, 1, 0] and c["fixed_chained"] == 4 and c["polls"] == c["ring_takes"] == 0
    assert c["continued"] == c["left_open"] == 0 and all(r["stop"] == ("end", 40) for r in recs)
    recs, c = both(tool, dict(sc, split=1))
    assert [r["chain"] for r in recs] == [0] * 6 and c["fixed_chained"] == 0


# ---- seeded random scenarios -------------------------------------------------------------------------------------------


def random_scenario(rng):
    groups = int(np.exp(rng.uniform(0, np.log(600)))) if rng.rand() < 0.9 else rng.randint(500, 601)
    groups = max(1, min(600, groups))
    G = rng.choice([1, 1, 2, 2, 3, 4, 5])
    T = groups * G - (rng.randint(0, G) if groups > 0 else 0)  # ragged last group
    T = max(T, (groups - 1) * G + 1)
    batch = T * M.TW - rng.randint(0, M.TW)  # ... and a ragged last tile
    max_iter = int(rng.choice([3, 7, 8, 9, 12, 20, 40]))
    L = min(max_iter, 12)
    style = rng.randint(4)
    left = []
    for gi in range(-(-T // min(G, T))):
        g = min(G, T - gi * G)
        real = min(batch - gi * G * M.TW, g * M.TW)
        if style == 0 or (style == 3 and rng.rand() < 0.9):  # mostly small remainders at some iteration: the unseen regime
            at = rng.choice([2, 3, 4, 4, 4, 5])
            small = rng.randint(0, max(1, real // 8) + 1)
            seq = [real if it < at else small for it in range(1, L + 1)]
        elif style == 1:  # anything non-increasing
            seq = sorted(rng.randint(0, real + 1, size=L).tolist(), reverse=True)
        else:  # nobody ever finishes, or everybody at once
            seq = [real] * L if rng.rand() < 0.5 else [real] * rng.randint(0, L) + [0] * L
            seq = seq[:L]
        left.append(seq)
    rows = int(rng.choice([M.ring_rows_wanted(T, G), 512, rng.randint(2, 40)]))
    slot = rows if rng.rand() < 0.5 else rng.randint(1, rows + 1)
    return scenario(left, T=T, G=G, batch=batch, early=int(rng.rand() < 0.9), lvl=rng.randint(4), split=rng.randint(1, 4),
                    compact_after=int(rng.choice([-1, -1, 0, 2, 3, 4, 5])), max_iter=max_iter, el_limit=int(rng.choice([0, 4, 6, 64])),
                    ring_slot=slot, ring_rows=rows, cleared=int(slot != rows or rng.rand() < 0.3))  # fmt: skip


def test_random_scenarios(tool):
    rng = np.random.RandomState(20260)
    scs = [random_scenario(rng) for _ in range(3000)]
    seen = {"unseen": 0, "continued": 0, "clears": 0, "hand": 0, "repoll": 0, "fixed_chained": 0}
    for sc, (h, hc, hs) in zip(scs, by_header(tool, scs)):
        m, mc, ms = by_model(sc)
        assert h == m and hc == mc and hs == ms, as_line(sc)[:200]
        check_invariants(sc, m, mc)
        for k in ("unseen", "continued", "clears", "fixed_chained"):
            seen[k] += mc[k] > 0
        seen["hand"] += any(r["stop"][0] == "hand" for r in m)
        seen["repoll"] += mc["unseen"] >= M.SPEC_PERIOD
    assert all(v >= 20 for v in seen.values()), seen  # (the sweep reaches every branch, many times)


def test_every_straggler_goes_down_exactly_once():
    """Whole calls from per-codeword iteration counts (the model alone): a codeword a group leaves unfinished at a
    hand-over is in the next level's set exactly once and in no other group's; a codeword that is not handed on finished
    by the time its group stopped, or its group ran all iterations."""
    rng = np.random.RandomState(7)
    deepest = 0
    for case in range(60):
        batch = rng.randint(1, 3000)
        max_iter = int(rng.choice([9, 20, 40]))
        iters = rng.choice([1, 2, 3, 3, 3, 4, 4, 5, 6, 7, 9, 12, max_iter], size=batch)
        conv = (iters < max_iter) | (rng.rand(batch) < 0.2)
        G = int(rng.choice([1, 2, 4, 64]))
        T = -(-batch // M.TW)
        res = M.predict(iters, conv, G=min(G, T), lanes=2, compact_after=int(rng.choice([-1, 2, 3])), max_iter=max_iter,
                        el_limit=int(rng.choice([0, 6, 64])), ring_rows=M.ring_rows_wanted(T, min(G, T)))
        finish = np.where(conv, iters, max_iter + 1)
        deepest = max(deepest, res["levels"])
        assert res["levels"] == len(res["sets"]) - 1 <= M.MAX_LEVELS and res["sets"][0] == list(range(batch))
        for lvl, (ids, recs) in enumerate(zip(res["sets"], res["records"])):
            nxt = res["sets"][lvl + 1] if lvl + 1 < len(res["sets"]) else []
            assert len(set(nxt)) == len(nxt) and set(nxt) <= set(ids) and nxt == sorted(nxt, key=ids.index)
            if not recs:  # the row-parallel kernels: the end of the line
                assert not nxt and len(ids) == res["row_parallel"]
                continue
            Gl = min(G, T, -(-len(ids) // M.TW))
            want = []
            for gi, r in enumerate(recs):
                mine = ids[gi * Gl * M.TW:(gi + 1) * Gl * M.TW]
                assert len(mine) == r["real"]
                kind, it = r["stop"]
                if kind in ("hand", "unseen"):
                    want += [i for i in mine if finish[i] > it]
                elif kind == "done":
                    assert all(finish[i] <= it for i in mine)
                else:
                    assert it == max_iter
            assert want == nxt and res["counters"]["handed_down"][lvl:lvl + 1] == ([len(nxt)] if lvl < 3 else [])
        assert res["counters"]["open_at_clear"] == 0 and sum(res["counters"]["groups"]) == sum(len(r) for r in res["records"])
    assert deepest == M.MAX_LEVELS


def test_the_library_decides_by_the_header():
    """scaldpc_bp.hip keeps no rules of its own: it calls the header's functions where it decides."""
    src = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_bp.hip")).read()
    assert '#include "scaldpc_bp_sched.h"' in src
    for name in ("poll_point", "stops_unseen", "runs_unseen", "deal_tiles", "after_poll", "chain_bits", "defer_after_of",
                 "ring_take", "ring_rows_wanted", "lanes_of", "el_poll_point"):  # fmt: skip
        assert not re.search(r"^\w[\w ]*\b%s\(.*\)\s*$" % name, src, re.M), name  # (no definition of its own)
    body = re.search(r"\nint iterate_tiles\(.*?\n}\n", src, re.S).group(0)
    for call in ("poll_point(it, defer_after, ps)", "stops_unseen(defer_after, max_iter, ps)", "after_poll(ps, it, defer_after, max_iter,",
                 "deal_tiles(g, nl, gs, t0)", "next_remaining_row(h, s, &rem, lanes.open)"):  # fmt: skip
        assert call in body, call
    body = re.search(r"\nint decode_level\(.*?\n}\n", src, re.S).group(0)
    assert "chain_bits(early, lanes2, g == Gl, g0 == 0, next_full, lanes.open, defer_after, max_iter, poll, h->rem)" in body
    assert "defer_after_of(early, lvl, h->kn.compact_after, max_iter)" in body
    body = re.search(r"\nint next_remaining_row\(.*?\n}\n", src, re.S).group(0)
    assert "ring_take(h->rem, &clears)" in body and "note_take(clears, lanes_open)" in body
    hdr = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_bp_sched.h")).read()
    assert "hip_runtime" not in hdr and "__global__" not in hdr and "__device__" not in hdr  # plain C++
