"""The settle rules of the fixed-iteration min-sum path are pure functions of integers (csrc/scaldpc_bp_sched.h): which test
a pass is a half of, which test is complete before it, the frozen-at number of a tile from its words, when a group may stop at
a horizon, and the horizon a handle's next call runs with.  Here the header -- compiled for the HOST with the address and
undefined-behaviour sanitizers (tests/settle_sched_main.cc) -- is held to a restatement of the rules in Python: on
hand-worked scenarios whose expected lines are written out below, and on seeded random ones."""
import os
import subprocess
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("settle_sched") / "settle_sched_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "settle_sched_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: settle_sched_main is built without them")
        subprocess.check_call(cmd)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return [[w if i == 0 else int(w) for i, w in enumerate(ln.split())] for ln in out.stdout.splitlines()]

    return run


# ---- the rules, restated --------------------------------------------------------------------------------------------
# Test t has two halves: variable pass t - 1 and check pass t.  Check pass 2 is the bootstrap pass and compares nothing, so the
# first test is 3 -- or later, if alpha still moves: tests t needs check passes t - 1 and t to run with one alpha.
def first_test(alpha_from):
    return max(3, alpha_from + 1)


def usable(K, ft, max_iter):
    return K >= ft and K + 1 < max_iter


def model_plan(alpha_from, max_iter, K):
    ft = first_test(alpha_from)
    ok = usable(K, ft, max_iter)
    K = K if ok else 0
    tests = range(ft, (K or max_iter) + 1)
    lines = [["plan", ft, int(ok)]]
    for it in range(1, max_iter + 1):
        last = it == max_iter
        if K and K < it < max_iter:
            continue
        has_check = it >= 2 and not (K and last)
        has_var = not (K and it == K)
        check = [-1, -1]
        if has_check:  # complete before it: test it - 1; a half of: test it
            check = [it - 1 if it - 1 in tests else 0, it if it in tests and it != 2 else 0]
        var = [-1, -1]
        if has_var:
            var = [0, 0] if last or it < 2 else [it if it in tests else 0, it + 1 if it + 1 in tests else 0]
        lines.append(["it", it] + check + var)
    lines.append(["saved", 2 * (max_iter - K) if K else 0])
    return lines


def model_frozen(latest, ft, lt):
    """latest = the last test in which something of the tile changed (0 = none)."""
    if lt < ft or latest >= lt:
        return 0
    return max(latest + 1, ft)


def model_next(tiles, frozen, mx, rerun, max_iter):
    if mx <= 0 or 8 * rerun > tiles or 8 * frozen < 7 * tiles or 2 * (mx + 2) >= max_iter:
        return 0
    return mx + 2


def model_calls(max_iter, forced, ft, calls):
    nxt, out = 0, []
    for at in calls:
        K = forced if forced > 0 else nxt
        K = K if usable(K, ft, max_iter) else 0
        seen = [x if ft <= x <= (K or max_iter) else 0 for x in at]
        rerun = sum(1 for s in seen if K and not s)
        fin = [(x if ft <= x <= max_iter else 0) if K and not s else s for x, s in zip(at, seen)]
        frozen, mx = sum(1 for f in fin if f), max(fin)
        nxt = model_next(len(at), frozen, mx, rerun, max_iter)
        out.append(["call", K, rerun, frozen, mx, nxt])
    return out


# ---- hand-worked scenarios ------------------------------------------------------------------------------------------
def test_constants(tool):
    assert tool(["consts"]) == [["consts", 3]]
    # the knob's default (-1): horizon and all on a graph [Hin | I], nothing on any other; a given value holds anywhere
    assert tool(["mode -1 1", "mode -1 0", "mode 0 1", "mode 1 0", "mode 2 0", "mode 2 1"]) == [
        ["mode", 2], ["mode", 0], ["mode", 0], ["mode", 1], ["mode", 2], ["mode", 2]]  # fmt: skip


def test_plan_without_horizon(tool):
    got = tool(["plan 1 6 0"])
    assert got == [["plan", 3, 0],
                   ["it", 1, -1, -1, 0, 0],  # iteration 1: no record-form check pass, a variable pass that is not tracked
                   ["it", 2, 0, 0, 0, 3],    # the bootstrap check pass; variable pass 2 is the first half of test 3
                   ["it", 3, 0, 3, 3, 4],    # check pass 3 completes test 3: variable pass 3 may skip on it
                   ["it", 4, 3, 4, 4, 5],
                   ["it", 5, 4, 5, 5, 6],
                   ["it", 6, 5, 6, 0, 0],    # the last variable pass runs as ever
                   ["saved", 0]]  # fmt: skip
    assert got == model_plan(1, 6, 0)


def test_plan_with_horizon(tool):
    got = tool(["plan 1 50 5"])
    assert got == [["plan", 3, 1],
                   ["it", 1, -1, -1, 0, 0],
                   ["it", 2, 0, 0, 0, 3],
                   ["it", 3, 0, 3, 3, 4],
                   ["it", 4, 3, 4, 4, 5],
                   ["it", 5, 4, 5, -1, -1],   # check pass K closes test K; the closing variable pass takes variable pass K's place
                   ["it", 50, -1, -1, 0, 0],  # the closing sequence: no check pass
                   ["saved", 90]]  # fmt: skip
    assert got == model_plan(1, 50, 5)


def test_plan_alpha_schedule(tool):
    # alpha is one float from iteration 25 on: no test before 26
    got = tool(["plan 25 30 0"])
    assert got[0] == ["plan", 26, 0]
    assert [ln for ln in got if ln[0] == "it" and ln[1] in (24, 25, 26, 27)] == [
        ["it", 24, 0, 0, 0, 0], ["it", 25, 0, 0, 0, 26], ["it", 26, 0, 26, 26, 27], ["it", 27, 26, 27, 27, 28]]  # fmt: skip
    assert got == model_plan(25, 30, 0)
    # max_iter below the first test: nothing is tracked at all
    assert all(ln[2:] in ([-1, -1, 0, 0], [0, 0, 0, 0]) for ln in tool(["plan 25 20 0"]) if ln[0] == "it")


@pytest.mark.parametrize("K, ok", [(2, 0), (3, 1), (48, 1), (49, 0), (50, 0), (60, 0)])
def test_horizon_usable(tool, K, ok):
    assert tool([f"plan 1 50 {K}"])[0] == ["plan", 3, ok]


def test_frozen_at(tool):
    # tests 3 .. 10: nothing ever changed -> frozen at the first test; last change in test 6 -> frozen at 7; a change in
    # the last test (or, stale, beyond it) -> never; no test at all -> never
    assert tool(["frozen 3 10 5 0 6 9 10 11"]) == [["frozen", 3, 7, 10, 0, 0]]
    assert tool(["frozen 3 2 2 0 1"]) == [["frozen", 0, 0]]
    assert tool(["frozen 26 30 3 0 26 29"]) == [["frozen", 26, 27, 30]]


def test_calls_learn_use_reset(tool):
    # 8 tiles, max_iter 50.  Call 1 learns (no horizon): all freeze by 7 -> K = 9.  Call 2 runs with K = 9, one tile now
    # needs 12: re-run (1/8 is not MORE than 1/8), K -> 14.  Call 3: three tiles never freeze: re-run, 3/8 > 1/8 -> off.
    # Call 4 learns again; only 6 of 8 froze (< 7/8) -> no horizon.  Call 5: largest 24 -> 2 K = 52 >= 50 -> none.
    lines = ["calls 50 0 3 8 5  5 6 6 7 6 6 5 6  5 6 6 7 6 12 5 6  5 6 0 7 0 6 0 6  5 6 0 7 0 6 5 6  5 6 6 7 6 6 5 24"]
    got = tool(lines)
    assert got == [["call", 0, 0, 8, 7, 9], ["call", 9, 1, 8, 12, 14], ["call", 14, 3, 5, 7, 0], ["call", 0, 0, 6, 7, 0],
                   ["call", 0, 0, 8, 24, 0]]  # fmt: skip
    assert got == model_calls(50, 0, 3, [[5, 6, 6, 7, 6, 6, 5, 6], [5, 6, 6, 7, 6, 12, 5, 6], [5, 6, 0, 7, 0, 6, 0, 6],
                                         [5, 6, 0, 7, 0, 6, 5, 6], [5, 6, 6, 7, 6, 6, 5, 24]])  # fmt: skip


def test_calls_forced(tool):
    # a forced horizon of 4 under tiles that need 6: every call re-runs them and reports their true numbers
    got = tool(["calls 50 4 3 2 2  4 6  3 6"])
    assert got == [["call", 4, 1, 2, 6, 0], ["call", 4, 1, 2, 6, 0]]


# ---- seeded random scenarios ----------------------------------------------------------------------------------------
def test_random_against_model(tool):
    rng = np.random.default_rng(20260)
    lines, want = [], []
    for _ in range(300):
        af, mi, K = int(rng.integers(1, 30)), int(rng.integers(1, 60)), int(rng.integers(0, 62))
        lines.append(f"plan {af} {mi} {K}")
        want += model_plan(af, mi, K)
    for _ in range(300):
        ft, lt, n = int(rng.integers(3, 30)), int(rng.integers(1, 60)), int(rng.integers(0, 9))
        lat = [int(x) for x in rng.integers(0, 62, n)]
        lines.append(f"frozen {ft} {lt} {n} " + " ".join(map(str, lat)))
        want.append(["frozen"] + [model_frozen(x, ft, lt) for x in lat])
    for _ in range(300):
        mi, forced, ft = int(rng.integers(4, 80)), int(rng.integers(0, 2) * rng.integers(0, 40)), int(rng.integers(3, 8))
        tiles, nc = int(rng.integers(1, 20)), int(rng.integers(1, 6))
        calls = [[int(x) for x in rng.integers(0, 14, tiles) * (rng.random(tiles) < 0.93)] for _ in range(nc)]
        lines.append(f"calls {mi} {forced} {ft} {tiles} {nc} " + " ".join(str(x) for c in calls for x in c))
        want += model_calls(mi, forced, ft, calls)
    got = tool(lines)
    assert got == want
    # invariants: a tracked pass never skips on the test it is a half of; a horizon saves an even, positive launch count
    for ln in got:
        if ln[0] == "it":
            assert ln[3] <= 0 or ln[2] < ln[3]
            assert ln[5] <= 0 or ln[4] < ln[5]
        if ln[0] == "call":
            assert ln[5] == 0 or ln[5] == ln[4] + 2
