"""The sparse settle gate on the CPU: tests/settle_sparse_ref.py restates the rule by which rows and columns of a tracked
tile run only when an input of theirs changed.  Here, before any kernel: the restatement's arithmetic is settle_ref's; the
rule is CONSERVATIVE on every input tests/test_settle_sparse_gpu.py uses -- no gated-out node has an output that differs in
any codeword of its tile; the inputs contain what that file relies on; and the pure functions that say which passes write
flags and which gate (csrc/scaldpc_bp_sched.h, built for the host under the sanitizers: tests/settle_sparse_main.cc) are
the restatement's."""
import os
import subprocess

import numpy as np
import pytest

import settle_matrix_cases as MC
import settle_ref as R
import settle_sparse_ref as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


def tiles_of(batch):
    return range((batch + 63) // 64)


@pytest.mark.parametrize("name", ["hqc", "schedule"])
def test_trace_is_settle_ref(name):
    c, tr = R.case(name), SP.traced(name)
    for it in (1, 2, 7, R.MAX_ITER):
        assert (tr.post[it].view(np.uint32) == c.post[it].view(np.uint32)).all()


@pytest.mark.parametrize("name", ["hqc", "schedule"])
def test_frozen_at_is_settle_ref(name):
    """The rule's own settle words -- taken from the nodes that RUN -- give settle_ref's frozen-at numbers."""
    c, tr = R.case(name), SP.traced(name)
    batch = c.synd.shape[0]
    want = R.frozen_at(c.same, c.first, R.MAX_ITER)
    assert [SP.activity(tr, t, batch, c.first).frozen_at for t in tiles_of(batch)] == want


@pytest.mark.parametrize("name,last", [("hqc", None), ("hqc", 8), ("schedule", None)])
def test_conservative(name, last):
    c, tr = R.case(name), SP.traced(name)
    batch = c.synd.shape[0]
    for t in tiles_of(batch):
        act = SP.activity(tr, t, batch, c.first, last)
        assert SP.violations(tr, act, t, batch) == 0, (name, t)
        # ... and the tables do not depend on the gate: a node that is gated out would have stamped nothing new that matters
        assert act.frozen_at == SP.activity(tr, t, batch, c.first, last, sparse=False).frozen_at


def test_a_weaker_rule_is_caught():
    """`violations` can fail: with the arg-min bits left out of `dirty` some gated-out column has another output."""
    c, tr = R.case("hqc"), SP.traced("hqc")
    orig = SP._bits
    SP._bits = lambda idx: np.uint64(0)
    try:
        bad = sum(SP.violations(tr, SP.activity(tr, t, R.BATCH, c.first), t, R.BATCH) for t in tiles_of(R.BATCH))
    finally:
        SP._bits = orig
    assert bad > 0


def test_the_own_sign_rule_is_needed_and_caught():
    """settle_sparse_ref.own_case: in tile 1 a column runs through its own sign_changed bit alone; the rule without that term
    gates out columns whose outputs differ and leaves other tables; the rule as it is stays conservative."""
    c = SP.own_case()
    right, wrong = SP.activity(c.tr, 1, SP.OWN_BATCH, 3), SP.activity(c.tr, 1, SP.OWN_BATCH, 3, own_rule=False)
    assert SP.violations(c.tr, right, 1, SP.OWN_BATCH) == 0 and SP.violations(c.tr, wrong, 1, SP.OWN_BATCH) > 0
    assert sum(int((right.col_runs[it] != wrong.col_runs[it]).sum()) for it in right.col_runs) > 50
    assert (right.col_flag != wrong.col_flag).any() or (right.row_stamp != wrong.row_stamp).any()
    assert SP.violations(c.tr, SP.activity(c.tr, 0, SP.OWN_BATCH, 3), 0, SP.OWN_BATCH) == 0


def test_inputs_hold_what_the_gpu_file_relies_on():
    c, tr = R.case("hqc"), SP.traced("hqc")
    acts = [SP.activity(tr, t, R.BATCH, c.first) for t in tiles_of(R.BATCH)]
    cdeg = np.diff(np.asarray(c.H.col_ptr))
    ncol = int((cdeg > 1).sum())
    some_rows = some_cols = 0
    for a in acts:
        some_rows += sum(1 for r in a.row_runs.values() if 0 < r.sum() < c.H.m)
        some_cols += sum(1 for r in a.col_runs.values() if 0 < r.sum() < ncol)
    assert some_rows > 0 and some_cols > 0  # passes in which some but not all nodes run
    assert [a.frozen_at > 0 for a in acts] == [True, False, True, False, True, True]  # tiles 1 and 3 never freeze
    assert R.BATCH % 64 == 3  # tile 5 is partial
    for t in (0, 2, 4):  # thin out, then stop
        a = acts[t]
        thin = [it for it in range(5, a.frozen_at) if 0 < a.col_runs[it].sum() < ncol]
        assert len(thin) >= 2 and all(a.col_runs[it].sum() == 0 for it in range(a.frozen_at, R.MAX_ITER))
    for t in (1, 3):  # cycle: partly active to the end
        a = acts[t]
        assert all(0 < a.col_runs[it].sum() < ncol for it in range(12, R.MAX_ITER))
    # a dirty mask that is neither empty nor full survives in the tables: the arg-min-only path
    assert any(((a.row_dirty != 0) & (a.row_dirty != SP.ALL)).any() for a in acts)
    # the schedule case gates only from its first test on
    s, ts = R.case("schedule"), SP.traced("schedule")
    a = SP.activity(ts, 0, 70, s.first)
    assert s.first > 20 and all(a.row_runs[it].all() for it in range(2, s.first + 1))
    assert all(a.col_runs[it].sum() == ncol for it in range(2, s.first))


@pytest.mark.parametrize("name", ["row32", "row64", "ties32", "ties64"])
def test_conservative_on_the_matrix_graphs(name):
    """Rows of 18 and 34 edges, and the tie inputs, whose last change in a tile is often an arg-min index alone."""
    c = MC.case(name)
    batch = c.synd.shape[0]
    tr = SP.trace(c.H, R.prior_llr(c.probs), c.synd, R.MAX_ITER, 1.0)
    assert (tr.post[R.MAX_ITER].view(np.uint32) == c.post.view(np.uint32)).all()
    acts = [SP.activity(tr, t, batch, 3) for t in tiles_of(batch)]
    assert [a.frozen_at for a in acts] == c.want
    for t, a in enumerate(acts):
        assert SP.violations(tr, a, t, batch) == 0, (name, t)


# ---- the pure functions of scaldpc_bp_sched.h ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("settle_sparse") / "settle_sparse_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "settle_sparse_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    built = subprocess.run(cmd + san, capture_output=True, text=True)
    if built.returncode != 0:
        pytest.fail("settle_sparse_main did not build under -fsanitize=address,undefined: " + built.stderr[-2000:])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr
        return [[w if i == 0 else int(w) for i, w in enumerate(ln.split())] for ln in out.stdout.splitlines()]

    return run


def model_gates(ft, lt, max_iter, start=0):
    out = []
    for it in range(2, max_iter + 1):
        var = it < lt
        out.append(["it", it, int(SP.check_writes(it, ft, lt)), int(SP.check_gates(it, ft, lt, start)),
                    int(var and SP.var_writes(it, ft, lt)), int(var and SP.var_gates(it, ft, lt, start))])
    return out


def test_gates_hand_worked(tool):
    # first test 3, horizon 6 of 9 iterations: check 3 writes, check 4 .. 6 gate; var 2 writes, var 3 .. 5 write and gate
    got = tool(["gates 3 6 9 0"])
    assert got == [["it", 2, 0, 0, 1, 0], ["it", 3, 1, 0, 1, 1], ["it", 4, 1, 1, 1, 1], ["it", 5, 1, 1, 1, 1],
                   ["it", 6, 1, 1, 0, 0], ["it", 7, 0, 0, 0, 0], ["it", 8, 0, 0, 0, 0], ["it", 9, 0, 0, 0, 0]]
    assert got == model_gates(3, 6, 9) == tool(["gates 3 6 9 3"]) == tool(["gates 3 6 9 2"])
    # a learned start of 5: variable pass 5 is the first to gate, check pass 6 the first check pass; the flags are written as ever
    assert tool(["gates 3 6 9 5"]) == [["it", 2, 0, 0, 1, 0], ["it", 3, 1, 0, 1, 0], ["it", 4, 1, 0, 1, 0], ["it", 5, 1, 0, 1, 1],
                                       ["it", 6, 1, 1, 0, 0], ["it", 7, 0, 0, 0, 0], ["it", 8, 0, 0, 0, 0], ["it", 9, 0, 0, 0, 0]]
    assert tool(["gates 3 6 9 5"]) == model_gates(3, 6, 9, 5)


def test_gates_random(tool):
    rng = np.random.RandomState(3)
    sc = [(int(rng.randint(3, 30)), int(rng.randint(2, 60)), int(rng.randint(2, 60))) for _ in range(200)]
    sc = [(ft, min(lt, mi), mi, int(rng.randint(0, 40))) for ft, lt, mi in sc]
    got = tool([f"gates {ft} {lt} {mi} {st}" for ft, lt, mi, st in sc])
    want = [ln for ft, lt, mi, st in sc for ln in model_gates(ft, lt, mi, st)]
    assert got == want


def test_next_start(tool):
    """Two passes before the smallest frozen-at number of the last call, the first test at the earliest; 0 = nothing froze."""
    assert tool(["start 8 3", "start 0 3", "start 4 3", "start 3 3", "start 30 26", "start 26 26"]) == [
        ["start", 6], ["start", 0], ["start", 3], ["start", 3], ["start", 28], ["start", 26]]
    sc = [(at, ft) for at in range(0, 40) for ft in (3, 7, 26)]
    assert tool([f"start {at} {ft}" for at, ft in sc]) == [["start", SP.next_start([0, at, at + 3] if at else [0, 0], ft)] for at, ft in sc]
    assert SP.next_start(None, 3) == SP.next_start([], 3) == SP.next_start([0, 0], 3) == 0


def test_conservative_under_a_learned_start():
    """Gating from a later pass on is the same rule on fewer passes: still conservative, the same frozen-at numbers, and on
    the tiles that thin out the passes before the start run in full."""
    c, tr = R.case("hqc"), SP.traced("hqc")
    want = R.frozen_at(c.same, c.first, R.MAX_ITER)
    start = SP.next_start(want, c.first)
    assert start == min(f for f in want if f) - 2 > c.first
    ncol = int((np.diff(np.asarray(c.H.col_ptr)) > 1).sum())
    for t in tiles_of(R.BATCH):
        a = SP.activity(tr, t, R.BATCH, c.first, start=start)
        assert SP.violations(tr, a, t, R.BATCH) == 0 and a.frozen_at == want[t]
        assert all(a.col_runs[it].sum() == ncol for it in range(2, min(start, a.frozen_at or start)))


def test_mode(tool):
    sc = [(k, s, i) for k in (-1, 0, 1) for s in (0, 1, 2) for i in (0, 1)]
    got = tool([f"mode {k} {s} {i}" for k, s, i in sc])
    assert got == [["mode", 0 if s == 0 else k if k >= 0 else int(s == 2 and i == 1)] for k, s, i in sc]
