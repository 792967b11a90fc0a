"""HQC sweeps that return the attack's decoder statistics (scaldpc_mc_hqc_run_stats) and the checks-needed curve
(driver.hqc_attack_curve), what can be held without a GPU: the answer key of tests/test_hqc_stats_gpu.py recomputed from the CPU
oracle and pinned, the prefix property of the trial law that lets one seed follow a key through a growing graph, the boundary,
and the driver on a decoder double backed by the oracle."""
import csv
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import hqc_stats_cases as cases
from hqc_stats_cases import MAX_ITER, N, OMEGA, RUNS, SEED, STEP, STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
driver = importlib.import_module("sca-ldpc_amd.driver")
bp = importlib.import_module("sca-ldpc_amd.bp")
L = importlib.import_module("sca-ldpc_amd._lib")
S = importlib.import_module("sca-ldpc_amd")


# ------------------------------------------------------------------------------------------------------------- the answer key
@pytest.mark.parametrize("r", STEPS)
def test_the_min_sum_table_is_the_oracle(r):
    """The GPU test's key: successes and the five counters of trials 1000 .. 1199 on the first r rows, from the f32 oracle with
    every codeword's own priors -- never from the library."""
    step = cases.oracle_step(r)
    assert cases.table_row(step) == cases.MIN_SUM_TABLE[r]
    assert (step["stats"][:, 0] == cases.law(r)["msg"][:, N:].sum(axis=1)).all()  # unsatisfied = the weight of the reported checks


def test_every_counter_is_exercised():
    """At 260 rows no counter is zero and no two count the same: 13 trials with bad flips, 7 with bad satisfied checks, 60 with
    bad unsatisfied ones -- a kernel that mixes up two counters or two planes cannot reproduce the row."""
    st = cases.oracle_step(260)["stats"]
    assert [(st[:, k] > 0).sum() for k in (2, 3, 4)] == [13, 7, 60]
    assert len(set(cases.MIN_SUM_TABLE[260])) == 6 and min(cases.MIN_SUM_TABLE[260]) > 0


def test_the_tanh_rule_on_the_oracle():
    assert cases.table_row(cases.oracle_step(260, "product_sum")) == cases.TANH_AT_260
    for r in STEPS[:-1]:
        assert int(cases.oracle_step(r, "product_sum")["success"].sum()) == cases.TANH_SUCCESSES[r]


@pytest.mark.parametrize("method, left", [("min_sum", 10), ("product_sum", 11)])
def test_a_compaction_level_must_be_reached(method, left):
    """What tests/test_hqc_stats_gpu.py's compaction test stands on (the rule: tests/test_mc_edges.py): after iteration 4 between
    1 and 100 of the 200 trials still run -- one tile's worth -- and some of them end with bad flips or checks found bad, so
    counters read before their decisions are scattered back would differ."""
    d = cases.oracle_step(260, method)
    late = (d["iters"] > 4) | (d["converged"] == 0)
    assert late.sum() == left and (d["stats"][late, 2:] > 0).any()


def test_the_trials_of_a_prefix_graph_are_a_prefix_of_the_trials():
    """A trial's secret does not depend on R and check r always takes stream-0 word r: `draw` on the first R' rows is the first
    R' columns of `draw` on all 260 -- what lets one seed follow a key through the attack's growing graph."""
    whole = cases.law(260)
    for r in STEPS[:-1]:
        part = cases.law(r)
        assert np.array_equal(part["y"], whole["y"])
        assert np.array_equal(part["outcome"], whole["outcome"][:, :r])
        assert np.array_equal(part["msg"][:, N:], whole["msg"][:, N : N + r]) and not part["msg"][:, :N].any()
        assert np.array_equal(part["probs"], whole["probs"][:, :r])
        t = cases.wrapped_table()
        assert np.array_equal(part["cost"], t["costs"][whole["outcome"][:, :r]].sum(axis=1))


# --------------------------------------------------------------------------------------------------------------- the boundary
def test_the_boundary_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    assert "#define SCALDPC_VERSION 104" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    soft = re.search(r"\bint scaldpc_mc_hqc_run_soft\(([^;]*)\);", code)
    decl = re.search(r"\bint scaldpc_mc_hqc_run_stats\(([^;]*)\);", code)
    assert decl and len(decl.group(1).split(",")) == 24
    # the soft entry's argument list, then the two new outputs
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    assert norm(decl.group(1)) == norm(soft.group(1)) + ", int32_t *out_stats, uint8_t *out_bits"
    for word in ("Defining property", "found_bad_unsatisfied_checks", "hard_{N+r} & ~reported_r", "scaldpc_bp_append_rows"):
        assert word in src, word
    lib = L.load()
    fn = lib.scaldpc_mc_hqc_run_stats
    assert lib.scaldpc_version() == 104
    assert fn.argtypes == lib.scaldpc_mc_hqc_run_soft.argtypes + [ctypes.c_void_p] * 2 and fn.restype is ctypes.c_int
    # refused before anything touches a device: no handle, no out_stats
    assert fn(*[None if t is ctypes.c_void_p else 0 for t in fn.argtypes]) == L.EINVAL


def test_the_python_surface():
    assert bp.HQC_STATS_COLUMNS == cases.COLUMNS == tuple(driver.STATS_COLUMNS[7:12]) == driver.HQC_STATS_COLUMNS
    for f in (bp.BpDecoder.mc_hqc_run_soft, bp.BpDecoder.mc_hqc_run):
        p = inspect.signature(f).parameters
        assert p["want_stats"].default is False and p["want_bits"].default is False
    assert inspect.signature(driver.hqc_oracle_sweep).parameters["want_stats"].default is False
    assert list(inspect.signature(driver.hqc_attack_curve).parameters) == [
        "first_row_support", "N", "rows", "omega", "table", "runs", "seed", "decode_every", "max_checks", "chunk", "bp_method",
        "max_iter", "bp_decoder"]  # fmt: skip
    assert not hasattr(bp.BpDecoder, "mc_hqc_run_soft_device")  # the class has no device variant of the soft sweep: none is added


# ----------------------------------------------------------------------------------------- the drivers on an oracle-backed double
class OracleSweep:
    """A decoder double with the surface hqc_attack_curve and hqc_oracle_sweep use: a graph that grows by `append_rows`, and
    `mc_hqc_run_soft(want_stats=)` answered by the NumPy law + the CPU oracle (cases.oracle_step).  The double's trial i is the
    law's trial FIRST + i: the key is computed for trials 1000 .. 1199, and the drivers count from 0."""

    log = []

    def __init__(self, H, max_iter, bp_method, channel_probs):
        assert max_iter == MAX_ITER and bp_method == "min_sum" and len(channel_probs) == H.n
        assert np.allclose(channel_probs[:N], OMEGA / N) and ((channel_probs[N:] >= 0) & (channel_probs[N:] <= 1)).all()
        self.m, self.n = H.m, H.n
        self.row_ptr, self.col_idx = H.row_ptr.copy(), H.col_idx.copy()
        self.closed = False
        OracleSweep.last = self

    def append_rows(self, row_ptr, col_idx, new_n, channel_probs_tail):
        assert row_ptr[0] == 0 and len(col_idx) == row_ptr[-1] and len(channel_probs_tail) == new_n - self.n == len(row_ptr) - 1
        self.row_ptr = np.concatenate([self.row_ptr, self.row_ptr[-1] + np.asarray(row_ptr[1:])])
        self.col_idx = np.concatenate([self.col_idx, col_idx])
        self.m += len(row_ptr) - 1
        self.n = new_n

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, max_iter=None, early_exit=True, want_inputs=False,
                        want_stats=False, want_bits=False):
        assert omega == OMEGA and seed == SEED and max_iter == MAX_ITER and early_exit and not want_inputs and not want_bits
        assert not self.closed and 0 <= first_trial and first_trial + runs <= RUNS
        H = cases.cut(self.m)[0]  # the graph the driver built must be the instance cut to its first m rows
        assert self.n == H.n and np.array_equal(self.row_ptr, H.row_ptr) and np.array_equal(self.col_idx, H.col_idx)
        OracleSweep.log.append((self.m, first_trial, runs))
        sl = slice(first_trial, first_trial + runs)
        step, d = cases.oracle_step(self.m), cases.law(self.m)
        res = {"success": step["success"][sl], "iters": step["iters"][sl].astype(np.int32), "flips": d["flips"][sl].astype(np.int32),
               "cost": d["cost"][sl].astype(np.int32) if table.get("costs") is not None else None, "msg": None, "y": None,
               "outcome": None}
        return dict(res, stats=step["stats"][sl], bits=None) if want_stats else res

    def close(self):
        self.closed = True


def curve(chunk=4096, table=None, **kw):
    sup, rows = cases.code()
    OracleSweep.log = []
    got = driver.hqc_attack_curve(sup, N, rows, OMEGA, table or cases.wrapped_table(), RUNS, SEED, STEP, chunk=chunk, bp_method="min_sum",
                                  max_iter=MAX_ITER, bp_decoder=OracleSweep, **kw)
    assert OracleSweep.last.closed
    return got


def test_the_attack_curve_on_the_oracle(tmp_path):
    got = curve()
    assert got["steps"].tolist() == list(STEPS)
    assert got["successes"].tolist() == [cases.MIN_SUM_TABLE[r][0] for r in STEPS] == [1, 13, 115, 176]
    need = got["checks_needed"]
    assert need.dtype == np.int32 and np.array_equal(need, cases.checks_needed())
    # a key is recovered at the first step that decodes it: the curve lies on or above the per-step counts
    assert [(need == r).sum() for r in STEPS] == [1, 13, 105, 58] and (need == -1).sum() == 23
    calls = got["oracle_calls_needed"]
    for r in STEPS:
        assert np.array_equal(calls[need == r], cases.law(r)["cost"][need == r])
    assert (calls[need == -1] == -1).all()
    # decoder_stats: per trial the steps up to and including its first success, the reference's rows (hqc.py:750-758, 980-982)
    rows = got["decoder_stats"]
    assert len(rows) == sum(STEPS.index(r) + 1 if r > 0 else len(STEPS) for r in need.tolist())
    at = {(row["trial"], row["checks"]): row for row in rows}
    assert len(at) == len(rows) and [row["trial"] for row in rows] == sorted(row["trial"] for row in rows)
    for t in range(RUNS):
        mine = [r for r in STEPS if (t, r) in at]
        assert mine == [r for r in STEPS if need[t] == -1 or r <= need[t]]
        for r in mine:
            step, row = cases.oracle_step(r), at[(t, r)]
            assert [row[c] for c in cases.COLUMNS] == step["stats"][t].tolist() and row["success"] == bool(step["success"][t])
            assert row["success"] == (r == need[t]) and row["oracle_calls"] == cases.law(r)["cost"][t]
    # ... which the CSV writer takes unchanged
    path = str(tmp_path / "stats.csv")
    driver.write_decoder_stats_csv(path, rows, "curve", "min_sum", OMEGA, (0.02, 0.1))
    back = list(csv.DictReader(open(path)))
    assert list(back[0]) == driver.STATS_COLUMNS and len(back) == len(rows)
    for line, row in zip(back, rows):
        assert [line[c] for c in driver.STATS_COLUMNS[5:]] == [str(row[c]) for c in driver.STATS_COLUMNS[5:]]
    assert sum(line["success"] == "True" for line in back) == (need > 0).sum()


def test_the_attack_curve_does_not_depend_on_the_chunk():
    want = curve()
    assert OracleSweep.log == [(r, 0, RUNS) for r in STEPS]
    for chunk in (64, 100):
        got = curve(chunk)
        assert OracleSweep.log == [(r, f, min(chunk, RUNS - f)) for r in STEPS for f in range(0, RUNS, chunk)]
        assert got["decoder_stats"] == want["decoder_stats"]
        for k in ("steps", "successes", "checks_needed", "oracle_calls_needed"):
            assert np.array_equal(got[k], want[k]), (chunk, k)


def test_the_attack_curve_edges():
    t = dict(cases.wrapped_table(), costs=None)
    got = curve(table=t, max_checks=140)  # a last partial step is not taken; no costs: nothing counted
    assert got["steps"].tolist() == [65, 130] and got["successes"].tolist() == [1, 13]
    assert got["oracle_calls_needed"] is None and {row["oracle_calls"] for row in got["decoder_stats"]} == {None}
    assert ((got["checks_needed"] == -1).sum(), len(got["decoder_stats"])) == (RUNS - 14, 2 * RUNS - 1)
    sup, rows = cases.code()
    for bad in (dict(decode_every=0), dict(decode_every=65, max_checks=64), dict(decode_every=65, chunk=0)):
        with pytest.raises(ValueError):
            driver.hqc_attack_curve(sup, N, rows, OMEGA, t, RUNS, SEED, **bad, bp_decoder=OracleSweep)


def test_the_sweep_sums_the_counters():
    """hqc_oracle_sweep(want_stats=True): the five counters over all trials and over the successful ones; without the flag the
    decoder is called as before (tests/test_hqc_soft_mc.py's double takes no such argument)."""
    Hin = cases.cut(260)[1]
    st, ok = cases.oracle_step(260)["stats"].astype(np.int64), cases.oracle_step(260)["success"].astype(bool)
    for chunk in (64, 4096):
        got = driver.hqc_oracle_sweep(Hin, N, OMEGA, cases.wrapped_table(), RUNS, SEED, chunk=chunk, bp_method="min_sum", max_iter=MAX_ITER,
                                      bp_decoder=OracleSweep, want_stats=True)
        assert OracleSweep.last.closed and got["successes"] == 176
        assert got["stats"] == dict(zip(cases.COLUMNS, cases.MIN_SUM_TABLE[260][1:]))
        assert got["stats_success"] == dict(zip(cases.COLUMNS, st[ok].sum(axis=0).tolist()))
        assert got["stats_success"]["bad_flips"] == 0 and got["stats_success"]["good_flips"] == 176 * OMEGA
    plain = driver.hqc_oracle_sweep(Hin, N, OMEGA, cases.wrapped_table(), RUNS, SEED, bp_method="min_sum", max_iter=MAX_ITER,
                                    bp_decoder=OracleSweep)
    assert "stats" not in plain and plain["successes"] == 176 and plain["oracle_calls"] == got["oracle_calls"]
