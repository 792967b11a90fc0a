"""TEST INFRASTRUCTURE shared by tests/test_hqc_stats.py (CPU) and tests/test_hqc_stats_gpu.py: the instance of
tests/test_hqc_soft_mc_gpu.py cut to its first 65 / 130 / 195 / 260 rows, the NumPy law on every cut, and the answer key -- the
f32 CPU oracle, one call per codeword with that codeword's own priors (soft_cases.oracle_per_codeword), counted by
driver.hqc_stats.  Nothing here comes from the library under test."""
import functools
import importlib

import numpy as np

import hqc_soft_mc_ref as ref
import soft_cases
from helpers import S, hqc_instance

driver = importlib.import_module("sca-ldpc_amd.driver")
trials = importlib.import_module("sca-ldpc_amd.trials")

N, W, R, OMEGA = 499, 7, 260, 5
SEED, FIRST, RUNS, MAX_ITER = 42, 1000, 200, 40  # 200 trials: a ragged fourth tile
STEP = 65
STEPS = (65, 130, 195, 260)
COLUMNS = ("unsatisfied", "good_flips", "bad_flips", "found_bad_satisfied_checks", "found_bad_unsatisfied_checks")
# The f32 CPU oracle on trials 1000 .. 1199, min-sum: successes and the five counters summed over the 200 trials, per number of
# rows (tests/test_hqc_stats.py recomputes them from the oracle); the tanh rule's successes.
MIN_SUM_TABLE = {
    65: (1, 863, 562, 1304, 0, 0),
    130: (13, 1684, 825, 425, 0, 12),
    195: (115, 2551, 967, 118, 1, 49),
    260: (176, 3457, 987, 13, 7, 76),
}
TANH_AT_260 = (175, 3457, 976, 4, 7, 76)
TANH_SUCCESSES = {65: 0, 130: 11, 195: 95, 260: 175}


@functools.lru_cache(maxsize=None)
def code():
    """(first row support, rows): hqc_instance's own draws, so that cuts of its Hin can be built."""
    rng = np.random.RandomState(11)
    sup = S.codes.make_random_ldpc_first_row(N, W, rng)
    rows = rng.permutation(N)[:R]
    Hin = hqc_instance(N, W, R, OMEGA, 0.04, 1, seed=11, flip=False)[1]
    mine = S.codes.hqc_check_graph(sup, N, rows)
    assert np.array_equal(Hin.row_ptr, mine.row_ptr) and np.array_equal(Hin.col_idx, mine.col_idx)
    return sup, rows


@functools.lru_cache(maxsize=None)
def cut(r):
    """(H, Hin, priors) on the first r rows; the check columns' shared priors are replaced per trial."""
    sup, rows = code()
    Hin = S.codes.hqc_check_graph(sup, N, rows[:r])
    return Hin.with_identity(), Hin, np.concatenate([np.full(N, OMEGA / N), np.full(r, 0.04)])


@functools.lru_cache(maxsize=None)
def wrapped_table():
    return trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))


@functools.lru_cache(maxsize=None)
def law(r=R):
    """The NumPy law of trials FIRST .. FIRST + RUNS - 1 on the first r rows (computed once, shared, left unchanged)."""
    return ref.draw(SEED, FIRST, RUNS, cut(r)[1], OMEGA, wrapped_table())


def count(bits, msg, y):
    """driver.hqc_stats per trial -> (success uint8 [k], stats int32 [k, 5])."""
    rows = [driver.hqc_stats(N, bits[i], msg[i, N:], y[i]) for i in range(len(bits))]
    return (np.array([ok for ok, _ in rows], dtype=np.uint8),
            np.array([[st[c] for c in COLUMNS] for _, st in rows], dtype=np.int32).reshape(len(bits), len(COLUMNS)))


@functools.lru_cache(maxsize=None)
def oracle_step(r, method="min_sum", k=RUNS):
    """The answer key on the first r rows: the oracle's decoded words of trials FIRST .. FIRST + k - 1 and their counters."""
    from oracle import pyoracle

    H, _, probs = cut(r)
    d = law(r)
    key = soft_cases.oracle_per_codeword(pyoracle, H, probs, d["probs"][:k], d["msg"][:k], 1, MAX_ITER, method)
    success, stats = count(key["bits"], d["msg"][:k], d["y"][:k])
    return dict(key, success=success, stats=stats)


def table_row(step):
    """(successes, five sums) of an oracle_step / sweep result, in MIN_SUM_TABLE's form."""
    return (int(np.asarray(step["success"]).sum()),) + tuple(int(v) for v in np.asarray(step["stats"], dtype=np.int64).sum(axis=0))


@functools.lru_cache(maxsize=None)
def checks_needed():
    """Per trial the first of STEPS at which the min-sum oracle recovers the key, -1 if none does."""
    ok = np.stack([oracle_step(r)["success"] for r in STEPS]).astype(bool)  # [step, trial]
    return np.where(ok.any(axis=0), np.asarray(STEPS)[ok.argmax(axis=0)], -1).astype(np.int32)
