"""TEST INFRASTRUCTURE: what tests/test_ref64_mc.py (CPU: the preconditions, on the oracle alone) and tests/test_ref64_mc_gpu.py
(the float64 Monte-Carlo sweeps, scaldpc_mc_*_f64) share.  The instances are mc_ref's F, H1 and H2 with its SEED, FIRST, RUNS and
MAX_ITER -- exactly the inputs ref64_cases.mc_case / mc_oracle decode with the float64 oracle -- and, for the soft sweep, the table
t9 under the law of hqc_soft_mc_ref.draw, the oracle called per codeword with the float64 probabilities of its outcomes.
Every reference is computed once per session and left unchanged."""
import functools
import importlib

import numpy as np

import hqc_soft_mc_ref
import mc_ref
import ref64_cases
from mc_ref import FIRST, MAX_ITER, RUNS, SEED  # noqa: F401  (re-exported)

driver = importlib.import_module("sca-ldpc_amd.driver")
trials = importlib.import_module("sca-ldpc_amd.trials")

SHARED = ("F", "H1", "H2")  # the sweeps on the handle's shared priors
SOFT = ("H1", "H2")  # the sweeps under t9
HANDOVERS = (2, 4)
# (converged, success, running after 2, running after 4) of the float64 oracle with early exit, measured when the tests were
# written; tests/test_ref64_mc.py derives them again from the oracle
PRECONDITIONS = {
    ("F", False): (109, 54, 65, 24),
    ("H1", False): (101, 79, 113, 47),
    ("H2", False): (72, 31, 119, 69),
    ("H1", True): (130, 121, 23, 3),
    ("H2", True): (120, 99, 60, 14),
}


def handed_over(name, soft, k):
    """Trials the hand-over at iteration k takes (0 where there is none: k = 0, k >= MAX_ITER)."""
    return PRECONDITIONS[(name, soft)][2 + HANDOVERS.index(k)] if k in HANDOVERS else 0


@functools.lru_cache(maxsize=None)
def t9():
    """K = 9; its float64 probabilities 0.0004 / 0.01 / 0.001 are no float32 numbers."""
    return trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))


def probs64(table=None):
    return np.asarray((table or t9())["probs"], dtype=np.float64)


def running_after(d, k):
    """Trials with iteration count > k or not converged."""
    return int(((d["iters"] > k) | (d["converged"] == 0)).sum())


# ---------------------------------------------------------------------------------------------------------------- shared priors
@functools.lru_cache(maxsize=None)
def shared_law(name):
    """dict(errors) of F, dict(y, msg) of H1 / H2: the trials FIRST .. FIRST + RUNS - 1."""
    return mc_ref.fer_law() if name == "F" else mc_ref.hqc_law(name)


@functools.lru_cache(maxsize=None)
def shared_oracle(name, early=True):
    """ref64_cases.mc_oracle with the success the sweeps report."""
    d = dict(ref64_cases.mc_oracle(name, early))
    if name == "F":
        d["success"] = (d["bits"] == mc_ref.fer_law()["errors"]).all(axis=1).astype(np.uint8)
    else:
        d["success"] = mc_ref.hqc_success(d["bits"], mc_ref.hqc_law(name)["y"], mc_ref.instance(name)["N"])
    return d


# ------------------------------------------------------------------------------------------------------------------ the soft sweep
@functools.lru_cache(maxsize=None)
def soft_law(name, first=FIRST, runs=RUNS, seed=SEED):
    """hqc_soft_mc_ref.draw under t9, and probs64 float64 [runs, R]: the check priors of every trial, unrounded."""
    i = mc_ref.instance(name)
    d = hqc_soft_mc_ref.draw(seed, first, runs, i["Hin"], i["omega"], t9())
    d["probs64"] = probs64()[d["outcome"]]
    return d


def count(N, bits, msg, y):
    """(success uint8 [runs], stats int32 [runs, 5]): driver.hqc_stats on every decoded word."""
    rows = [driver.hqc_stats(N, bits[i], msg[i, N:], y[i]) for i in range(len(bits))]
    return (np.array([ok for ok, _ in rows], dtype=np.uint8),
            np.array([[st[c] for c in driver.HQC_STATS_COLUMNS] for _, st in rows], dtype=np.int32).reshape(len(bits), 5))


def soft_decode(H, N, omega, law, early=True, max_iter=MAX_ITER, dtype="f64"):
    """The oracle per codeword on H = [Hin | I], every one with the probabilities of its own outcomes on the check columns
    (float64: as they are; f32: the fp32 kernels' order on the rounded values) and omega / N below:
    dict(bits, iters, converged, success, stats)."""
    from oracle import pyoracle

    method = "product_sum" if dtype == "f64" else "tanh_complement"
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(len(law["msg"])):
            tail = law["probs64"][b] if dtype == "f64" else law["probs64"][b].astype(np.float32).astype(np.float64)
            probs = np.concatenate([np.full(N, omega / N), tail])
            out.append(pyoracle.bp_decode_batch(H, probs, law["msg"][b : b + 1], 1, max_iter, method, dtype=dtype, threads=1,
                                                early_exit=early))
    d = {k: np.concatenate([o[k] for o in out]) for k in ("bits", "iters", "converged")}
    d["success"], d["stats"] = count(N, d["bits"], law["msg"], law["y"])
    return d


@functools.lru_cache(maxsize=None)
def soft_oracle(name, early=True, dtype="f64"):
    i = mc_ref.instance(name)
    assert np.array_equal(i["probs"][: i["N"]], np.full(i["N"], i["omega"] / i["N"]))
    return soft_decode(i["H"], i["N"], i["omega"], soft_law(name), early, dtype=dtype)


# ------------------------------------------------------------------------------------------------------ H2's graph, row by row
CURVE_STEP = 10
CURVE_STEPS = (10, 20, 30, 40, 50, 60, 70)


@functools.lru_cache(maxsize=None)
def h2_code():
    """(first row support, rows) of H2: hqc_instance's own draws, so that its Hin can be built row by row."""
    from helpers import S

    i = mc_ref.instance("H2")
    rng = np.random.RandomState(11)
    sup = S.codes.make_random_ldpc_first_row(i["N"], 5, rng)
    rows = rng.permutation(i["N"])[: i["R"]]
    mine = S.codes.hqc_check_graph(sup, i["N"], rows)
    assert np.array_equal(i["Hin"].row_ptr, mine.row_ptr) and np.array_equal(i["Hin"].col_idx, mine.col_idx)
    return sup, rows


@functools.lru_cache(maxsize=None)
def h2_cut(r):
    """(H, Hin) on H2's first r rows."""
    from helpers import S

    sup, rows = h2_code()
    Hin = S.codes.hqc_check_graph(sup, mc_ref.instance("H2")["N"], rows[:r])
    return Hin.with_identity(), Hin


@functools.lru_cache(maxsize=None)
def h2_cut_law(r):
    i = mc_ref.instance("H2")
    d = hqc_soft_mc_ref.draw(SEED, FIRST, RUNS, h2_cut(r)[1], i["omega"], t9())
    d["probs64"] = probs64()[d["outcome"]]
    return d


@functools.lru_cache(maxsize=None)
def h2_cut_oracle(r, dtype="f64", max_iter=MAX_ITER):
    """Trials FIRST .. FIRST + RUNS - 1 under t9 on H2's first r rows, decoded per codeword."""
    i = mc_ref.instance("H2")
    return soft_decode(h2_cut(r)[0], i["N"], i["omega"], h2_cut_law(r), True, max_iter, dtype)


def curve_key(dtype="f64"):
    """checks_needed int32 [RUNS] and successes per step of the attack curve on H2's rows, from the per-step oracle decodes."""
    ok = np.stack([h2_cut_oracle(r, dtype)["success"] for r in CURVE_STEPS]).astype(bool)
    return np.where(ok.any(axis=0), np.asarray(CURVE_STEPS)[ok.argmax(axis=0)], -1).astype(np.int32), ok.sum(axis=1)
