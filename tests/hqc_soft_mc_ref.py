"""TEST INFRASTRUCTURE: the trial law of scaldpc_mc_hqc_run_soft (include/scaldpc.h) restated in NumPy, on the Philox words and
the secret of oracle/mc_oracle.c, and the tables the CPU and GPU tests of the entry share.  Thresholds and words are those of
tests/qary_mc_ref.py: the two entries draw by one rule."""
import numpy as np

from oracle import pyoracle
from qary_mc_ref import thresholds, words  # noqa: F401  (re-exported)


def outcomes_of(w, true_bits, weights):
    """Per check the smallest k with word < T^b_k, b the check's true bit; w, true_bits: [..., R]; weights [2, K]."""
    T = np.array([thresholds(weights[0]), thresholds(weights[1])], dtype=np.uint64)
    sel = T[np.asarray(true_bits, dtype=np.int64)]  # [..., R, K]
    return (np.asarray(w, dtype=np.uint64)[..., None] < sel).argmax(axis=-1).astype(np.uint8)


def eps_table(eps):
    """The K = 2 table that is scaldpc_mc_hqc_run(eps): outcome 0 = "flipped", drawn below floor(eps 2^32) whatever the true bit."""
    return dict(weights=np.array([[eps, 1.0 - eps]] * 2), flips=np.array([1, 0], dtype=np.uint8), probs=np.array([eps, eps]),
                costs=None)


def draw(seed, first, batch, Hin, omega, table):
    """The inputs and counters of trials first .. first + batch - 1: dict(y int32 [batch, omega], outcome uint8 [batch, R],
    msg uint8 [batch, N + R], probs float32 [batch, R] (the check priors of every trial), flips, cost int64 [batch] (cost None
    without costs in the table))."""
    N, R = Hin.n, Hin.m
    y = pyoracle.mc_hqc_secret(seed, first, batch, N, omega)
    yv = np.zeros((batch, N), dtype=np.uint8)
    if omega:
        np.put_along_axis(yv, y.astype(np.int64), 1, axis=1)
    c = Hin.syndrome(yv)
    out = outcomes_of(words(seed, first, batch, R), c, np.asarray(table["weights"], dtype=np.float64))
    fl = np.asarray(table["flips"], dtype=np.uint8)[out]
    msg = np.concatenate([np.zeros((batch, N), dtype=np.uint8), c ^ fl], axis=1)
    costs = table.get("costs")
    return dict(y=y, outcome=out, msg=msg, probs=np.asarray(table["probs"], dtype=np.float32)[out],
                flips=fl.sum(axis=1, dtype=np.int64),
                cost=None if costs is None else np.asarray(costs, dtype=np.int64)[out].sum(axis=1))
