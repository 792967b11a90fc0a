"""Synthetic HQC attack trials (host side): the inputs `hqc.decode()` assembles
(simulate/hqc.py:678-705), generated without the liboqs oracle.

Trial i (global index, independent of how trials are sharded over GPUs):
    rng   = RandomState(base_seed + i)
    y     = omega distinct positions            (the secret's support)
    c     = Hin y mod 2, each bit flipped with probability eps   (noisy oracle answers)
    msg   = [0]*N ++ c                          (hqc.py:703-705)
    prior = [omega/N]*N ++ [eps]*R              (hqc.py:684-690 with certainty 1-eps)
"""
from __future__ import annotations

import numpy as np


def hqc_trials(Hin, omega, eps, count, base_seed=2, first_index=0):
    """Returns (msg uint8 [count, N+R], y_support int32 [count, omega])."""
    N, R = Hin.n, Hin.m
    msg = np.zeros((count, N + R), dtype=np.uint8)
    ys = np.zeros((count, omega), dtype=np.int32)
    col_ptr, csc_row = Hin.col_ptr, Hin.csc_row
    for i in range(count):
        rng = np.random.RandomState(base_seed + first_index + i)
        y = rng.choice(N, omega, replace=False)
        ys[i] = y
        hit = np.concatenate([csc_row[col_ptr[j] : col_ptr[j + 1]] for j in y]) if omega else np.zeros(0, np.int64)
        c = (np.bincount(hit, minlength=R) & 1).astype(np.uint8)
        if eps > 0:
            c ^= (rng.rand(R) < eps).astype(np.uint8)
        msg[i, N:] = c
    return msg, ys


def hqc_soft_trials(Hin, omega, levels, weights, count, base_seed=2, first_index=0):
    """Trials whose checks come with their OWN certainties, as the oracles of simulate/hqc.py hand them out
    (`inner_hqc_decoding_oracle` keys the certainty on the answer, `wrapped_hqc_decoding_oracle` raises it with every
    repeated measurement, hqc.py:782-806).  Trial i, seeded base_seed + first_index + i like `hqc_trials` (same secret):
        y      = omega distinct positions
        cert_r = one of `levels`, drawn with probabilities `weights`, per check
        c      = Hin y mod 2, bit r flipped with probability 1 - cert_r
    Returns (msg uint8 [count, N+R], y_support int32 [count, omega], cert float64 [count, R]); the check priors of
    trial i are 1 - cert[i] (hqc.py:689)."""
    N, R = Hin.n, Hin.m
    levels = np.asarray(levels, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    if levels.ndim != 1 or levels.shape != weights.shape or not ((levels >= 0) & (levels <= 1)).all():
        raise ValueError("levels: certainties in [0, 1]; weights: one probability per level")
    msg = np.zeros((count, N + R), dtype=np.uint8)
    ys = np.zeros((count, omega), dtype=np.int32)
    cert = np.zeros((count, R), dtype=np.float64)
    col_ptr, csc_row = Hin.col_ptr, Hin.csc_row
    for i in range(count):
        rng = np.random.RandomState(base_seed + first_index + i)
        y = rng.choice(N, omega, replace=False)
        ys[i] = y
        hit = np.concatenate([csc_row[col_ptr[j] : col_ptr[j + 1]] for j in y]) if omega else np.zeros(0, np.int64)
        c = (np.bincount(hit, minlength=R) & 1).astype(np.uint8)
        cert[i] = levels[rng.choice(levels.size, R, p=weights / weights.sum())]
        c ^= (rng.rand(R) < 1.0 - cert[i]).astype(np.uint8)
        msg[i, N:] = c
    return msg, ys, cert


MAX_OUTCOMES = 32  # scaldpc_mc_hqc_run_soft takes tables of up to 32 outcomes


def _tries_needed(a, bar):
    """The smallest number of tries with one answer after which wrapped_hqc_decoding_oracle stops on that answer: each such
    try carries certainty `a`, the answer's certainty is 1 - (1 - a)^count (hqc.py:798-800, the same float64 expression:
    1.0 - product of the 1.0 - a), and the loop ends once it reaches `bar` (hqc.py:801).  None: never within MAX_OUTCOMES."""
    miss = 1.0
    for count in range(1, MAX_OUTCOMES + 1):
        miss *= 1.0 - a
        if 1.0 - miss >= bar:
            return count, miss
    return None


def wrapped_oracle_table(accuracy, require=(0.5, 0.5)):
    """The exact outcome table of the reference's WRAPPED oracle (simulate/hqc.py:782-871) for `BpDecoder.mc_hqc_run_soft`.

      accuracy = (a0, a1)  params.EPSILON: a single measurement of a check whose true value is b is right with probability
                           a_b (hqc.py:830-831,864) and reports certainty a_b (hqc.py:870)
      require  = (require_false, require_true)  the bar the certainty of an answer must reach (hqc.py:791,801)

    For true value b the measurement is repeated; answer r is final after k_r(b) tries that gave r, the smallest count with
    1 - (1 - a_b)^count >= require[r].  An outcome is (b, right or wrong, total tries n): the final answer came k times, the
    other one n - k < k_other times, and the last try gave the final answer:
        weight = C(n - 1, n - k) p^k (1 - p)^(n - k),  p = a_b for the right answer, 1 - a_b for the wrong one
        probs  = (1 - a_b)^k   (1 - certainty, what hqc.decode gives the decoder, hqc.py:689)
        costs  = n             oracle calls spent
    Returns dict(weights float64 [2, K], flips uint8 [K], probs float64 [K], costs int32 [K]); row b of `weights` is zero on
    the outcomes of the other true value.  Raises ValueError if more than 32 outcomes result (or an answer can never reach
    its bar)."""
    from math import comb

    a = [float(accuracy[0]), float(accuracy[1])]
    bar = [float(require[0]), float(require[1])]
    if not all(0.0 <= x <= 1.0 for x in a + bar):
        raise ValueError("accuracy and require are probabilities")
    rows = []  # (b, flip, weight, prob, cost)
    for b in (0, 1):
        need = {}
        for wrong in (0, 1):
            p = 1.0 - a[b] if wrong else a[b]
            if p > 0.0:  # (an answer that never comes needs no bar)
                need[wrong] = _tries_needed(a[b], bar[b ^ wrong])
                if need[wrong] is None:
                    raise ValueError(f"true value {b}: the answer {b ^ wrong} never reaches certainty {bar[b ^ wrong]} within {MAX_OUTCOMES} tries")
        for wrong in sorted(need):
            p = 1.0 - a[b] if wrong else a[b]
            k, miss = need[wrong]
            others = need[1 - wrong][0] if 1 - wrong in need else 1  # the other answer never comes: 0 of them, always
            for other in range(others):
                n = k + other
                rows.append((b, wrong, comb(n - 1, other) * p**k * (1.0 - p) ** other, miss, n))
    if len(rows) > MAX_OUTCOMES:
        raise ValueError(f"{len(rows)} outcomes: scaldpc_mc_hqc_run_soft takes up to {MAX_OUTCOMES}")
    K = len(rows)
    weights = np.zeros((2, K), dtype=np.float64)
    for k, (b, _, w, _, _) in enumerate(rows):
        weights[b, k] = w
    return dict(weights=weights, flips=np.array([r[1] for r in rows], dtype=np.uint8),
                probs=np.array([r[3] for r in rows], dtype=np.float64), costs=np.array([r[4] for r in rows], dtype=np.int32))


def levels_table(levels, weights):
    """The law of `hqc_soft_trials` as an outcome table for `BpDecoder.mc_hqc_run_soft`: a check draws certainty levels[l] with
    probability weights[l] (normalised, as there) and is reported wrong with probability 1 - levels[l], whatever its true
    value.  2 K outcomes, level by level (wrong, right); no costs.  A level of certainty 1.0 gives an outcome of weight 0, which
    is never drawn."""
    levels = np.asarray(levels, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    if levels.ndim != 1 or levels.shape != weights.shape or not ((levels >= 0) & (levels <= 1)).all():
        raise ValueError("levels: certainties in [0, 1]; weights: one probability per level")
    if 2 * levels.size > MAX_OUTCOMES:
        raise ValueError(f"{2 * levels.size} outcomes: scaldpc_mc_hqc_run_soft takes up to {MAX_OUTCOMES}")
    w = weights / weights.sum()
    row = np.stack([w * (1.0 - levels), w * levels], axis=1).reshape(-1)
    return dict(weights=np.stack([row, row]), flips=np.tile(np.array([1, 0], dtype=np.uint8), levels.size),
                probs=np.repeat(1.0 - levels, 2), costs=None)


def hqc_priors(N, R, omega, eps):
    return np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(R, float(eps), dtype=np.float64)])


def success(bits, ys, N):
    """hqc.py:742-749: decoded[:N] must equal the indicator of y."""
    truth = np.zeros((bits.shape[0], N), dtype=np.uint8)
    np.put_along_axis(truth, ys.astype(np.int64), 1, axis=1)
    return (bits[:, :N] == truth).all(axis=1)
