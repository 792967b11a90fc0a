"""Synthetic HQC attack trials (host side): the inputs `hqc.decode()` assembles
(simulate/hqc.py:678-705), generated without the liboqs oracle.

Trial i (global index, independent of how trials are sharded over GPUs):
    rng   = RandomState(base_seed + i)
    y     = omega distinct positions            (the secret's support)
    c     = Hin y mod 2, each bit flipped with probability eps   (noisy oracle answers)
    msg   = [0]*N ++ c                          (hqc.py:703-705)
    prior = [omega/N]*N ++ [eps]*R              (hqc.py:684-690 with certainty 1-eps)

Kyber attack trials (simulate/kyber.py) are drawn on the device (`QarySpecialDecoder.mc_run_secret`); what the host builds for
them is here: the secret's law (`centered_binomial`) and, per kind of variable, the table of an oracle's answers with the
posterior each answer hands the decoder (`oracle_posterior_table`).
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


def centered_binomial(eta, sum_weight=1):
    """kyber.secret_distribution (simulate/kyber.py:60-64): the law of a sum of `sum_weight` coefficients of the centred binomial
    of parameter eta, float64 [2B+1] with B = sum_weight * eta, index q = value q - B."""
    from math import comb

    B = int(sum_weight) * int(eta)
    if B < 1:
        raise ValueError("eta and sum_weight must be positive")
    n = 2 * B
    den = 2**n
    return np.array([comb(n, q) / den for q in range(n + 1)], dtype=np.float64)


MAX_POSTERIOR_OUTCOMES = 32  # scaldpc_mc_qary_run_secret takes tables of up to 32 outcomes: five oracle bits


def _oracle_bit_law(accuracy, P):
    """pr[i][expected][actual] of oracle bit i: a scalar is max_likelihood.SimpleOracle (right with probability `accuracy`), P
    (false-positive, false-negative) pairs are FalsePositiveNegativePositionalOracle (simulate/max_likelihood.py:9-38), the
    same float64 expressions."""
    if np.ndim(accuracy) == 0:
        p = float(accuracy)
        if not 0.0 <= p <= 1.0:
            raise ValueError("accuracy is a probability")
        return [((p, 1 - p), (1 - p, p))] * P
    pairs = [(float(fp), float(fn)) for fp, fn in accuracy]
    if len(pairs) != P or not all(0.0 <= x <= 1.0 for pair in pairs for x in pair):
        raise ValueError(f"accuracy: one probability, or {P} (false-positive, false-negative) pairs of probabilities")
    return [((1 - fp, fp), (fn, 1 - fn)) for fp, fn in pairs]


def oracle_posterior_table(coding, prior, accuracy, reverse=False):
    """The table of one kind of variable for `QarySpecialDecoder.mc_run_secret`, from the oracle's code:

      coding[s]  the P oracle bits of symbol s (a tuple of 0 / 1, or a single 0 / 1), s = 0 .. Q-1 standing for the value s - B
      prior      float64 [Q], the law of the symbol (`centered_binomial`)
      accuracy   a scalar (SimpleOracle) or P (false-positive, false-negative) pairs (FalsePositiveNegativePositionalOracle)

    An outcome is one of the 2^P answers y, in the order of itertools.product((0, 1), repeat=P):
        weights[s][y] = prod_i Pr[y_i | coding[s][i]]                 (max_likelihood.pr_cond_yx)
        levels[y][s]  = weights[s][y] * prior[s] / sum_s' prior[s'] * weights[s'][y]
    the posterior max_likelihood.s_distribution_from_hard_y gives the decoder for the answer y, in the same order of float64
    operations.  An answer whose probability is 0 under every symbol is dropped (its posterior is 0 / 0 and it is never drawn).
    reverse: the table of the variable t = -s (kyber.get_channel_probabilities reverses the row sums' distributions,
    kyber.py:374-375): the symbol axis of both arrays is reversed.
    Returns dict(levels float64 [K, Q], weights float64 [Q, K], answers [K] tuples).  Raises ValueError beyond 32 outcomes."""
    import itertools

    code = [tuple(int(b) for b in (c if np.ndim(c) else (c,))) for c in coding]
    pr = [float(x) for x in np.asarray(prior, dtype=np.float64).reshape(-1)]
    Q = len(code)
    if Q < 1 or len(pr) != Q:
        raise ValueError("coding and prior: one entry per symbol")
    P = len(code[0])
    if P < 1 or any(len(c) != P or any(b not in (0, 1) for b in c) for c in code):
        raise ValueError("coding: the same number of oracle bits, 0 or 1, for every symbol")
    if 2**P > MAX_POSTERIOR_OUTCOMES:
        raise ValueError(f"{2 ** P} outcomes: scaldpc_mc_qary_run_secret takes up to {MAX_POSTERIOR_OUTCOMES}")
    law = _oracle_bit_law(accuracy, P)
    answers, weights, levels = [], [], []
    for y in itertools.product((0, 1), repeat=P):
        cond = []
        for s in range(Q):
            res = 1
            for i in range(P):
                res *= law[i][code[s][i]][y[i]]
            cond.append(res)
        pr_y = 0
        for s in range(Q):
            pr_y += pr[s] * cond[s]
        if pr_y == 0:
            continue
        answers.append(y)
        weights.append(cond)
        levels.append([cond[s] * pr[s] / pr_y for s in range(Q)])
    if not answers:
        raise ValueError("no answer has a positive probability")
    weights = np.array(weights, dtype=np.float64).T
    levels = np.array(levels, dtype=np.float64)
    if reverse:
        weights, levels = weights[::-1], levels[:, ::-1]
    return dict(levels=np.ascontiguousarray(levels), weights=np.ascontiguousarray(weights), answers=answers)


def hqc_priors(N, R, omega, eps):
    return np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(R, float(eps), dtype=np.float64)])


def success(bits, ys, N):
    """hqc.py:742-749: decoded[:N] must equal the indicator of y."""
    truth = np.zeros((bits.shape[0], N), dtype=np.uint8)
    np.put_along_axis(truth, ys.astype(np.int64), 1, axis=1)
    return (bits[:, :N] == truth).all(axis=1)
