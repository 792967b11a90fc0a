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


def hqc_priors(N, R, omega, eps):
    return np.concatenate([np.full(N, omega / N, dtype=np.float64), np.full(R, float(eps), dtype=np.float64)])


def success(bits, ys, N):
    """hqc.py:742-749: decoded[:N] must equal the indicator of y."""
    truth = np.zeros((bits.shape[0], N), dtype=np.uint8)
    np.put_along_axis(truth, ys.astype(np.int64), 1, axis=1)
    return (bits[:, :N] == truth).all(axis=1)
