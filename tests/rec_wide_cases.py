"""Shared inputs of tests/test_rec_wide.py (CPU) and tests/test_rec_wide_gpu.py: the min-sum record form on columns of 33
to 64 edges (`minsum_rec = 2`, csrc/scaldpc_bp.hip: rec_form, launch_var; csrc/scaldpc_bp_kernels.h: var_col_rec_wide).

  matrix     graphs of tests/kernel_matrix_cases.py with the designated column at 33, 48, 63 and 64 edges (one past the
             line of the narrow kernels, the middle of the third chunk of 16, one short of the cap, the cap) and (64, 64);
             past the cap (16, 65) and (65, 48).  SEEDS: per graph and size the first seed, counted up from 1, whose
             early-exit min-sum key is not vacuous (`kernel_matrix_cases.vacuous`) for ALL THREE prior sources -- shared,
             per codeword [65, n], [65, 40]; seed 1 passes on every one of them, the two graphs past the cap included.
  staircase  `helpers.staircase_graph(RandomState(5), colmax=64)`: one column of every degree 0 .. 64.
  settle     an HQC-shaped [Hin | I] with one column of 40 edges, 130 codewords: the first tile holds easy trials and
             freezes, the second holds syndromes of heavy errors and never does.
"""
import functools
import types

import numpy as np

import settle_ref
from helpers import S, staircase_graph

WIDE = [(16, 33), (16, 48), (16, 63), (16, 64), (64, 64)]
PAST = [(16, 65), (65, 48)]  # a column / a row past 64: not the record form, whatever the knob
SEEDS = {(R, C, tall): 1 for R, C in WIDE + PAST for tall in (False, True)}


# ---- every exact degree ----------------------------------------------------------------------------------------------
STAIR_BATCH, STAIR_ITER = 130, 9


@functools.lru_cache(maxsize=None)
def staircase():
    """(graph, dense H, priors with a tenth at p = 0, syndromes of errors at 0, 0.5, 1, 1.5, 2 times the priors)."""
    rng = np.random.RandomState(5)
    G, Hd = staircase_graph(rng, colmax=64)
    probs = rng.uniform(0.02, 0.2, size=G.n)
    probs[rng.choice(G.n, size=G.n // 10, replace=False)] = 0.0
    scale = 0.5 * (np.arange(STAIR_BATCH) % 5)
    err = (rng.rand(STAIR_BATCH, G.n) < scale[:, None] * probs[None, :]).astype(np.uint8)
    synd = G.syndrome(err)
    for a in (Hd, probs, synd):
        a.setflags(write=False)
    return G, Hd, probs, synd


@functools.lru_cache(maxsize=None)
def staircase_key(early):
    from oracle import pyoracle

    G, _, probs, synd = staircase()
    with np.errstate(divide="ignore", invalid="ignore"):
        return pyoracle.bp_decode_batch(G, probs, synd, 0, STAIR_ITER, "min_sum", dtype="f32", threads=8, early_exit=early)


# ---- settle and sweeps -----------------------------------------------------------------------------------------------
SETTLE_N, SETTLE_R, SETTLE_WIDE = 260, 150, 40
SETTLE_OMEGA, SETTLE_EPS = 3, 0.02
SETTLE_BATCH, SETTLE_ITER = 130, 30
SETTLE_SEED = 1  # the first seed, counted up from 1, at which a tile freezes and another does not (tests/test_rec_wide.py)


def settle_dense(seed):
    """Hin, 150 x 260: about 3 % ones, column 0 with exactly 40, every row at least two."""
    rng = np.random.RandomState(4100 + seed)
    H = (rng.rand(SETTLE_R, SETTLE_N) < 0.03).astype(np.int8)
    H[:, 0] = 0
    H[rng.choice(SETTLE_R, size=SETTLE_WIDE, replace=False), 0] = 1
    for r in range(SETTLE_R):
        while H[r].sum() < 2:
            H[r, 1 + rng.randint(SETTLE_N - 1)] = 1
    assert H[:, 0].sum() == SETTLE_WIDE and H[:, 1:].sum(axis=0).max() <= 16
    return H


@functools.lru_cache(maxsize=None)
def settle_case(seed=SETTLE_SEED):
    """H = [Hin | I], its priors, 130 syndromes (tile 0: trials by the sweep's law; tile 1: syndromes of 40 errors among the
    first N columns and a quarter of the checks flipped; tile 2: two more trials), and settle_ref's run of them."""
    trials = settle_ref.trials
    Hin = S.TannerGraph.from_dense(settle_dense(seed))
    H = Hin.with_identity()
    probs = trials.hqc_priors(SETTLE_N, SETTLE_R, SETTLE_OMEGA, SETTLE_EPS)
    msg, _ = trials.hqc_trials(Hin, SETTLE_OMEGA, SETTLE_EPS, SETTLE_BATCH, base_seed=seed)
    synd = np.ascontiguousarray(msg[:, SETTLE_N:])
    rng = np.random.RandomState(4200 + seed)
    y = np.zeros((64, SETTLE_N), dtype=np.uint8)
    for b in range(64):
        y[b, rng.choice(SETTLE_N, size=40, replace=False)] = 1
    synd[64:128] = Hin.syndrome(y) ^ (rng.rand(64, SETTLE_R) < 0.25).astype(np.uint8)
    synd.setflags(write=False)
    out = settle_ref.run(H, settle_ref.prior_llr(probs), synd, SETTLE_ITER, 1.0)
    return types.SimpleNamespace(H=H, Hin=Hin, probs=probs, synd=synd, alpha=1.0, first=settle_ref.first_test(1.0, SETTLE_ITER),
                                 **out)


HORIZON_BATCH = 9 * 64 + 2  # ten tiles, the last with two codewords: every one of them freezes, so a call learns a horizon
HORIZON_ITER = 50  # (a horizon K is learned only with 2 K < max_iter: settle_next_horizon)
HORIZON_TRIALS = 4000  # base seed of the trials: 1000, 2000, ... counted up, the first at which EVERY tile freezes


@functools.lru_cache(maxsize=None)
def horizon_case(seed=SETTLE_SEED):
    """The settle graph with HORIZON_BATCH trials by the sweep's law alone (no hard tile), and settle_ref's run of them."""
    c = settle_case(seed)
    msg, _ = settle_ref.trials.hqc_trials(c.Hin, SETTLE_OMEGA, SETTLE_EPS, HORIZON_BATCH, base_seed=HORIZON_TRIALS)
    synd = np.ascontiguousarray(msg[:, SETTLE_N:])
    synd.setflags(write=False)
    out = settle_ref.run(c.H, settle_ref.prior_llr(c.probs), synd, HORIZON_ITER, 1.0)
    return types.SimpleNamespace(H=c.H, Hin=c.Hin, probs=c.probs, synd=synd, alpha=1.0, first=c.first, **out)


@functools.lru_cache(maxsize=None)
def horizon_key(seed=SETTLE_SEED):
    from oracle import pyoracle

    c = horizon_case(seed)
    return pyoracle.bp_decode_batch(c.H, c.probs, c.synd, 0, HORIZON_ITER, "min_sum", alpha=1.0, dtype="f32", threads=8,
                                    early_exit=False)


@functools.lru_cache(maxsize=None)
def settle_key(seed=SETTLE_SEED):
    from oracle import pyoracle

    c = settle_case(seed)
    return pyoracle.bp_decode_batch(c.H, c.probs, c.synd, 0, SETTLE_ITER, "min_sum", alpha=1.0, dtype="f32", threads=8,
                                    early_exit=False)
