"""The records of the min-sum record form carry the row's parity in their SIGN BIT -- per row and codeword the two floats
+-m1 * alpha and +-m2 * alpha, negative where the syndrome bit XOR the signs of the row's inputs is odd -- and the variable
pass rebuilds a message as (arg-min byte == edge ? second : first) with the sign bit XORed with the column's own sign mask.  That
must be the float `negative ? -m : m` of the message form bit for bit, the sign of a zero and of FLT_MAX included.

Every test runs the tile kernels on a small graph (path="stream"), at batch 70 and 192 in groups of 3 tiles on two stream
lanes (two and three tiles, a ragged last tile, a lane at a tile offset), for 2, 3 and 8 fixed iterations and 8 with early
exit, alpha 1 and 0.75, and compares hard decisions, posteriors, iteration counts and flags with the f32 oracle
(np.array_equal) and with the same build in the message form (minsum_rec = 0; posteriors as uint32 bit patterns there,
because array_equal cannot see the sign of a zero)."""
import importlib

import numpy as np
import pytest

from helpers import S, staircase_graph

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

KEYS = ("bits", "llr", "iters", "converged")
SETTINGS = [(2, False), (3, False), (8, False), (8, True)]  # (iterations, early exit)
ALPHAS = (1.0, 0.75)
BATCHES = (70, 192)


def decode(graph, probs, synd, max_iter, early, rec, alpha):
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(graph, max_iter=max_iter, bp_method="min_sum", channel_probs=probs, ms_scaling_factor=alpha)
    dec.configure(path="stream", minsum_rec=rec, split=2)
    dec.set_tile_group(3)
    got = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome")
    assert dec.time_kernels(2)["record_form"] is bool(rec)  # the form that ran is the one asked for
    dec.close()
    return got


def hold_to_oracle_and_message_form(oracle, graph, probs, synd):
    """`synd`: 192 syndromes; batch 70 is its first 70 rows (the oracle decodes codewords independently: computed once)."""
    assert len(synd) == max(BATCHES)
    for max_iter, early in SETTINGS:
        for alpha in ALPHAS:
            with np.errstate(divide="ignore", invalid="ignore"):
                ref = oracle.bp_decode_batch(graph, probs, synd, 0, max_iter, "min_sum", alpha=alpha, dtype="f32", threads=8,
                                             early_exit=early)
            for batch in BATCHES:
                what = (max_iter, early, alpha, batch)
                got = decode(graph, probs, synd[:batch], max_iter, early, 1, alpha)
                msgform = decode(graph, probs, synd[:batch], max_iter, early, 0, alpha)
                for k in KEYS:
                    want = np.asarray(ref[k])[:batch]
                    assert np.array_equal(np.asarray(got[k]).astype(want.dtype), want, equal_nan=(k == "llr")), ("oracle", what, k)
                    assert np.array_equal(np.asarray(got[k]), np.asarray(msgform[k]), equal_nan=(k == "llr")), ("message form", what, k)
                a = np.ascontiguousarray(got["llr"], dtype=np.float32).view(np.uint32)
                b = np.ascontiguousarray(msgform["llr"], dtype=np.float32).view(np.uint32)
                assert np.array_equal(a, b), ("message form, posterior bit patterns", what)


def regular_3_6(rng, n):
    """A (3,6)-regular graph: three layers, each a random partition of the columns into rows of six."""
    H = np.zeros((n // 2, n), dtype=np.int8)
    for layer in range(3):
        perm = rng.permutation(n)
        for r in range(n // 6):
            H[layer * (n // 6) + r, perm[6 * r : 6 * r + 6]] = 1
    assert (H.sum(axis=1) == 6).all() and (H.sum(axis=0) == 3).all()
    return H


def test_signed_zeros_next_to_nonzeros(oracle):
    """Half the columns have p = 0.5 exactly (LLR +0), the rest p in [0.01, 0.2]; random syndromes, so the parity differs
    lane by lane within a wave: records of -0.0 and +0.0 in one row, and `x <= 0` on exact zeros."""
    rng = np.random.RandomState(4101)
    Hd = regular_3_6(rng, 96)
    G = S.TannerGraph.from_dense(Hd)
    probs = rng.uniform(0.01, 0.2, size=G.n)
    probs[rng.permutation(G.n)[: G.n // 2]] = 0.5
    synd = (rng.rand(max(BATCHES), G.m) < 0.5).astype(np.uint8)
    assert len({tuple(s) for s in synd[:64].T}) > 1  # rows whose syndrome bits differ inside the first wave
    hold_to_oracle_and_message_form(oracle, G, probs, synd)


def test_certainties(oracle):
    """p = 0 (LLR +inf) on all six columns of row 0 and on 8 further columns: FLT_MAX records that carry a parity sign,
    rows in which no edge attains the clamped minimum (REC_NO_ARG), and inf - inf = NaN downstream in the same places."""
    rng = np.random.RandomState(4102)
    Hd = regular_3_6(rng, 96)
    G = S.TannerGraph.from_dense(Hd)
    probs = rng.uniform(0.01, 0.2, size=G.n)
    row0 = np.flatnonzero(Hd[0])
    assert len(row0) == 6
    probs[row0] = 0.0
    probs[rng.choice(np.setdiff1d(np.arange(G.n), row0), 8, replace=False)] = 0.0
    synd = (rng.rand(max(BATCHES), G.m) < 0.5).astype(np.uint8)
    hold_to_oracle_and_message_form(oracle, G, probs, synd)


TARGET_DEGREES = (1, 2, 8, 9, 15, 16, 17, 24, 25, 31, 32)


def staircase_with_separate_columns(rng):
    """helpers.staircase_graph (colmax = 32), with the staircase columns of TARGET_DEGREES re-seated on rows of their own:
    no two of them share a row (their 180 edges need 180 of the graph's rows; the generator seats staircase columns
    wherever a row has room).  A row that lost its only edge is seated first; every row keeps 1 .. 64 edges."""
    _, H = staircase_graph(rng, rows_per_degree=4, colmax=32, fillers=600)
    H = H.copy()
    H[:, list(TARGET_DEGREES)] = 0  # (staircase column k is column k)
    deg = H.sum(axis=1)
    free = [r for r in rng.permutation(H.shape[0]) if deg[r] < 64]
    free.sort(key=lambda r: deg[r] != 0)  # rows left without an edge come first (stable: the rest stay shuffled)
    assert len(free) >= sum(TARGET_DEGREES)
    for k in TARGET_DEGREES:
        rows, free = free[:k], free[k:]
        H[rows, k] = 1
    H = H[H.sum(axis=1) > 0]  # (no row without an edge is left unless it was seated; belt and braces)
    return H


def test_second_magnitude_at_every_position(oracle):
    """One column each of degree 1, 2, 8, 9, 15, 16, 17, 24, 25, 31 and 32 with prior 0.45 (|LLR| 0.2) against <= 0.05
    (|LLR| >= 2.9) everywhere else, no two of them in one row: such a column is the smallest input of every row it touches
    wherever its message stays near its prior, so its edges -- the first and the last edge of a column, the edges on either
    side of the 16 a column record carries inline -- take the second magnitude, the rest of the row the first."""
    rng = np.random.RandomState(4103)
    Hd = staircase_with_separate_columns(rng)
    cols = list(TARGET_DEGREES)
    assert (Hd[:, cols].sum(axis=0) == np.array(TARGET_DEGREES)).all()
    assert (Hd[:, cols].sum(axis=1) <= 1).all()  # no two of them share a row
    rdeg, cdeg = Hd.sum(axis=1), Hd.sum(axis=0)
    assert rdeg.min() >= 1 and rdeg.max() <= 64 and cdeg.max() == 32
    G = S.TannerGraph.from_dense(Hd)
    probs = rng.uniform(0.01, 0.05, size=G.n)
    probs[cols] = 0.45
    err = (rng.rand(max(BATCHES), G.n) < probs[None, :] * 0.5).astype(np.uint8)
    err[::5] = 0  # (codewords with an all-zero syndrome among them)
    hold_to_oracle_and_message_form(oracle, G, probs, G.syndrome(err))
