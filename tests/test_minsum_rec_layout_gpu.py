"""The record form of min-sum on the tile kernels keeps NOTHING per edge in its check pass: per row and tile the two
magnitudes, one arg-min byte per codeword (the index in the row of the first edge that attains the minimum) and one
parity mask; the sign masks are the variable pass's own, per column, taken from the floats it stores (`x <= 0` as a float
compare).  The first record-form check pass of a group in a call -- iteration 2, whatever ran iteration 1 -- also writes
the sign masks a variable pass would have left (its bootstrap form).

Every test here runs the tile kernels (path="stream"), asserts that the record form is what ran, and compares hard
decisions, iteration counts, converged flags and posteriors BIT FOR BIT with the f32 oracle (min-sum) and with the same
decoder in the message form (minsum_rec = 0)."""
import importlib

import numpy as np
import pytest

from helpers import S, hqc_instance, staircase_graph
from soft_cases import oracle_per_codeword

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

KEYS = ("bits", "llr", "iters", "converged")


def same(a, b, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]).astype(np.asarray(b[k]).dtype), b[k], equal_nan=(k == "llr")), (what, k)


def take(res, n):
    return {k: res[k][:n] for k in KEYS}


def new_decoder(graph, probs, max_iter, rec, alpha=1.0, group=0, **knobs):
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(graph, max_iter=max_iter, bp_method="min_sum", channel_probs=probs, ms_scaling_factor=alpha)
    dec.configure(path="stream", minsum_rec=rec, **knobs)
    dec.set_tile_group(group)
    return dec


def decode(graph, probs, x, kind, max_iter, early, rec, alpha=1.0, group=0, soft=None, **knobs):
    dec = new_decoder(graph, probs, max_iter, rec, alpha, group, **knobs)
    got = dec.decode_batch(x, early_exit=early, want_llr=True, input_vector_type=kind, channel_probs=soft)
    assert dec.time_kernels(2)["record_form"] is bool(rec)  # the form that ran is the one asked for
    dec.close()
    return got


def key(oracle, graph, probs, x, kind, max_iter, early, alpha=1.0):
    with np.errstate(divide="ignore", invalid="ignore"):
        return oracle.bp_decode_batch(graph, probs, x, 1 if kind == "received_vector" else 0, max_iter, "min_sum", alpha=alpha,
                                      dtype="f32", threads=8, early_exit=early)


@pytest.fixture(scope="module")
def hqc():
    """An HQC-shaped [Hin | I] of 200 x 901 with noisy checks, 256 trials; oracle results computed once per setting."""
    H, Hin, probs, msg, _ = hqc_instance(701, 9, 200, 6, 0.03, 256, seed=91)
    return {"H": H, "Hin": Hin, "probs": probs, "msg": msg, "refs": {}}


def hqc_key(oracle, hqc, max_iter, early):
    if (max_iter, early) not in hqc["refs"]:
        hqc["refs"][(max_iter, early)] = key(oracle, hqc["H"], hqc["probs"], hqc["msg"], "received_vector", max_iter, early)
    return hqc["refs"][(max_iter, early)]


def test_staircase_every_degree(oracle):
    """Rows of every degree 1 .. 64, columns of every degree 1 .. 32 and an identity block: the straight-line code of
    every exact-degree instantiation of both kernels (and of the bootstrap check pass), two tiles, the last ragged."""
    rng = np.random.RandomState(2601)
    _, Hd = staircase_graph(rng, rows_per_degree=2, colmax=32, fillers=500)  # rows of degree 1 .. 64, 128 of them
    m = Hd.shape[0]
    ident = np.eye(m, dtype=np.int8)[:, Hd.sum(axis=1) < 64]  # an identity column for every row that has room for its edge
    Hd = np.concatenate([Hd, ident], axis=1)
    Hd = np.concatenate([Hd, np.zeros((2, Hd.shape[1]), dtype=np.int8)], axis=0)
    Hd[m:, 40] = 1  # two rows of degree 1 (on a filler column), which the identity block took away
    G = S.TannerGraph.from_dense(Hd)
    rdeg, cdeg = Hd.sum(axis=1), Hd.sum(axis=0)
    assert set(rdeg) == set(range(1, 65)) and set(range(1, 33)) <= set(cdeg) and cdeg.max() == 32
    probs = rng.uniform(0.01, 0.2, size=G.n)
    batch, iters = 70, 6
    scale = np.array([0.0, 0.03, 0.1, 0.3, 1.0])[np.arange(batch) % 5]
    synd = G.syndrome((rng.rand(batch, G.n) < probs[None, :] * scale[:, None]).astype(np.uint8))
    for early in (False, True):
        ref = key(oracle, G, probs, synd, "syndrome", iters, early)
        got = decode(G, probs, synd, "syndrome", iters, early, 1)
        same(got, ref, ("oracle", early))
        same(got, decode(G, probs, synd, "syndrome", iters, early, 0), ("message form", early))


def regular_3_6(rng, n):
    """A (3,6)-regular graph: three layers, each a random partition of the columns into rows of six."""
    m = n // 2
    while True:
        H = np.zeros((m, n), dtype=np.int8)
        for layer in range(3):
            perm = rng.permutation(n)
            for r in range(n // 6):
                H[layer * (n // 6) + r, perm[6 * r : 6 * r + 6]] = 1
        if (H.sum(axis=1) == 6).all() and (H.sum(axis=0) == 3).all():
            return H


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("certain", [False, True])
def test_ties_and_zeros(oracle, p, certain):
    """All priors equal.  p = 0.5: every message is exactly +0, which `x <= 0` counts as negative (a sign-bit test would
    not).  p = 0.1: every |x| of a row is the same, so the arg-min is a tie over the whole row and goes to the first
    edge.  certain: priors of p = 0 (LLR +inf) on some columns -- all six of row 0 among them, so that row has lanes in
    which NO edge attains the clamped minimum -- and inf - inf = NaN messages downstream."""
    rng = np.random.RandomState(77)
    Hd = regular_3_6(rng, 96)
    G = S.TannerGraph.from_dense(Hd)
    probs = np.full(G.n, p)
    if certain:
        probs[np.flatnonzero(Hd[0])] = 0.0
        probs[rng.choice(G.n, 8, replace=False)] = 0.0
    batch, iters = 70, 8
    synd = G.syndrome((rng.rand(batch, G.n) < 0.05).astype(np.uint8))
    for early in (False, True):
        for alpha in (1.0, 0.75):
            ref = key(oracle, G, probs, synd, "syndrome", iters, early, alpha)
            got = decode(G, probs, synd, "syndrome", iters, early, 1, alpha)
            same(got, ref, ("oracle", early, alpha))
            same(got, decode(G, probs, synd, "syndrome", iters, early, 0, alpha), ("message form", early, alpha))


@pytest.mark.parametrize("batch", [64, 192, 256])
def test_launch_geometry(oracle, hqc, batch):
    """One to four tiles in groups of 1, 2, 3 and 4, on one and two stream lanes: XCD-aware tile placement taken (2, 4)
    and not (1, 3), sub-groups at a tile offset inside the group's arrays, lanes of unequal size (3 tiles: 2 + 1), and
    fixed-iteration passes that leave out the identity block's columns (their sign masks are the bootstrap pass's)."""
    iters = 8
    x = hqc["msg"][:batch]
    for early in (False, True):
        ref = take(hqc_key(oracle, hqc, iters, early), batch)
        msgform = decode(hqc["H"], hqc["probs"], x, "received_vector", iters, early, 0)
        same(msgform, ref, ("message form vs oracle", early))
        for split in (1, 2):
            for group in (1, 2, 3, 4):
                got = decode(hqc["H"], hqc["probs"], x, "received_vector", iters, early, 1, group=group, split=split)
                same(got, ref, ("oracle", early, split, group))
                same(got, msgform, ("message form", early, split, group))


def test_early_exit_forms(oracle, hqc):
    """Early exit with the convergence test riding on the record check pass and stand-alone, iteration 1 with and without
    its check pass, with and without the compact pass over stragglers: every combination reaches the record form at
    iteration 2 and bootstraps there (compaction levels included)."""
    iters, batch = 20, 200
    x = hqc["msg"][:batch]
    ref = take(hqc_key(oracle, hqc, iters, True), batch)
    assert len(np.unique(ref["iters"])) > 3  # a spread of iteration counts
    for ft in (0, 1):
        for ff in (0, 1):
            for compact in (0, 2):
                knobs = dict(fuse_test=ft, first_fused=ff, compact_after=compact, group=2)
                got = decode(hqc["H"], hqc["probs"], x, "received_vector", iters, True, 1, **knobs)
                same(got, ref, ("oracle", ft, ff, compact))
                same(got, decode(hqc["H"], hqc["probs"], x, "received_vector", iters, True, 0, **knobs), ("message form", ft, ff, compact))


def test_soft_call(oracle, hqc):
    """A call with per-codeword priors runs iteration 1 WITH its check pass, in the message form: the record form starts
    at iteration 2, behind k_var, and bootstraps there."""
    rng = np.random.RandomState(5)
    iters, batch = 12, 70
    R = hqc["Hin"].m
    x = hqc["msg"][:batch]
    cp = rng.uniform(0.005, 0.2, size=(batch, R)).astype(np.float32)
    for early in (True, False):
        ref = oracle_per_codeword(oracle, hqc["H"], hqc["probs"], cp, x, 1, iters, "min_sum", early_exit=early)
        got = decode(hqc["H"], hqc["probs"], x, "received_vector", iters, early, 1, soft=cp)
        same(got, ref, ("oracle", early))
        same(got, decode(hqc["H"], hqc["probs"], x, "received_vector", iters, early, 0, soft=cp), ("message form", early))


def test_timing_entry_leaves_state(oracle, hqc):
    """scaldpc_bp_time_kernels runs on the state a decode left behind (sign masks current) and never bootstraps; the
    decode after it starts over and equals the first."""
    iters, batch = 8, 192
    x = hqc["msg"][:batch]
    for early in (False, True):
        dec = new_decoder(hqc["H"], hqc["probs"], iters, 1)
        a = dec.decode_batch(x, early_exit=early, want_llr=True)
        t = dec.time_kernels(3)
        assert t["record_form"] is True
        b = dec.decode_batch(x, early_exit=early, want_llr=True)
        dec.close()
        same(b, a, ("second decode", early))
        same(a, take(hqc_key(oracle, hqc, iters, early), batch), ("oracle", early))


def test_growing_graph(oracle):
    """Rows appended to a live decoder: the row words (row + index in the row), records and masks are rebuilt for the
    grown graph; the result is a freshly built decoder's and the oracle's."""
    H, Hin, probs, msg, _ = hqc_instance(701, 9, 160, 6, 0.03, 100, seed=92)
    N, iters = 701, 10

    def graph(r):
        rp = Hin.row_ptr[: r + 1]
        cols = np.concatenate([Hin.col_idx[: rp[-1]].reshape(r, -1), N + np.arange(r, dtype=np.int32)[:, None]], axis=1)
        return S.TannerGraph.from_csr(r, N + r, np.arange(r + 1, dtype=np.int64) * cols.shape[1], cols.reshape(-1))

    ref = key(oracle, H, probs, msg, "received_vector", iters, True)
    outs = {}
    for rec in (1, 0):
        dec = new_decoder(graph(150), probs[: N + 150], iters, rec)
        dec.decode_batch(msg[:, : N + 150], early_exit=True, want_llr=True)
        g = graph(160)
        e0 = g.row_ptr[150]
        dec.append_rows(g.row_ptr[150:] - e0, g.col_idx[e0:], N + 160, probs[N + 150 :])
        outs[rec] = dec.decode_batch(msg, early_exit=True, want_llr=True)
        assert dec.time_kernels(2)["record_form"] is bool(rec)
        dec.close()
    fresh = decode(graph(160), probs, msg, "received_vector", iters, True, 1)
    same(outs[1], ref, "oracle")
    same(outs[1], fresh, "fresh decoder")
    same(outs[1], outs[0], "message form")
