"""Shared inputs of tests/test_kernel_matrix.py (CPU) and tests/test_kernel_matrix_gpu.py: small graphs that put the
binary BP kernels' template grid under the oracle by construction.

Which instantiation of a check / variable kernel runs is decided by the graph's MAXIMUM row / column degree (the 16 /
32 / 64 ladder of `with_cap`, csrc/scaldpc_bp.hip), so a cap-16 or cap-32 kernel runs only on a graph whose every row
(column) stays below the line.  Graph (R, C), R and C in {16, 32, 64, 65}: 72 x 200, one designated row of exactly R
edges, one designated column of exactly C edges (not in that row), every other row 2 .. 8 edges, every other column at
most 6.  16 / 32 / 64 sit ON the lines (a `<` for a `<=` in the ladder would show), 65 selects the any-degree forms.
Every graph also holds a block of 35 columns of degree 1, each the last edge of its row (the record form's constant
last edge and slim variable pass), one column in no row and one row with a single edge.

Each graph comes in a second size, 144 x 400 (`tall`), built the same way: the convergence test rides on the next check
pass (the PAR instantiations of the check kernels) only on a graph of at least 129 rows -- 36 words of unsatisfied-check
flags per tile, `pw >= FT_WORDS` in csrc/scaldpc_bp.hip -- which 72 rows do not reach.

Inputs: 65 codewords (two tiles, the second with one live lane), priors uniform in [0.02, 0.2] (min-sum: a tenth of
them exactly 0, so inf - inf = NaN posteriors occur), syndromes of errors drawn at 0, 0.3, 1, 2, 4 times the priors,
9 iterations.  The answer key is the f32 oracle in the kernels' operation order; per-codeword priors: one oracle call
per codeword (`soft_cases.oracle_per_codeword`).  tests/test_kernel_matrix.py checks, without a GPU, that the key is not
vacuous on any graph; SEEDS were searched for that there (the first seed, counted up from 1, that passes for both
update rules)."""
import functools

import numpy as np

from helpers import ORACLE_METHOD, S
from soft_cases import oracle_per_codeword

DEGREES = (16, 32, 64, 65)
GRAPHS = [(R, C) for R in DEGREES for C in DEGREES]
BATCH = 65
EDGE_BATCH = 5
MAX_ITER = 9
SCALES = (0.0, 0.3, 1.0, 2.0, 4.0)
TAIL = 40  # columns of the short per-codeword prior array
METHODS = ("min_sum", "product_sum")
ROW, COL = 0, 0  # the designated row / column
NBLOCK = 35  # degree-1 columns, each the last edge of its row: the last NBLOCK columns; the one before them is in no row


def shape(tall):
    return (144, 400) if tall else (72, 200)


# (R, C, tall) -> seed; see the module docstring
SEEDS = {
    (16, 16, False): 1, (16, 32, False): 3, (16, 64, False): 5, (16, 65, False): 8,
    (32, 16, False): 2, (32, 32, False): 2, (32, 64, False): 3, (32, 65, False): 3,
    (64, 16, False): 4, (64, 32, False): 3, (64, 64, False): 2, (64, 65, False): 12,
    (65, 16, False): 3, (65, 32, False): 5, (65, 64, False): 3, (65, 65, False): 1,
    (16, 16, True): 11, (16, 32, True): 30, (16, 64, True): 1, (16, 65, True): 10,
    (32, 16, True): 4, (32, 32, True): 3, (32, 64, True): 17, (32, 65, True): 16,
    (64, 16, True): 4, (64, 32, True): 2, (64, 64, True): 26, (64, 65, True): 2,
    (65, 16, True): 16, (65, 32, True): 14, (65, 64, True): 8, (65, 65, True): 3,
}  # fmt: skip


def build_dense(R, C, tall, seed):
    M, N = shape(tall)
    block = np.arange(N - NBLOCK, N)
    empty_col = N - NBLOCK - 1
    middle = np.arange(1, empty_col)
    lone_row = M - 1  # the row with a single edge
    rng = np.random.RandomState(1000 * seed + 10 * R + C + (500 if tall else 0))
    H = np.zeros((M, N), dtype=np.int8)
    H[ROW, rng.choice(middle, size=R, replace=False)] = 1
    others = np.arange(1, M - 1)  # the rows between the designated row and the single-edge row
    H[rng.choice(others, size=C, replace=False), COL] = 1
    block_rows = rng.choice(others, size=block.size, replace=False)
    H[block_rows, block] = 1

    def room():
        return middle[H[:, middle].sum(axis=0) < 6]

    for r in others:
        want = max(int(H[r].sum()), rng.randint(2, 9))
        free = np.setdiff1d(room(), np.flatnonzero(H[r]))
        H[r, rng.choice(free, size=want - int(H[r].sum()), replace=False)] = 1
    H[lone_row, rng.choice(room())] = 1
    for c in middle[H[:, middle].sum(axis=0) == 0]:  # exactly ONE column sits in no row
        H[rng.choice(others[H[others].sum(axis=1) < 8]), c] = 1
    rdeg, cdeg = H.sum(axis=1), H.sum(axis=0)
    assert rdeg[ROW] == R and cdeg[COL] == C and H[ROW, COL] == 0
    assert rdeg[others].min() >= 2 and rdeg[others].max() <= 8 and rdeg[lone_row] == 1
    assert cdeg[middle].min() >= 1 and cdeg[middle].max() <= 6
    assert cdeg[empty_col] == 0 and (cdeg[block] == 1).all() and block.size >= 30
    for c in block:  # ... the last edge of its row
        r = int(np.flatnonzero(H[:, c])[0])
        assert np.flatnonzero(H[r])[-1] == c
    assert rdeg.max() == R and cdeg.max() == C
    return H


@functools.lru_cache(maxsize=None)
def graph(R, C, tall=False, seed=None):
    """(TannerGraph, dense H) of graph (R, C)."""
    Hd = build_dense(R, C, tall, SEEDS[(R, C, tall)] if seed is None else seed)
    return S.TannerGraph.from_dense(Hd), Hd


@functools.lru_cache(maxsize=None)
def inputs(R, C, method, tall=False, seed=None):
    """dict(probs float64 [n] shared priors, soft float32 [65, n] per-codeword priors, synd uint8 [65, m])."""
    seed = SEEDS[(R, C, tall)] if seed is None else seed
    G, _ = graph(R, C, tall, seed)
    N = G.n
    rng = np.random.RandomState(7000 * seed + 10 * R + C + (500 if tall else 0))
    probs = rng.uniform(0.02, 0.2, size=N)
    soft = rng.uniform(0.02, 0.2, size=(BATCH, N)).astype(np.float32)
    if method == "min_sum":
        probs[rng.choice(N, size=N // 10, replace=False)] = 0.0
        soft[rng.rand(BATCH, N) < 0.1] = 0.0
    scale = np.array(SCALES)[np.arange(BATCH) % len(SCALES)]
    err = (rng.rand(BATCH, N) < scale[:, None] * probs[None, :]).astype(np.uint8)
    out = {"probs": probs, "soft": soft, "synd": G.syndrome(err)}
    for v in out.values():
        v.setflags(write=False)
    return out


def prior_array(inp, prior):
    """The `channel_probs` argument of a decode: None (shared), the whole [65, n] array, or its last TAIL columns."""
    return {"shared": None, "full": inp["soft"], "tail": inp["soft"][:, -TAIL:]}[prior]


@functools.lru_cache(maxsize=None)
def key(R, C, method, early, prior, nb=BATCH, tall=False, seed=None):
    """The oracle's answer for the first nb codewords of a graph (computed once per session; the knobs of a decode
    never change the answer)."""
    from oracle import pyoracle

    G, _ = graph(R, C, tall, seed)
    inp = inputs(R, C, method, tall, seed)
    synd = inp["synd"][:nb]
    with np.errstate(divide="ignore", invalid="ignore"):
        if prior == "shared":
            ref = pyoracle.bp_decode_batch(G, inp["probs"], synd, 0, MAX_ITER, ORACLE_METHOD[method], dtype="f32", threads=8,
                                           early_exit=early)
        else:
            ref = oracle_per_codeword(pyoracle, G, inp["probs"], prior_array(inp, prior)[:nb], synd, 0, MAX_ITER, method,
                                      early_exit=early)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def vacuous(ref):
    """What the early-exit key of a graph lacks (empty list: nothing).  The key must hold a converged and a stuck
    codeword, at least three distinct iteration counts, a codeword that converges at iteration >= 5 (a fused-test pass
    after the first poll decides something), one that converges at iteration 1, and the lone codeword of the second
    tile must not converge before iteration 3."""
    conv, it = ref["converged"].astype(bool), ref["iters"]
    missing = []
    if not conv.any():
        missing.append("no converged codeword")
    if conv.all():
        missing.append("no stuck codeword")
    if len(set(it.tolist())) < 3:
        missing.append("fewer than three iteration counts")
    if not (conv & (it >= 5)).any():
        missing.append("none converges at iteration >= 5")
    if not (conv & (it == 1)).any():
        missing.append("none converges at iteration 1")
    if conv[BATCH - 1] and it[BATCH - 1] < 3:
        missing.append("the second tile's codeword converges before iteration 3")
    return missing
