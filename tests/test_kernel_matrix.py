"""The answer key of tests/test_kernel_matrix_gpu.py is not vacuous (CPU, oracle alone).

A graph on which every codeword converges at once, or none does, would let a wrong convergence test, a wrong poll or a
wrong later pass through: the early-exit key of every graph (either size) and update rule must hold a converged and a
stuck codeword, at least three distinct iteration counts, a codeword that converges at iteration >= 5, one that
converges at iteration 1, and the lone codeword of the second tile must still run at iteration 3
(`kernel_matrix_cases.vacuous`).  The case builder asserts the degrees of every graph itself."""
import numpy as np
import pytest

import kernel_matrix_cases as K


@pytest.mark.parametrize("method", K.METHODS)
@pytest.mark.parametrize("tall", [False, True], ids=["72x200", "144x400"])
@pytest.mark.parametrize("R,C", K.GRAPHS)
def test_key_is_not_vacuous(oracle, R, C, tall, method):
    G, Hd = K.graph(R, C, tall)
    assert (G.m, G.n) == K.shape(tall) and Hd.sum(axis=1).max() == R and Hd.sum(axis=0).max() == C
    ref = K.key(R, C, method, True, "shared", K.BATCH, tall)
    assert K.vacuous(ref) == []
    inp = K.inputs(R, C, method, tall)
    assert inp["synd"].shape == (K.BATCH, G.m) and not inp["synd"][0].any() and inp["synd"][K.BATCH - 1].any()
    assert ((inp["probs"] == 0).sum() == G.n // 10) == (method == "min_sum")
    assert inp["probs"][inp["probs"] > 0].min() >= 0.02 and inp["probs"].max() <= 0.2
    if method == "min_sum":  # p = 0 priors: infinite posteriors are part of the key
        assert np.isinf(ref["llr"]).any()


def test_the_tall_graphs_are_tall_enough_for_the_fused_test():
    """The convergence test rides on a check pass only with at least 36 words of unsatisfied-check flags per tile, one
    word per 4 rows in blocks of 4 words (parity_waves, FT_WORDS in the library's sources): 129 rows and up."""
    words = lambda m: 4 * ((m + 15) // 16)
    assert words(K.shape(True)[0]) >= 36 > words(K.shape(False)[0])


def test_the_short_key_of_the_row_parallel_cases_decides_something(oracle):
    """Five codewords, one per error scale: the first converges at iteration 1, and not all of them stop together."""
    for R in (16, 32, 64):
        for method in K.METHODS:
            ref = K.key(R, 16, method, True, "shared", K.EDGE_BATCH)
            assert ref["converged"][0] and ref["iters"][0] == 1 and len(set(ref["iters"].tolist())) >= 2, (R, method)
