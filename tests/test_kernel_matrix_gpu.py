"""The template grid of the binary BP kernels, every instantiation launched by construction and held to the oracle.

The check and variable kernels are compiled per row / column cap (16 / 32 / 64 and the any-degree forms), per pass
(first, fused convergence test, first record pass, last pass) and per prior source; which one runs is decided by the
graph's maximum degrees and the call.  The rest of the suite is organised by feature and by graph shape: the kernel
census (tests/golden/kernel_census.json) shows that it launches every instantiation somewhere, several of them in a
single file whose subject is something else, and not every launching test compares with a reference.  Here the grid is
closed on purpose: the sixteen graphs of tests/kernel_matrix_cases.py (maximum row degree x maximum column degree, each
ON a line of the cap ladder or just past the last), one test per graph, every case of

    method x early exit x prior source (shared, per codeword [65, n], [65, 40]) x knobs (first_fused, fuse_test, minsum_rec)

on the 64-codeword-tile kernels with 65 codewords and 9 iterations (polls at 4 and 8, the first record pass at 2, a last
pass at 9).  Every graph is decoded at two sizes, 72 x 200 and 144 x 400: the convergence test rides on a check pass
(iterations 2, 3, 5, 6, 7) only from 129 rows on.  The smaller one also runs in the LDS-resident decoder.  min-sum:
decisions, iteration counts, converged flags and posteriors bit for bit, NaNs in the same places; tanh rule:
`helpers.compare` as it is.  A second parametrisation runs five codewords on the row-parallel kernels.
tests/test_kernel_matrix.py shows that the key decides something; tests/test_kernel_census.py and
profiles/kernel_census/README.md say which kernel each test file launches."""
import importlib

import numpy as np
import pytest

import kernel_matrix_cases as K
from helpers import compare
from test_production_range_gpu import _exact

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

KNOBS = {"min_sum": ({}, {"first_fused": 0}, {"fuse_test": 0}, {"minsum_rec": 0}),
         "product_sum": ({}, {"first_fused": 0}, {"fuse_test": 0})}


@pytest.fixture(autouse=True)
def own_knobs(monkeypatch):
    """Every knob at the library's default unless a case sets it."""
    for v in ("SCALDPC_PATH", "SCALDPC_SPLIT", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_COMPACT_AFTER",
              "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST", "SCALDPC_MINSUM_REC", "SCALDPC_PRECISION"):
        monkeypatch.delenv(v, raising=False)


def _decoder(G, method, probs, path, knobs):
    with np.errstate(divide="ignore"):  # (p = 0 priors)
        dec = bp.bp_decoder(G, max_iter=K.MAX_ITER, bp_method=method, channel_probs=probs)
    dec.configure(path=path, **knobs)
    return dec


def _held(got, ref, method, what):
    if method == "min_sum":
        _exact(got, ref, what)
    else:
        try:
            compare(got, ref, method)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from e


@pytest.mark.parametrize("R,C", K.GRAPHS)
def test_tile_kernels_on_graph(oracle, R, C):
    """Graph (R, C) at both sizes (the taller one is where the convergence test rides on the check passes), every case
    on the tile kernels; the smaller one also through the LDS-resident single-launch decoder (the library's own choice
    for a graph of this size), shared and per-codeword priors."""
    for tall in (False, True):
        G, _ = K.graph(R, C, tall)
        for method in K.METHODS:
            inp = K.inputs(R, C, method, tall)
            for knobs in KNOBS[method]:
                dec = _decoder(G, method, inp["probs"], "stream", knobs)
                record = C <= 32 and R <= 64 and knobs.get("minsum_rec", 1) == 1
                for prior in ("shared", "full") + (("tail",) if not knobs else ()):
                    for early in (True, False):
                        what = (R, C, tall, method, knobs, prior, early)
                        with np.errstate(divide="ignore"):
                            got = dec.decode_batch(inp["synd"], early_exit=early, want_llr=True, input_vector_type="syndrome",
                                                   channel_probs=K.prior_array(inp, prior))
                        assert dec.last_row_parallel() == 0, what
                        if method == "min_sum":
                            assert dec.time_kernels(2)["record_form"] == record, what
                        _held(got, K.key(R, C, method, early, prior, K.BATCH, tall), method, what)
                dec.close()
            if tall:
                # A group skips its poll at iteration 1 once an earlier group of the call saw nobody finish there, and only
                # then does iteration 1's test ride on iteration 2's check pass -- min-sum's FIRST record pass with the
                # test on it.  Tile groups of one tile; the first tile holds codewords that (by the oracle) are still
                # running after iteration 1, the batch of 65 follows.
                ref = K.key(R, C, method, True, "shared", K.BATCH, tall)
                late = np.flatnonzero(~(ref["converged"].astype(bool) & (ref["iters"] == 1)))
                order = np.concatenate([np.resize(late, 64), np.arange(K.BATCH)])
                dec = _decoder(G, method, inp["probs"], "stream", {})
                dec.set_tile_group(1)
                got = dec.decode_batch(inp["synd"][order], early_exit=True, want_llr=True, input_vector_type="syndrome")
                assert dec.last_row_parallel() == 0 and dec.last_schedule()["polls"] >= 2
                _held(got, {k: v[order] for k, v in ref.items()}, method, (R, C, tall, method, "one-tile groups"))
                dec.close()
                continue
            dec = _decoder(G, method, inp["probs"], "lds", {})
            for prior in ("shared", "full", "tail"):
                for early in (True, False):
                    with np.errstate(divide="ignore"):
                        got = dec.decode_batch(inp["synd"], early_exit=early, want_llr=True, input_vector_type="syndrome",
                                               channel_probs=K.prior_array(inp, prior))
                    assert dec.last_row_parallel() == 0
                    _held(got, K.key(R, C, method, early, prior), method, (R, C, method, "lds", prior, early))
            dec.close()


@pytest.mark.parametrize("R", K.DEGREES)
def test_row_parallel_kernels_on_graph(oracle, R):
    """Five codewords on the row-parallel kernels (k_el_check, k_el_var), both update rules, shared and per-codeword
    priors, iteration 1 with and without its check pass.  A 65-edge row is wider than a wave: the same call then runs
    on the tile kernels, and still equals the oracle."""
    C, nb = 16, K.EDGE_BATCH
    G, _ = K.graph(R, C)
    for method in K.METHODS:
        inp = K.inputs(R, C, method)
        for knobs in ({}, {"first_fused": 0}):
            dec = _decoder(G, method, inp["probs"], "edge", knobs)
            for prior in ("shared", "full"):
                cp = K.prior_array(inp, prior)
                for early in (True, False):
                    what = (R, C, method, knobs, prior, early, "edge")
                    with np.errstate(divide="ignore"):
                        got = dec.decode_batch(inp["synd"][:nb], early_exit=early, want_llr=True, input_vector_type="syndrome",
                                               channel_probs=None if cp is None else cp[:nb])
                    assert dec.last_row_parallel() == (nb if R <= 64 else 0), what
                    _held(got, K.key(R, C, method, early, prior, nb), method, what)
            dec.close()
