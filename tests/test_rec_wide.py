"""What tests/test_rec_wide_gpu.py relies on, shown without a GPU (oracle and tests/settle_ref.py alone).

The wide-column record form (`minsum_rec = 2`) is held to the f32 oracle bit for bit; a key on which every codeword stops
at once, a staircase without its wide columns, or settle inputs on which every tile (or none) freezes would let a wrong
kernel, a wrong slice of the records or a wrong mark through.  The public header documents the knob's new value."""
import os
import re

import numpy as np
import pytest

import kernel_matrix_cases as K
import rec_wide_cases as W
import settle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prior", ["shared", "full", "tail"])
@pytest.mark.parametrize("tall", [False, True], ids=["72x200", "144x400"])
@pytest.mark.parametrize("R_,C", W.WIDE + W.PAST)
def test_key_is_not_vacuous(oracle, R_, C, tall, prior):
    seed = W.SEEDS[(R_, C, tall)]
    G, Hd = K.graph(R_, C, tall, seed)
    assert (G.m, G.n) == K.shape(tall) and Hd.sum(axis=1).max() == R_ and Hd.sum(axis=0).max() == C
    assert (Hd.sum(axis=0) > 6).sum() == 1  # ONE wide column: the narrow launch runs the 16-edge build beside it
    ref = K.key(R_, C, "min_sum", True, prior, tall=tall, seed=seed)
    assert K.vacuous(ref) == []
    inp = K.inputs(R_, C, "min_sum", tall, seed)
    assert inp["synd"].shape == (K.BATCH, G.m) and (inp["probs"] == 0).sum() == G.n // 10
    assert np.isinf(ref["llr"]).any()  # p = 0 priors: infinite posteriors are part of the key
    # the call with one-tile groups whose first tile is still running after iteration 1 can be composed
    assert (~(ref["converged"].astype(bool) & (ref["iters"] == 1))).any()


def test_staircase_holds_every_wide_degree(oracle):
    G, Hd, probs, synd = W.staircase()
    cdeg = Hd.sum(axis=0)
    assert (G.m, G.n) == (192, 665) and Hd.sum(axis=1).max() == 64 and cdeg.max() == 64 and (cdeg > 32).sum() == 32
    assert sorted(cdeg[cdeg > 32].tolist()) == list(range(33, 65))
    assert synd.shape == (W.STAIR_BATCH, G.m) and not synd[0].any() and (probs == 0).sum() == G.n // 10
    early, fixed = W.staircase_key(True), W.staircase_key(False)
    conv = early["converged"].astype(bool)
    # (rows of up to 64 edges: only the error-free codewords converge, at iteration 1; the others run all nine iterations,
    # and their posteriors -- finite, infinite and NaN -- are what holds the wide columns)
    assert conv.any() and not conv.all() and set(early["iters"].tolist()) == {1, W.STAIR_ITER}
    assert (fixed["iters"] == W.STAIR_ITER).all() and np.isinf(fixed["llr"]).any()
    wide = np.flatnonzero(cdeg > 32)
    assert np.isfinite(fixed["llr"][:, wide]).any() and len(np.unique(fixed["llr"][~conv][:, wide])) > 100


def test_settle_inputs_freeze_one_tile_and_not_another(oracle):
    """Seeds are counted up from 1; SETTLE_SEED is the first at which the first tile freezes, the second never does."""
    c = W.settle_case()
    cdeg = np.diff(np.asarray(c.H.col_ptr))
    assert (c.H.m, c.H.n) == (W.SETTLE_R, W.SETTLE_N + W.SETTLE_R) and cdeg.max() == W.SETTLE_WIDE == cdeg[0]
    assert (cdeg > 32).sum() == 1 and (cdeg[W.SETTLE_N:] == 1).all()
    assert W.SETTLE_SEED == 1 and c.first == 3
    frozen = R.frozen_at(c.same, c.first, W.SETTLE_ITER, batch=W.SETTLE_BATCH)
    assert len(frozen) == 3 and frozen[0] >= 5 and frozen[1] == 0 and frozen[2] > 0, frozen
    assert max(frozen) + 2 < W.SETTLE_ITER  # a horizon forced to max + 2 leaves passes out, and is too short for tile 1
    # the restatement IS the oracle on these inputs, wide column included
    ref = W.settle_key()
    assert np.array_equal(ref["llr"], c.post[W.SETTLE_ITER], equal_nan=True)


def test_horizon_inputs_freeze_every_tile(oracle):
    """Ten tiles of trials by the sweep's law, every one of which freezes well before the last iteration: a settle = 2 call
    learns the horizon max + 2 from them.  (Trial seeds 1000, 2000, 3000 each leave a tile that never freezes.)"""
    c = W.horizon_case()
    frozen = R.frozen_at(c.same, c.first, W.HORIZON_ITER, batch=W.HORIZON_BATCH)
    assert len(frozen) == 10 and all(frozen) and 2 * (max(frozen) + 2) < W.HORIZON_ITER, frozen  # (settle_next_horizon's rule)
    assert len(set(frozen)) >= 3  # (tiles freeze at different iterations: the horizon is the slowest one's)
    assert np.array_equal(W.horizon_key()["llr"], c.post[W.HORIZON_ITER], equal_nan=True)


def test_header_documents_the_wide_value():
    text = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    knob = re.search(r'\n \*   "minsum_rec"(.*?)\n \*   "', text, re.S)  # (the entry, up to the next knob's)
    assert knob, "include/scaldpc.h: no minsum_rec entry in the knob text of scaldpc_bp_configure"
    assert re.search(r"\b2 = [^\n]*\b33\b[^\n]*\b64\b", knob.group(1)), "value 2 (columns of 33 ... 64 edges) is not documented"
