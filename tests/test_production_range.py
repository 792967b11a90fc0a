"""The preconditions of tests/test_production_range_gpu.py, pinned without a GPU.

The binary BP kernels are chosen by the SHAPE of the graph: the maximum column degree picks the 16 / 32 / 64-edge
variable builds and, at 32, whether min-sum runs in its record form at all; the row degree picks the check kernels.
The GPU tests hold each of those selections to the oracle at full size and across a live decoder's growth; they only
mean something if (a) the graphs are what their table says and (b) the trials are hard enough to reach the later
iterations, the early-exit latching and the compaction.  Both are pinned here, on the CPU, so that a changed fixture or
generator fails in this file and not silently on the GPU.  (c): at these points the tanh rule's tolerance is not the
weak link -- the oracle's own float32 and float64 runs agree within `compare`'s bound."""
import numpy as np
import pytest

from helpers import (PRODUCTION_GROWTH, PRODUCTION_POINTS, S, compare, growth_run, hqc_first_rows, hqc_full_size_point,
                     prefix_point, sample_rows)

SAMPLE = 32  # codewords per oracle sample
MAX_ITER = 50


def _column_degrees(Hin, R):
    return np.bincount(Hin.col_idx[: Hin.row_ptr[R]], minlength=Hin.n)


@pytest.mark.parametrize("label", list(PRODUCTION_POINTS))
def test_graph_is_what_the_table_says(label):
    p = PRODUCTION_POINTS[label]
    H, Hin, _ = S.codes.hqc_bench_graph(p["name"], hqc_first_rows()[p["key"]], R=p["R"])
    assert (H.m, H.n, H.nnz) == (p["R"], S.codes.HQC_PARAMS[p["name"]][0] + p["R"], p["E"])
    assert set(np.diff(H.row_ptr).tolist()) == {p["row_deg"]}
    d = _column_degrees(Hin, p["R"])
    assert d.max() == p["max_col_deg"] and int((d > 32).sum()) == p["cols_over_32"]
    # what runs follows from these: record form iff no column is wider than 32; 16-edge variable builds iff none is wider than 16
    assert (p["max_col_deg"] <= 32) == (label not in ("hqc128_W50_R8000", "hqc256_W60_R20000"))


@pytest.mark.parametrize("run", list(PRODUCTION_GROWTH))
def test_crossing_rows(run):
    """The first row count at which the maximum column degree exceeds 16 / 32, and that the growth run starts below the
    line, ends above it and has whole steps of 50 rows on either side of the step that holds the crossing row."""
    g = PRODUCTION_GROWTH[run]
    _, Hin, _ = S.codes.hqc_bench_graph(g["name"], hqc_first_rows()[g["key"]], R=g["R1"])
    W = int(Hin.row_ptr[1])
    cols = Hin.col_idx.reshape(g["R1"], W)
    deg = np.zeros(Hin.n, dtype=np.int64)
    first = None
    for r in range(g["R1"]):
        deg[cols[r]] += 1
        if first is None and deg[cols[r]].max() > g["line"]:
            first = r + 1  # the graph of the first r + 1 rows is the first one past the line
    assert first == g["crossing"]
    assert _column_degrees(Hin, g["R0"]).max() <= g["line"] < _column_degrees(Hin, g["R1"]).max()
    step_with_crossing = (g["crossing"] - g["R0"] + 49) // 50
    assert 2 <= step_with_crossing <= (g["R1"] - g["R0"]) // 50 - 1


def test_sample_rows():
    assert np.array_equal(sample_rows(390, 15), np.r_[0:15, 192:207, 384:390])  # the last tile is ragged: 6 codewords
    assert np.array_equal(sample_rows(130, 17), np.r_[0:17, 64:81, 128:130])
    assert np.array_equal(sample_rows(200, 14), np.r_[0:14, 128:142, 192:200])
    assert np.array_equal(sample_rows(4096, 8, (0, 2, 61)), np.r_[0:8, 128:136, 3904:3912])
    assert all(36 <= sample_rows(b, k, t).size <= 48 for b, k, t in ((390, 15, None), (130, 17, None), (200, 14, None),
                                                                    (4096, 5, (0, 2, 4, 32, 34, 36, 60, 62))))


def _conditions(oracle, H, probs, msg, spread, stuck, what):
    """On the oracle alone (f32, early exit): the sample holds >= 3 distinct iteration counts, a codeword that converges
    and one that does not."""
    out = {}
    for method in ("min_sum", "tanh_complement"):
        r = oracle.bp_decode_batch(H, probs, msg, 1, MAX_ITER, method, dtype="f32", threads=16)
        conv = r["converged"].astype(bool)
        counts = set(r["iters"].tolist())
        print(what, method, "converged %.2f" % conv.mean(), "iteration counts", sorted(counts))
        assert conv.any(), (what, method, "nothing converges")
        if spread:
            assert len(counts) >= 3, (what, method, sorted(counts))
        if stuck:
            assert not conv.all(), (what, method, "everything converges")
        out[method] = r
    return out


@pytest.mark.parametrize("label", list(PRODUCTION_POINTS))
def test_oracle_sample_is_hard_enough_and_the_tolerance_is_not_the_weak_link(oracle, label):
    p = PRODUCTION_POINTS[label]
    H, Hin, probs, msg, ys = hqc_full_size_point(p["name"], p["key"], p["R"], p["eps"], SAMPLE)
    with np.errstate(divide="ignore"):
        f32_early = _conditions(oracle, H, probs, msg, p["spread"], p["stuck"], label)["tanh_complement"]
        # the oracle's own float32 run within `compare`'s tolerance of its float64 run, SAME formulation: at these
        # points BP is not chaotic, so a tanh-rule failure on the GPU is a finding about the kernel or the schedule
        for early in (True, False):
            f32 = f32_early if early else oracle.bp_decode_batch(H, probs, msg, 1, MAX_ITER, "tanh_complement", dtype="f32",
                                                                  threads=16, early_exit=False)
            f64 = oracle.bp_decode_batch(H, probs, msg, 1, MAX_ITER, "tanh_complement", dtype="f64", threads=16, early_exit=early)
            compare({k: f32[k] for k in ("bits", "llr", "iters", "converged")}, f64, "product_sum")


@pytest.mark.parametrize("run", list(PRODUCTION_GROWTH))
def test_growth_runs_start_and_end_hard_enough(oracle, run):
    g = PRODUCTION_GROWTH[run]
    Hin, probs, msg = growth_run(run, SAMPLE)
    with np.errstate(divide="ignore"):
        for r in (g["R0"], g["R1"]):
            H, pr, x = prefix_point(Hin, probs, msg, r)
            _conditions(oracle, H, pr, x, True, True, (run, r))
