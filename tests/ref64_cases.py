"""TEST INFRASTRUCTURE: the instances, oracle results and the parity bar that tests/test_ref64.py (CPU: the preconditions,
on the oracle alone) and tests/test_ref64_gpu.py (the float64 ratio-domain decode, scaldpc_bp_decode_batch_f64) share.
Every reference is computed once per session and left unchanged."""
import functools

import numpy as np

import mc_ref
from helpers import PRODUCTION_POINTS, S, hqc_full_size_point, staircase_graph
from oracle import pyoracle

ULP_BAR = 4  # |dL| <= 4 ulp of the oracle's value: glibc's log (< 1 ulp) + the device library's (1 ulp), doubled
FULL_SIZE_ROWS = np.array([0, 1, 2, 3, 62, 63, 64, 65, 66, 126, 127, 128, 129, 5, 6, 7])


def oracle64(H, probs, x, kind, max_iter, early, threads=8):
    """The key: the oracle's method 0 in float64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return pyoracle.bp_decode_batch(H, probs, x, kind, max_iter, "product_sum", dtype="f64", threads=threads, early_exit=early)


def worst_ulp(got_llr, ref_llr):
    """Largest |got - ref| in units of the spacing of the oracle's value, over the finite entries; asserts that +-inf and NaN
    sit in the same places (infinities with the same sign)."""
    got_llr = np.asarray(got_llr)
    assert got_llr.dtype == np.float64 and ref_llr.dtype == np.float64 and got_llr.shape == ref_llr.shape
    assert np.array_equal(np.isnan(got_llr), np.isnan(ref_llr)), "NaN posteriors in different places"
    inf = np.isinf(ref_llr)
    assert np.array_equal(np.isinf(got_llr), inf) and np.array_equal(got_llr[inf], ref_llr[inf]), "infinite posteriors differ"
    fin = np.isfinite(ref_llr)
    if not fin.any():
        return 0.0
    return float((np.abs(got_llr[fin] - ref_llr[fin]) / np.spacing(np.abs(ref_llr[fin]))).max())


MEASURED = {}  # label -> worst ulp distance seen (printed by the GPU tests, recorded in profiles/ref64/README.md)


def hold_to_bar(got, ref, label=None):
    """The parity bar of the float64 decode: bits, iters and converged EQUAL on every codeword, settled or not; llr with
    +-inf / NaN in the same places and within ULP_BAR ulp of the oracle's value elsewhere.  Returns the worst ulp distance."""
    assert np.array_equal(got["iters"], ref["iters"]), "iteration counts differ"
    assert np.array_equal(got["converged"].astype(np.int32), ref["converged"]), "converged flags differ"
    assert np.array_equal(got["bits"], ref["bits"]), "hard decisions differ"
    if got.get("llr") is None:
        return 0.0
    w = worst_ulp(got["llr"], ref["llr"])
    if label is not None:
        MEASURED[label] = max(MEASURED.get(label, 0.0), w)
        print(f"ref64 worst ulp distance [{label}]: {w:.2f}")
    assert w <= ULP_BAR, f"posterior {w:.2f} ulp from the oracle's (bar {ULP_BAR})"
    return w


def equal_bit_for_bit(a, b):
    """Two device results, llr included (as bit patterns: NaN payloads too)."""
    ok = all(np.array_equal(a[k], b[k]) for k in ("bits", "iters", "converged"))
    if a.get("llr") is not None or b.get("llr") is not None:
        ok = ok and np.array_equal(a["llr"].view(np.uint64), b["llr"].view(np.uint64))
    return ok


# ------------------------------------------------------------------------------------------------------------ F, H1, H2
@functools.lru_cache(maxsize=None)
def mc_case(name):
    """(H, probs, inputs, kind) of the mc_ref instance: F in syndrome mode, H1 / H2 in received mode; 130 trials."""
    i = mc_ref.instance(name)
    if name == "F":
        return i["H"], i["probs"], mc_ref.fer_law()["synd"], 0
    return i["H"], i["probs"], mc_ref.hqc_law(name)["msg"], 1


@functools.lru_cache(maxsize=None)
def mc_oracle(name, early):
    H, probs, x, kind = mc_case(name)
    return oracle64(H, probs, x, kind, mc_ref.MAX_ITER, early, threads=4)


# ------------------------------------------------------------------------------------------------------------ staircase
STAIRCASE_ITERS = {32: 8, 64: 20}


@functools.lru_cache(maxsize=None)
def staircase_case(colmax):
    """tests/test_bp_gpu.py::test_staircase_graph_every_degree's graph, priors and syndromes: (G, probs, synd)."""
    rng = np.random.RandomState(640 + colmax)
    G, Hd = staircase_graph(rng, rows_per_degree=3, colmax=colmax, fillers=600)
    probs = rng.uniform(0.01, 0.2, size=G.n)
    batch = 150
    scale = np.array([0.0, 0.01, 0.03, 0.1, 0.3, 1.0])[np.arange(batch) % 6]
    err = (rng.rand(batch, G.n) < probs[None, :] * scale[:, None]).astype(np.uint8)
    return G, probs, G.syndrome(err)


@functools.lru_cache(maxsize=None)
def staircase_oracle(colmax, early=True):
    G, probs, synd = staircase_case(colmax)
    return oracle64(G, probs, synd, 0, STAIRCASE_ITERS[colmax], early)


# ------------------------------------------------------------------------------------------------------------- wide toy
WIDE_ITERS = 12


@functools.lru_cache(maxsize=None)
def wide_case():
    """A toy for the any-degree loops: row 0 has 200 edges, row 1 has 65, column 0 sits in 70 rows; a p = 0 and a p = 1 prior
    on columns of the wide rows.  Syndromes of errors drawn at a few weights.  (G, probs, synd), batch 70."""
    rng = np.random.RandomState(6465)
    m, n = 96, 260
    H = np.zeros((m, n), dtype=np.int8)
    H[0, :200] = 1
    H[1, 150:215] = 1
    H[rng.choice(np.arange(2, m), size=69, replace=False), 0] = 1  # column 0: row 0 and 69 more
    for r in range(2, m):
        H[r, rng.choice(np.arange(1, n), size=4, replace=False)] = 1
    G = S.TannerGraph.from_dense(H)
    assert H.sum(axis=1).max() == 200 and H[1].sum() == 65 and H[:, 0].sum() == 70
    probs = rng.uniform(0.01, 0.08, size=n)
    probs[7] = 0.0
    probs[160] = 1.0
    batch = 70
    scale = np.array([0.0, 0.3, 1.0, 2.0, 4.0])[np.arange(batch) % 5]
    err = (rng.rand(batch, n) < np.minimum(probs[None, :] * scale[:, None], 1.0)).astype(np.uint8)
    err[:, 7] = 0
    err[:, 160] = 1
    return G, probs, G.syndrome(err)


@functools.lru_cache(maxsize=None)
def wide_oracle(early=True):
    G, probs, synd = wide_case()
    return oracle64(G, probs, synd, 0, WIDE_ITERS, early)


# ------------------------------------------------------------------------------------------------------------ full size
FULL_SIZE_ITERS = 50


@functools.lru_cache(maxsize=None)
def full_size_case():
    """The hqc128_W50_R2000 point at batch 130: (H, probs, msg)."""
    p = PRODUCTION_POINTS["hqc128_W50_R2000"]
    H, _, probs, msg, _ = hqc_full_size_point(p["name"], p["key"], p["R"], p["eps"], 130)
    return H, probs, msg


@functools.lru_cache(maxsize=None)
def full_size_oracle(dtype="f64"):
    """The oracle on FULL_SIZE_ROWS: method 0 in float64, or the f32 instantiation in the fp32 kernels' order."""
    H, probs, msg = full_size_case()
    x = np.ascontiguousarray(msg[FULL_SIZE_ROWS])
    if dtype == "f64":
        return oracle64(H, probs, x, 1, FULL_SIZE_ITERS, True, threads=16)
    with np.errstate(divide="ignore", invalid="ignore"):
        return pyoracle.bp_decode_batch(H, probs, x, 1, FULL_SIZE_ITERS, "tanh_complement", dtype="f32", threads=16, early_exit=True)
