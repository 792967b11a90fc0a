"""Shared builders for the parity tests (seeded inputs, HQC-shaped instances)."""
import importlib
import json
import os

import numpy as np

S = importlib.import_module("sca-ldpc_amd")


def random_graph(rng, m, n, density, ensure_cover=True):
    H = (rng.rand(m, n) < density).astype(np.int8)
    if ensure_cover:
        for i in range(m):
            if not H[i].any():
                H[i, rng.randint(n)] = 1
    return S.TannerGraph.from_dense(H)


def hqc_instance(N, W, R, omega, eps, batch, seed, flip=True):
    """[Hin | I_R] with synthetic trials as SURVEY.md 8(d) defines them: y = omega
    distinct positions, checks = Hin y (+ flips with prob eps), priors
    [omega/N]*N ++ [eps]*R, message [0]*N ++ checks (hqc.py:684-705)."""
    rng = np.random.RandomState(seed)
    sup = S.codes.make_random_ldpc_first_row(N, W, rng)
    rows = rng.permutation(N)[:R]
    Hin = S.codes.hqc_check_graph(sup, N, rows)
    H = Hin.with_identity()
    y = np.zeros((batch, N), dtype=np.uint8)
    for b in range(batch):
        y[b, rng.choice(N, omega, replace=False)] = 1
    checks = Hin.syndrome(y)
    if flip and eps > 0:
        checks = checks ^ (rng.rand(batch, R) < eps).astype(np.uint8)
    msg = np.concatenate([np.zeros((batch, N), dtype=np.uint8), checks], axis=1)
    probs = np.concatenate([np.full(N, omega / N), np.full(R, eps)])
    return H, Hin, probs, msg, y


def staircase_graph(rng, rows_per_degree=3, colmax=32, fillers=600):
    """A graph whose rows take EVERY degree 1 .. 64 (`rows_per_degree` of each) and whose columns take every degree
    0 .. colmax (one "staircase" column of each), the rest of the edges spread over `fillers` columns of middling degree:
    every exact-degree instantiation of the register-resident kernels (check kernels 1 .. 64; record-form variable
    kernel 1 .. 32, bucketed variable kernels up to 64) meets the oracle in ONE decode (VERDICT r03 #1d)."""
    degs = np.repeat(np.arange(1, 65), rows_per_degree)
    rng.shuffle(degs)  # (degrees in no particular row order: the library sorts its launch lists itself)
    m = len(degs)
    n = (colmax + 1) + fillers
    H = np.zeros((m, n), dtype=np.int8)
    left = degs.copy()
    for k in range(colmax, 0, -1):  # staircase column k: k distinct rows that still have room, heaviest first
        cand = np.flatnonzero(left > 0)
        w = left[cand].astype(np.float64)
        pick = rng.choice(cand, size=k, replace=False, p=w / w.sum())
        H[pick, k] = 1
        left[pick] -= 1
    for r in range(m):  # the rest of each row: distinct filler columns
        if left[r]:
            H[r, (colmax + 1) + rng.choice(fillers, size=left[r], replace=False)] = 1
    assert (H.sum(axis=1) == degs).all() and (H[:, : colmax + 1].sum(axis=0) == np.arange(colmax + 1)).all()
    return S.TannerGraph.from_dense(H), H


def hqc_first_rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hqc_first_rows.json")) as fh:
        return json.load(fh)


def hqc_full_size_point(name, key, R, eps, batch, base_seed=2):
    """One full-size point of the production range: H = [Hin | I_R] with Hin the first R rows of
    `codes.hqc_bench_graph(name, first row `key` of tests/golden/hqc_first_rows.json)` (row_seed 1, so a graph with more
    rows EXTENDS one with fewer: the attack loop's growth), `batch` synthetic trials (`trials.hqc_trials`, trial i seeded
    base_seed + i) and their priors (eps = 0: certainty-1.0 checks, p = 0, hqc.py:689).
    Returns (H, Hin, probs, msg, ys)."""
    trials = importlib.import_module("sca-ldpc_amd.trials")
    H, Hin, _ = S.codes.hqc_bench_graph(name, hqc_first_rows()[key], R=R)
    N, omega = S.codes.HQC_PARAMS[name]
    msg, ys = trials.hqc_trials(Hin, omega, eps, batch, base_seed=base_seed)
    return H, Hin, trials.hqc_priors(N, R, omega, eps), msg, ys


def sample_rows(batch, per_tile, tiles=None):
    """Codeword indices for an oracle sample: the first `per_tile` codewords of each 64-codeword tile in `tiles`
    (default: the first, a middle and the last tile); a last tile that is ragged gives what it has."""
    T = (batch + 63) // 64
    tiles = sorted({0, T // 2, T - 1}) if tiles is None else tiles
    return np.concatenate([np.arange(t * 64, min(t * 64 + per_tile, batch, (t + 1) * 64)) for t in tiles])


# The production range at full size (tests/test_production_range.py pins what each graph is and that its trials are
# hard enough; tests/test_production_range_gpu.py holds the kernels to the oracle there).  Per point: the arguments of
# `hqc_full_size_point`, the GPU batch, the table's facts (edges, row degree, maximum column degree, columns wider
# than 32) and what the oracle sample must hold (`spread`: >= 3 distinct iteration counts; `stuck`: a codeword that does
# not converge).  eps was raised from the bench's 0.05 where every codeword converges in 2-3 iterations there.
PRODUCTION_POINTS = {
    "hqc128_W50_R2000": dict(name="hqc128", key="N17669_W50_s0", R=2000, eps=0.0, batch=4096,
                             E=102000, row_deg=51, max_col_deg=16, cols_over_32=0, spread=True, stuck=True),
    "hqc128_W50_R4000": dict(name="hqc128", key="N17669_W50_s0", R=4000, eps=0.0, batch=4096,  # the literal `bench.py --eps 0` graph:
                             E=204000, row_deg=51, max_col_deg=24, cols_over_32=0, spread=False, stuck=False),  # easy, kept for its priors
    "hqc128_W20_R4000": dict(name="hqc128", key="N17669_W20_s0", R=4000, eps=0.01, batch=390,
                             E=84000, row_deg=21, max_col_deg=13, cols_over_32=0, spread=True, stuck=True),
    "hqc128_W50_R8000": dict(name="hqc128", key="N17669_W50_s0", R=8000, eps=0.2, batch=390,
                             E=408000, row_deg=51, max_col_deg=36, cols_over_32=54, spread=True, stuck=True),
    "hqc256_W60_R12000": dict(name="hqc256", key="N57637_W60_s0", R=12000, eps=0.08, batch=200,
                              E=732000, row_deg=61, max_col_deg=27, cols_over_32=0, spread=True, stuck=True),
    "hqc256_W60_R6000": dict(name="hqc256", key="N57637_W60_s0", R=6000, eps=0.0, batch=200,
                             E=366000, row_deg=61, max_col_deg=18, cols_over_32=0, spread=True, stuck=True),
    "hqc256_W60_R20000": dict(name="hqc256", key="N57637_W60_s0", R=20000, eps=0.2, batch=200,
                              E=1220000, row_deg=61, max_col_deg=38, cols_over_32=61, spread=True, stuck=True),
}
# A live decoder grown across a line of the kernel selection: (first row key, start rows, end rows, the column degree
# that is passed, the first row count at which the maximum column degree exceeds it, eps)
PRODUCTION_GROWTH = {
    "W50_across_16": dict(name="hqc128", key="N17669_W50_s0", R0=1900, R1=2100, line=16, crossing=2016, eps=0.0),
    "W50_across_32": dict(name="hqc128", key="N17669_W50_s0", R0=6500, R1=7000, line=32, crossing=6708, eps=0.2),
    "W20_across_16": dict(name="hqc128", key="N17669_W20_s0", R0=7200, R1=7400, line=16, crossing=7262, eps=0.1),
}


def growth_run(run, batch, base_seed=2):
    """Inputs of one growth run: the END graph's Hin, priors and trials; `prefix_point` cuts them down to the first r
    checks.  The eps = 0 run has noise-free answers and MIXED priors: half of the checks at certainty 1.0 (p = 0,
    hqc.py:689), the others at certainty 0.95 -- infinite and finite check priors side by side (with a tenth at
    certainty 1.0 the min-sum oracle converges on every codeword of its sample at 2100 rows).
    Returns (Hin, probs, msg)."""
    g = PRODUCTION_GROWTH[run]
    _, Hin, probs, msg, _ = hqc_full_size_point(g["name"], g["key"], g["R1"], g["eps"], batch, base_seed=base_seed)
    if g["eps"] == 0.0:
        cert = np.where(np.random.RandomState(77).rand(g["R1"]) < 0.5, 1.0, 0.95)
        probs = np.concatenate([probs[: Hin.n], 1.0 - cert])
    return Hin, probs, msg


def prefix_graph(Hin, r):
    """[Hin[:r] | I_r] of a constant-row-weight Hin."""
    N = Hin.n
    rp = Hin.row_ptr[: r + 1]
    cols = np.concatenate([Hin.col_idx[: rp[-1]].reshape(r, -1), N + np.arange(r, dtype=np.int32)[:, None]], axis=1)
    return S.TannerGraph.from_csr(r, N + r, np.arange(r + 1, dtype=np.int64) * cols.shape[1], cols.reshape(-1))


def prefix_point(Hin, probs, msg, r, nb=None):
    """(H, priors, received words) of the first r checks and the first nb codewords."""
    N = Hin.n
    return prefix_graph(Hin, r), probs[: N + r], np.ascontiguousarray(msg[:nb, : N + r])


# the f32 oracle instantiation that mirrors each kernel's operation order
ORACLE_METHOD = {"min_sum": "min_sum", "product_sum": "tanh_complement"}


def compare(got, ref, method, llr_rtol=2e-4, llr_atol=2e-4, widened_tol=None, tie_codewords=0):
    """HIP result vs the f32 oracle instantiation that runs the same operation order.

    min-sum  : everything bit-exact -- hard decisions, iteration counts, converged
               flags AND posteriors (only add / compare / abs, same order).
    tanh rule: the device evaluates exp / reciprocal / log on the hardware
               transcendental units (~1 ulp), the oracle with glibc, so the stated fp32
               tolerance is |dL| <= 2e-4 + 2e-4*|L| after clamping both sides to +-80
               (measured max 4.6e-5), and hard decisions bit-exact
               wherever |L| exceeds that tolerance.  Positions inside the tolerance are
               ties of the rule `L <= 0 -> 1`.  They pile up on trials that never
               converge (with certainty-1.0 checks a stuck trial collapses many
               messages to exactly 0), so their number is bounded only on the
               CONVERGED trials, where a tie would be a real disagreement.
               widened_tol (the property test on tiny dense graphs only): BP that does not settle
               on a graph full of 4-cycles is a chaotic map -- it amplifies the 1-ulp
               differences of exp / log 2-3x per iteration (and runs into inf - inf = NaN on
               both sides) -- so that test holds every posterior to
               |dL| <= widened_tol * (1 + |L|), with widened_tol derived from how far the oracle
               itself moves between float32 and float64 (never below 2e-4).  The tests on
               LDPC-like graphs (sparse, HQC-shaped, the BASELINE sizes) never relax anything.
    """
    if tie_codewords and method != "min_sum":
        # (property tests only) a posterior that is a tie of `L <= 0 -> 1` can decide whether H e == s
        # holds at some iteration: measured case -- device 4.8e-7, float64 oracle 1.6e-7, float32
        # oracle exactly 0, which alone called the codeword converged one iteration early.  Such
        # codewords (at most `tie_codewords`) are left out of the rest of the comparison.
        odd = (got["iters"] != ref["iters"]) | (got["converged"].astype(np.int32) != ref["converged"])
        assert odd.sum() <= tie_codewords, "iteration counts / converged flags differ on too many codewords"
        if odd.any():
            keep = ~odd
            got = {k: (v[keep] if v is not None else None) for k, v in got.items()}
            ref = {k: (v[keep] if v is not None else None) for k, v in ref.items()}
    assert np.array_equal(got["iters"], ref["iters"]), "iteration counts differ"
    assert np.array_equal(got["converged"].astype(np.int32), ref["converged"]), "converged flags differ"
    if method == "min_sum":
        assert np.array_equal(got["bits"], ref["bits"]), "hard decisions differ"
        if got.get("llr") is not None:
            assert np.array_equal(got["llr"], ref["llr"]), "min-sum posteriors must be bit-exact"
        return
    if got.get("llr") is None:
        assert (got["bits"] != ref["bits"]).mean() < 1e-4
        return
    # Saturation: an fp32 message turns infinite where 2 / (e^|x| + 1) drops below FLT_MIN, |x| = 87.34, and
    # whether a message sits a hair below or above that edge is a 1e-5-relative matter of the exponential
    # (measured: device posterior 157.98 = 35 + 35 + 87.9 against the oracle's inf).  Posteriors are
    # therefore compared after clamping to +-SAT: beyond it both sides say "certain", which is all a
    # posterior of that size means.
    SAT = 80.0
    a = np.clip(np.nan_to_num(got["llr"].astype(np.float64), nan=np.nan, posinf=SAT, neginf=-SAT), -SAT, SAT)
    b = np.clip(np.nan_to_num(ref["llr"].astype(np.float64), nan=np.nan, posinf=SAT, neginf=-SAT), -SAT, SAT)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN posteriors (inf - inf) in different places"
    fin = ~np.isnan(b)
    tol_all = llr_atol + llr_rtol * np.abs(b)
    if widened_tol is not None:
        tol_all = widened_tol * (1.0 + np.abs(b))
    assert (np.abs(a[fin] - b[fin]) <= tol_all[fin]).all(), "posterior outside the fp32 tolerance"
    with np.errstate(invalid="ignore"):
        decided = fin & (np.abs(b) > tol_all)
    assert np.array_equal(got["bits"][decided], ref["bits"][decided]), "hard decisions differ outside ties"
    conv = ref["converged"].astype(bool)
    # (not in the property tests: a widened tolerance widens the tie band with it, and with p = 0
    # priors on odd little graphs whole trials collapse to exact zeros whatever their flag says)
    if widened_tol is None and not tie_codewords:
        assert (~decided)[conv].sum() <= max(3, 1e-3 * decided[conv].size), "ties on converged trials"


REFERENCE_FORM_CLAMP = 24.0


def compare_with_reference_form(got, ref64, tol=1e-3, clamp=REFERENCE_FORM_CLAMP):
    """HIP fp32 tanh rule vs the float64 probability-ratio recursion the reference's
    package runs ("product_sum", oracle method 0).  Stated fp32 tolerance (SURVEY.md
    App. A): after clamping, |dL| <= 1e-3 * max(1, |L|); hard decisions
    exact wherever the reference's |L| exceeds that tolerance.  (inf - inf = NaN posteriors, which
    +-inf priors can produce on both sides, must sit in the same places.)
    The clamp is 24, not the 30 SURVEY suggested: the ratio form computes 1 - t as 2 / (1 + r) - 1 with
    r = e^-|L|, which in float64 is good to 1e-16 * e^|L| per factor -- 1e-6 at |L| = 24 but 1e-3 at |L| = 30
    times the row degree.  Measured (round 3): at L = -27.06 the float64 LLR-domain forms and the device agree
    to 1e-7 while the ratio form itself is off by 0.036; beyond the clamp both sides just say "certain"."""
    a = np.clip(got["llr"].astype(np.float64), -clamp, clamp)
    b = np.clip(ref64["llr"], -clamp, clamp)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), "NaN posteriors in different places"
    assert (np.abs(a - b)[~nan] <= (tol * np.maximum(1.0, np.abs(b)))[~nan]).all()
    with np.errstate(invalid="ignore"):
        decided = ~nan & (np.abs(ref64["llr"]) > tol)
    assert np.array_equal(got["bits"][decided], ref64["bits"][decided])


def reference_floor(ref, share=0.8):
    """Floor for `check_reference_form`: `share` of the codewords the f32 oracle converged on must also
    qualify for the float64 comparison -- so the check cannot pass by comparing nothing, yet a test whose
    trials mostly do not converge (by design) is not asked for more than exists."""
    return share * float(np.asarray(ref["converged"]).astype(bool).mean())


COMPARED = {}  # call-site label -> [codewords compared with the float64 reference form, codewords seen]


def check_reference_form(oracle, got, H, probs, x, kind, max_iter, early, *, min_fraction, threads=8, tol=1e-3, label=None,
                         same_order64=None, oracle32=None):
    """The independent check of every product-sum parity test: the HIP result against the float64
    probability-ratio recursion of the reference's package (oracle method 0) -- a different
    formulation in a different precision, so nothing here can mirror the device.  Compared on the
    codewords whose float64 decode settles (converged, and the same iteration count as the device):
    a trial that never converges wanders chaotically and float32 and float64 part ways on it by
    construction.  `min_fraction` (REQUIRED: every call site states its floor, see `reference_floor`)
    keeps the check from going vacuous; `label` adds the counts to COMPARED so that a property test can
    assert, over its whole run, that something was compared.  `same_order64` (the two property tests, whose sweeps reach
    corners no decoder is meant for): the oracle's float64 LLR-domain result (method 3); codewords on which the ORACLE's
    two float64 formulations already part ways (NaN posteriors in different places, or clamped posteriors further apart
    than 1e-3 relative) are outside what a cross-formulation comparison can say anything about.  Two measured causes:
    (1) on a small graph dense with short cycles, loopy BP saturates within a few iterations and CONTRADICTING
    certainties meet (+inf from one check, -inf from another, or a degree-1 check against a p = 0 prior): the LLR forms
    make inf - inf = NaN or keep the infinity, the package's ratio form multiplies 0 * inf and resets the NaN to 1.0
     and carries on with a finite number (8.06 against inf, both float64); (2) with p = 0 priors on
    an HQC-shaped graph, messages grow past |L| ~ 37, where the float64 ratio form rounds (1 - r) / (1 + r) to exactly
    +-1 and turns "very likely" into "certain": harmless where the posterior is large too (both sides clamp), but a
    variable whose large messages CANCEL (+500 and -512: posterior -11.90 in the LLR form, N=873 W=6 omega=11 eps=0,
    found by the 1000-example soak) comes out as -inf in the ratio form.  The filter uses oracle results only, never
    the device's, and the floor `min_fraction` still applies after it.  `oracle32` (the property tests): the f32 oracle's
    result in the kernel's operation order -- what `compare` has just held the device to, NaN places included.  Codewords
    whose float32 ORACLE has NaN posteriors where the float64 form has none are float32 SATURATION, not a formulation
    matter: on a small graph dense with short cycles (32 checks on 10 variables, column degree ~11: found by the
    3000-example soak of round 4) messages pass |L| = 87.3 within five iterations, become +-inf in float32, and
    contradicting infinities sum to NaN, while float64 still carries finite numbers.  Such codewords are left out
    (oracle results only again).  Returns the fraction compared."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ref64 = oracle.bp_decode_batch(H, probs, x, kind, max_iter, "product_sum", dtype="f64", threads=threads,
                                       early_exit=early)
    keep = ref64["converged"].astype(bool) & (got["iters"] == ref64["iters"])
    if oracle32 is not None:
        keep &= (np.isnan(oracle32["llr"]) == np.isnan(ref64["llr"])).all(axis=1)
    if same_order64 is not None:
        keep &= (np.isnan(ref64["llr"]) == np.isnan(same_order64["llr"])).all(axis=1)
        with np.errstate(invalid="ignore"):
            a64 = np.clip(same_order64["llr"], -REFERENCE_FORM_CLAMP, REFERENCE_FORM_CLAMP)
            b64 = np.clip(ref64["llr"], -REFERENCE_FORM_CLAMP, REFERENCE_FORM_CLAMP)
            apart = np.abs(a64 - b64) > 1e-3 * np.maximum(1.0, np.abs(b64))  # NaN compares False
        keep &= ~apart.any(axis=1)
    frac = float(keep.mean())
    if label is not None:
        c = COMPARED.setdefault(label, [0, 0])
        c[0] += int(keep.sum())
        c[1] += int(keep.size)
    assert frac >= min_fraction, f"only {frac:.3f} of the codewords qualify for the float64 comparison (floor {min_fraction:.3f})"
    if keep.any():
        compare_with_reference_form({k: (v[keep] if v is not None else None) for k, v in got.items()},
                                    {k: (v[keep] if v is not None else None) for k, v in ref64.items()}, tol=tol)
    return frac
