"""The answer key of tests/message_probes.py, checked without a GPU: the closed forms against enumeration (and against
50-digit arithmetic where mpmath is installed), the float32 oracle's own distance from them on every forest and comb the
GPU file uses (tests/test_message_probes_gpu.py measures the device against the same key and derives its bound from
these figures), and that the probes tell formulations apart -- a float32 ratio-domain or textbook tanh rule does NOT pass.

Run with -s for the oracle's error table, worst per (row-degree band, magnitude profile), in u = 2^-24 * max(1, |L|).
"""
import numpy as np
import pytest

import exact
import message_probes as mp
from message_probes import COMB_CASES, FOREST_CASES, PROFILES, comb_case, forest_case, soft_variants

ORACLE_CAP = 16.0  # u; measured worst 6.6 over eight seeds of an earlier set of profiles, 8.4 on these forests
COMB_CAP = 8.0  # u'; measured worst 3.2 on these combs (the summation order's rounding, not the messages')


def oracle_probe(oracle, f, synd, method, max_iter=1, dtype="f32", probs=None, early=False, alpha=1.0):
    with np.errstate(all="ignore"):
        r = oracle.bp_decode_batch(f.graph, f.probs if probs is None else probs, synd, 0, max_iter, method, alpha=alpha,
                                   dtype=dtype, threads=8, early_exit=early)
    return r, r["llr"][:, f.probe[f.rows]]


def print_table(title, cells):
    print(f"\n{title}")
    kinds = sorted({k for _, k in cells})
    print("  band   " + "".join(f"{k:>13s}" for k in kinds))
    for b in mp.BANDS:
        if any(bb == b for bb, _ in cells):
            print(f"  {mp.band_name(b):6s} " + "".join(f"{cells[(b, k)]:13.2f}" if (b, k) in cells else " " * 13 for k in kinds))


# ------------------------------------------------------------------------------------------------ the closed forms
def test_true_message_is_the_enumerated_marginal():
    """Stars of 2 .. 10 edges: the probe's exact posterior (tests/exact.binary_exact: enumeration over all 2^n vectors)
    is `true_message` of the other priors' float64 LLRs, to 1e-12 relative; p on both sides of 1/2, both syndrome bits.
    phi is its own inverse: a degree-2 row's message is the other input."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for n in range(2, 11):
        for _ in range(6):
            # (priors of 1e-5 .. 0.2 on either side: the message stays above 1e-2, where the enumeration's own
            # log-sum-exp difference is good to 1e-12 relative)
            p = 10.0 ** rng.uniform(-5.0, -0.7, n)
            p = np.where(rng.rand(n) < 0.3, 1.0 - p, p)
            probe = int(rng.randint(n))
            p[probe] = 0.5
            x = np.log((1.0 - p) / p)
            H = np.ones((1, n), dtype=np.int8)
            ex = exact.binary_exact(H, p, np.array([[0], [1]], dtype=np.uint8))["sp"]
            for s in (0, 1):
                t = mp.true_message(np.delete(x, probe), s)
                worst = max(worst, abs(ex[s, probe] - t) / abs(t))
    assert worst < 1e-12, worst
    for a in (1e-3, 0.3, 5.58, 40.0, 85.0):
        assert abs(mp.true_message([a]) - a) <= 1e-12 * a and abs(mp.true_message([-a], 1) - a) <= 1e-12 * a
    # the ends: certainties drop out, a row of certainties is certain, an uninformative input silences the row
    assert mp.true_message([np.inf, -2.0, 3.0]) == mp.true_message([-2.0, 3.0])
    assert mp.true_message([np.inf, -np.inf]) == -np.inf and mp.true_message([np.inf, -np.inf], 1) == np.inf
    assert mp.true_message([0.0, 7.0]) == 0.0


def test_true_message_against_50_digit_arithmetic():
    """`true_message` on the magnitudes the forests use (1e-3 .. 85, rows of up to 200 edges) against mpmath at 50
    digits: 1e-13 relative.  (mpmath is optional: without it this part is skipped, the enumeration above stays.)"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    rng = np.random.RandomState(12)
    worst = 0.0
    for d in (2, 3, 17, 64, 200):
        for name, prof in PROFILES.items():
            x = prof(rng, d - 1, d)
            prod = mpmath.mpf(1)
            for a in x:
                prod *= mpmath.tanh(mpmath.mpf(float(a)) / 2)
            ref = 2 * mpmath.atanh(prod)
            worst = max(worst, float(abs(mpmath.mpf(mp.true_message(x)) - ref) / ref))
    assert worst < 1e-13, worst


def test_comb_closed_form_is_the_enumerated_marginal():
    """A comb of hub degree 1 .. 4 (up to 9 variables): `true_comb_posteriors` is the enumerated posterior."""
    rng = np.random.RandomState(13)
    cb = mp.comb(rng, [1, 2, 4][:3])
    # one comb at a time (the enumeration takes up to 18 variables)
    for h, lv, rr in zip(cb.hub, cb.leaves, cb.rows):
        cols = np.concatenate([[h], lv])
        H = np.zeros((len(rr), len(cols)), dtype=np.int8)
        for i in range(len(rr)):
            H[i, 0] = H[i, 1 + i] = 1
        p32 = cb.probs.astype(np.float32).astype(np.float64)[cols]
        synd = (rng.rand(4, len(rr)) < 0.5).astype(np.uint8)
        full = np.zeros((4, cb.m), dtype=np.uint8)
        full[:, rr] = synd
        post, _ = mp.true_comb_posteriors(cb, full)
        ex = exact.binary_exact(H, p32, synd)["sp"]
        # (the key takes the float32 LLRs logf((1 - p) / p): 1e-6 relative from the float64 priors' own)
        assert np.allclose(post[:, cols], ex, rtol=2e-6, atol=2e-6)


# ------------------------------------------------------------------------------------------------ the oracle's distance
@pytest.mark.parametrize("stuck", [False, True])
def test_f32_oracle_is_within_16_u_of_the_truth(oracle, stuck):
    """The float32 oracle in the kernels' operation order (`tanh_complement`) on every probe of every forest, shared and
    per-codeword priors: within 16 u; +-inf and exact-zero corners exact; the table is printed."""
    cells = {}
    for name in FOREST_CASES:
        f, synd = forest_case(name, stuck)
        _, got = oracle_probe(oracle, f, synd, "tanh_complement")
        truth = f.truth(synd)
        for k, v in mp.worst_per_cell(f, mp.errors_in_u(got, truth)).items():
            cells[k] = max(cells.get(k, 0.0), v)
        zero = np.isin(f.kind[f.rows], ["zero_source"])
        assert (got[:, zero] == 0).all() and (truth[:, zero] == 0).all()
        assert np.isinf(truth[:, f.kind[f.rows] == "all_certain"]).all()
        big = np.abs(truth) > mp.unit(truth) * ORACLE_CAP
        assert np.array_equal(np.sign(got)[big], np.sign(truth)[big])
        if stuck:  # ... and per-codeword priors, one oracle call per draw
            p32, kinds, which = soft_variants(name)
            truth = f.truth(synd, p32, which)
            for v in range(len(p32)):
                _, got = oracle_probe(oracle, f, synd[which == v], "tanh_complement", probs=p32[v].astype(np.float64))
                e = mp.errors_in_u(got, truth[which == v])
                for k, w in mp.worst_per_cell(f, e, kinds[v:v + 1]).items():
                    cells[k] = max(cells.get(k, 0.0), w)
    print_table(f"f32 oracle (tanh_complement) against the true message, worst error in u (stuck row: {stuck})", cells)
    assert max(cells.values()) <= ORACLE_CAP, cells
    assert {k for _, k in cells} == set(PROFILES) | set(mp.CORNERS)


def test_probes_tell_formulations_apart(oracle):
    """The same probes with other float32 formulations of the same function: the ratio form (`product_sum`) is outside
    the bound on the 1 .. 12 profile, and it and the textbook LLR form (`product_sum_log`) give non-finite probes on the
    15 .. 40 profile (1 - tanh cancels at |L| ~ 17 in float32).  So the bound is one a cheaper formulation does not meet."""
    f, synd = forest_case("cap64", True)
    truth = f.truth(synd)
    kind = f.kind[f.rows]
    _, ratio = oracle_probe(oracle, f, synd, "product_sum")
    _, textbook = oracle_probe(oracle, f, synd, "product_sum_log")
    e = mp.errors_in_u(ratio, truth)[:, kind == "mid"]
    print(f"\nf32 ratio form on the 1 .. 12 profile: worst {np.nanmax(e):.1f} u")
    assert np.nanmax(e) > 4 * ORACLE_CAP
    assert not np.isfinite(ratio[:, kind == "large"]).all()
    assert not np.isfinite(textbook[:, kind == "large"]).all()
    assert np.isfinite(truth[:, kind == "large"]).all()


@pytest.mark.parametrize("alpha", [1.0, 0.75])
def test_minsum_oracle_probe_is_the_scaled_minimum(oracle, alpha):
    """Min-sum: the probe is +-fl(alpha * min |x|), bit for bit, on every forest (the order of scaling and the FLT_MAX
    start of the running minimum are the oracle's, `true_minsum_message`)."""
    for name in FOREST_CASES:
        f, synd = forest_case(name, True)
        _, got = oracle_probe(oracle, f, synd, "min_sum", max_iter=3, alpha=alpha)
        key = f.truth_minsum(synd, alpha)
        assert got.dtype == np.float32 and np.array_equal(got, key), name
        p32, _, which = soft_variants(name)
        key = f.truth_minsum(synd, alpha, p32, which)
        for v in range(len(p32)):
            _, got = oracle_probe(oracle, f, synd[which == v], "min_sum", alpha=alpha, probs=p32[v].astype(np.float64))
            assert np.array_equal(got, key[which == v]), (name, v)


def test_every_cell_is_informative():
    """Non-vacuity: in every (band, profile) cell of every forest at least 90 % of the probes have |truth| > 1e-3 (a
    message that has underflowed to 0 makes any kernel exact), shared and per-codeword priors; every exact row degree
    2 .. 64 and every band occurs."""
    degs, bands = set(), set()
    for name in FOREST_CASES:
        f, synd = forest_case(name, True)
        p32, kinds, which = soft_variants(name)
        draws = [(f.truth(synd[:1]), f.kind)] + [(f.truth(synd[:1], p32[v]), kinds[v]) for v in range(len(p32))]
        for truth, kind in draws:
            for b in set(f.band[f.rows]):
                for prof in PROFILES:
                    sel = (f.band[f.rows] == b) & (kind[f.rows] == prof)
                    assert sel.sum() >= 2 and (np.abs(truth[0, sel]) > 1e-3).mean() >= 0.9, (name, b, prof)
        degs |= set(f.deg[f.rows])
        bands |= set(f.band[f.rows])
        x = mp.prior32(f.probs)
        assert np.abs(x[np.isfinite(x)]).max() <= 85.0 and np.abs(mp.prior32(p32)[np.isfinite(mp.prior32(p32))]).max() <= 85.0
        neg = (x[np.isfinite(x)] < 0).mean()
        assert 0.05 < neg < 0.35, neg  # negative sources: 30 % of those below 16
    assert set(range(2, 65)) <= degs and bands == set(mp.BANDS)
    assert FOREST_CASES["cap16"][1][-1] == 16 and FOREST_CASES["cap32"][1][-1] == 32 and FOREST_CASES["cap64"][1][-1] == 64
    f, _ = forest_case("lds", True)
    assert 8 * f.graph.nnz + 2 * f.n + f.m + 64 <= 60 * 1024  # the LDS-resident decoder takes it


@pytest.mark.parametrize("method", ["tanh_complement", "min_sum"])
def test_iteration_invariance_and_the_stuck_row(oracle, method):
    """Oracle posteriors on a forest are bit-identical for max_iter 1, 2 and 5 (every iteration recomputes the same
    messages from the same inputs), and with the stuck component an early-exit run goes to max_iter on every codeword:
    iters == max_iter, none converged, the stuck variable's posterior NaN (tanh rule: inf - inf), nothing else touched."""
    for name in ("cap16", "cap200"):
        f, synd = forest_case(name, True)
        runs = [oracle_probe(oracle, f, synd, method, max_iter=it)[0] for it in (1, 2, 5)]
        assert all(np.array_equal(r["llr"], runs[0]["llr"], equal_nan=True) for r in runs[1:])
        early, _ = oracle_probe(oracle, f, synd, method, max_iter=4, early=True)
        assert (early["iters"] == 4).all() and not early["converged"].any()
        assert np.array_equal(early["llr"], runs[0]["llr"], equal_nan=True)
        col = f.graph.col_idx[f.graph.row_ptr[f.stuck]]
        if method == "tanh_complement":
            assert np.isnan(early["llr"][:, col]).all() and np.isnan(early["llr"]).sum() == synd.shape[0]
        g, s0 = forest_case(name, False)  # without it, the same run stops at once somewhere
        free, _ = oracle_probe(oracle, g, s0, method, max_iter=4, early=True)
        assert (free["iters"] < 4).any()


# ------------------------------------------------------------------------------------------------ combs
def test_f32_oracle_on_the_combs(oracle):
    """The variable pass: hub and leaf posteriors of the float32 oracle against the closed-form signed sums, in
    u' = 2^-24 * (sum of |terms|), after 2 and after 5 iterations (bit-identical); tanh rule and min-sum.  No message of
    a comb comes near the float32 saturation."""
    rows = []
    for name in COMB_CASES:
        cb, synd = comb_case(name)
        assert mp.max_comb_message(cb, synd) < 80.0
        assert max(len(lv) for lv in cb.leaves) == max(COMB_CASES[name][1])
        post, un = mp.true_comb_posteriors(cb, synd)
        hub = np.zeros(cb.n, dtype=bool)
        hub[cb.hub] = True
        for method in ("tanh_complement", "min_sum"):
            out = [oracle.bp_decode_batch(cb.graph, cb.probs, synd, 0, it, method, dtype="f32", threads=8, early_exit=False)["llr"]
                   for it in (2, 5)]
            assert np.array_equal(out[0], out[1])
            e = np.abs(out[0] - post) / un
            rows.append((name, method, e[:, hub].max(), e[:, ~hub].max()))
    print("\nf32 oracle on the combs, worst error in u' (hub, leaves)")
    for name, method, eh, el in rows:
        print(f"  {name:7s} {method:16s} {eh:6.2f} {el:6.2f}")
    assert max(max(r[2], r[3]) for r in rows) <= COMB_CAP
