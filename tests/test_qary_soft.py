"""Soft output of the q-ary decoders, the part that needs no GPU (tests/test_qary_soft_gpu.py holds the kernels to it):

(a) tests/qary_soft_ref.py -- the NumPy float32 restatement that KEEPS the last variable update's totals -- decides what the
    CPU oracle decides (oracle/qary_oracle.c: the reference's loop), on trees and on graphs with cycles;
(b) its totals are the truth where the truth is known: on cycle-free graphs a row of totals minus its minimum is the exact
    min-marginal cost difference, and the margin is the gap between the two best symbols (tests/exact.tree_exact_qary, (min, +)
    elimination in float64; nothing shared with the decoders' sweeps);
(c) the interface is bound: header, exported symbols, ctypes argtypes, version.

Bound of (b): the restatement's worst absolute deviation over every entry of the case list below, measured on the CPU, is
1.86e-6 (totals) and 7.7e-7 (margins) over 5876 finite entries, cost differences up to 15.1 (852 more entries are infinite);
the bound is 4x the larger, 7.5e-6 -- the rounding of a few dozen fp32 additions of such numbers (ulp(8) = 9.5e-7) plus that
of the fp32 LLRs themselves."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

import exact
import qary_soft_ref as ref
from test_exact_inference import large_qary_tree_case, large_special_tree_case, qary_tree_case, special_tree_case

S = importlib.import_module("sca-ldpc_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 7.5e-6  # 4 x the measured 1.86e-6 (module docstring)
WORST = {"cost": 0.0, "margin": 0.0, "entries": 0, "infinite": 0, "top": 0.0}


def crossing_iterations(H):
    """Flooding iterations after which every variable has heard from every other on a forest: a path crosses at most
    R checks, one per iteration."""
    return H.shape[0] + 1


def against_exact(mm_rows, got_cost_rows, got_margin):
    """One codeword: exact min-marginal rows (float64) against the restatement's totals and margins.  EVERY entry is
    compared: finite ones by value after subtracting the row minimum, infinite ones must be +inf or NaN."""
    for v, (mm, row) in enumerate(zip(mm_rows, got_cost_rows)):
        mm = np.asarray(mm, dtype=np.float64)
        fin = np.isfinite(mm)
        assert fin.any()
        with np.errstate(invalid="ignore"):
            norm = row.astype(np.float64) - np.nanmin(np.where(np.isfinite(row), row, np.nan))
        dev = np.abs(norm[fin] - (mm[fin] - mm[fin].min()))
        assert np.isfinite(row[fin]).all()
        assert (np.isposinf(row[~fin]) | np.isnan(row[~fin])).all(), (v, mm, row)
        srt = np.sort(mm)
        WORST["cost"] = max(WORST["cost"], float(dev.max()))
        WORST["top"] = max(WORST["top"], float((mm[fin] - mm[fin].min()).max()))
        WORST["entries"] += int(fin.sum())
        WORST["infinite"] += int((~fin).sum())
        assert dev.max() <= BOUND, (v, dev.max())
        if np.isfinite(srt[1]):
            mdev = abs(float(got_margin[v]) - (srt[1] - srt[0]))
            WORST["margin"] = max(WORST["margin"], mdev)
            assert mdev <= BOUND, (v, mdev)
        else:  # one possible symbol: no runner-up
            assert np.isposinf(got_margin[v]) or np.isnan(got_margin[v])


# ------------------------------------------------------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("seed", range(10))
def test_plain_decoder_on_small_trees(oracle, B, seed):
    H, pmf, best = qary_tree_case(seed, B, batch=4)
    it = crossing_iterations(H)
    g = S.TannerGraph.from_dense(H)
    with np.errstate(divide="ignore"):
        want = oracle.qary_min_sum_batch(g, 2 * B + 1, pmf, it)
    r = ref.min_sum_soft(oracle, H, B, pmf, it)
    assert np.array_equal(r["symbols"], want) and np.array_equal(want, best)
    assert not r["unmet"].any()  # the optimum of a tree is a valid word
    for b in range(len(pmf)):
        against_exact(exact.tree_exact_qary(H, exact.pmf_to_llr64(pmf[b]), B), r["costs"][b], r["margins"][b])


@pytest.mark.parametrize("seed", range(12))
def test_special_decoder_on_small_trees(oracle, seed):
    H, pb, ps, best = special_tree_case(seed, batch=2)
    R, N = H.shape
    it = crossing_iterations(H)
    want = oracle.qary_special_batch(S.TannerGraph.from_dense(H), 2, 12, pb, ps, it)
    r = ref.special_min_sum_soft(oracle, H, 2, 12, pb, ps, it)
    assert np.array_equal(r["symbols"], want) and np.array_equal(want, best)
    assert not r["unmet"].any()
    for b in range(len(pb)):
        llr = [exact.pmf_to_llr64(pb[b][v]) for v in range(N - R)] + [exact.pmf_to_llr64(ps[b][c]) for c in range(R)]
        mm = exact.tree_exact_qary(H, llr, [2] * (N - R) + [12] * R)
        against_exact(mm, list(r["costs"][b]) + list(r["costs_sum"][b]), r["margins"][b])


def test_plain_decoder_on_a_large_tree(oracle):
    """250 variables (tests/test_exact_inference.py's case): totals against the exact min-marginals of every variable."""
    H, pmf, dec, ok = large_qary_tree_case(250, 1, 2, seed=41)
    r = ref.min_sum_soft(oracle, H, 1, pmf, 80)
    assert np.array_equal(r["symbols"], oracle.qary_min_sum_batch(S.TannerGraph.from_dense(H), 3, pmf, 80))
    assert np.array_equal(r["symbols"][ok], dec[ok])
    for b in range(len(pmf)):
        against_exact(exact.tree_exact_qary(H, exact.pmf_to_llr64(pmf[b]), 1), r["costs"][b], r["margins"][b])


def test_special_decoder_on_a_large_tree(oracle):
    H, pb, ps, dec, ok = large_special_tree_case(16, 2, seed=70)
    R, N = H.shape
    r = ref.special_min_sum_soft(oracle, H, 2, 12, pb, ps, R + 1)
    assert np.array_equal(r["symbols"], oracle.qary_special_batch(S.TannerGraph.from_dense(H), 2, 12, pb, ps, R + 1))
    assert np.array_equal(r["symbols"][ok], dec[ok])
    for b in range(len(pb)):
        llr = [exact.pmf_to_llr64(pb[b][v]) for v in range(N - R)] + [exact.pmf_to_llr64(ps[b][c]) for c in range(R)]
        against_exact(exact.tree_exact_qary(H, llr, [2] * (N - R) + [12] * R), list(r["costs"][b]) + list(r["costs_sum"][b]),
                      r["margins"][b])


def test_the_measured_deviation_is_what_the_bound_was_set_from():
    """Runs after the tree tests of this module: prints the figures the bound rests on and checks that something infinite
    and a good many finite entries were compared (nothing is left out of the comparison)."""
    print(f"worst |total - exact| {WORST['cost']:.3g}, worst |margin - exact| {WORST['margin']:.3g} over {WORST['entries']} finite "
          f"entries (costs up to {WORST['top']:.3g}), {WORST['infinite']} infinite ones; bound {BOUND:.3g}")
    if WORST["entries"]:  # (the module was run as a whole)
        assert WORST["entries"] > 3000 and WORST["infinite"] > 20
        assert max(WORST["cost"], WORST["margin"]) <= BOUND


def test_graphs_with_cycles_decide_as_the_oracle_does(oracle):
    """The 6 x 3 Q = 15 instance (decoder.rs:771-799) and Q = 3 / 5 / 7 graphs with cycles: the restatement's symbols are the
    oracle's at 1, 2 and 5 iterations; its margins and unmet counts follow their definitions."""
    cases = [ref.q15_instance(4), ref.cyclic_instance(1, 6, seed=3), ref.cyclic_instance(2, 3, seed=5), ref.cyclic_instance(3, 2, seed=7)]
    unmet_seen = set()
    for H, B, pmf in cases:
        g = S.TannerGraph.from_dense(H)
        for it in (1, 2, 5):
            with np.errstate(divide="ignore"):
                want = oracle.qary_min_sum_batch(g, 2 * B + 1, pmf, it)
                r = ref.min_sum_soft(oracle, H, B, pmf, it)
            assert np.array_equal(r["symbols"], want), (B, it)
            assert np.array_equal(r["unmet"], [(H.astype(int) @ x.astype(int) != 0).sum() for x in want])
            unmet_seen |= set(int(u) > 0 for u in r["unmet"])
            srt = np.sort(np.where(np.isnan(r["costs"]), np.inf, r["costs"]), axis=2)
            with np.errstate(invalid="ignore"):
                gap = (srt[..., 1] - srt[..., 0]).astype(np.float32)
            sel = np.isfinite(srt[..., 0])  # a decided symbol with a finite total: the margin is the gap of the two smallest
            assert ref.same_bits(r["margins"][sel], gap[sel])
    assert unmet_seen == {False, True}


def test_the_oracles_last_totals_are_the_restatements_bit_for_bit(oracle):
    """oracle/qary_oracle.c hands out the totals of its last variable pass (qary_min_sum_soft_batch / qary_special_soft_batch:
    the fast answer key of tests/test_qary_shapes_gpu.py).  On every case of this module -- the small and the large trees of both
    decoders, the graphs with cycles at 1, 2 and 5 iterations -- they are the slow restatement's as uint32 bit patterns (any
    NaN equal to any NaN), and so are its symbols; a good part of the totals is +inf (symbols of probability 0)."""
    seen = {"finite": 0, "inf": 0, "nan": 0}

    def tally(*tables):
        for t in tables:
            seen["finite"] += int(np.isfinite(t).sum())
            seen["inf"] += int(np.isposinf(t).sum())
            seen["nan"] += int(np.isnan(t).sum())

    def plain(H, B, pmf, it):
        with np.errstate(divide="ignore"):
            r = ref.min_sum_soft(oracle, H, B, pmf, it)
            sym, cost = oracle.qary_min_sum_soft_batch(S.TannerGraph.from_dense(H), 2 * B + 1, pmf, it, threads=2)
        assert np.array_equal(sym, r["symbols"]) and cost.dtype == np.float32 and cost.shape == r["costs"].shape
        assert ref.same_bits(cost, r["costs"]), (B, it)
        tally(cost)

    def special(H, B, BSUM, pb, ps, it):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = ref.special_min_sum_soft(oracle, H, B, BSUM, pb, ps, it)
            sym, cb, cs = oracle.qary_special_soft_batch(S.TannerGraph.from_dense(H), B, BSUM, pb, ps, it, threads=2)
        assert np.array_equal(sym, r["symbols"]) and cb.shape == r["costs"].shape and cs.shape == r["costs_sum"].shape
        assert ref.same_bits(cb, r["costs"]) and ref.same_bits(cs, r["costs_sum"]), it
        tally(cb, cs)

    for B in (1, 2):
        for seed in range(10):
            H, pmf, _ = qary_tree_case(seed, B, batch=4)
            plain(H, B, pmf, crossing_iterations(H))
    for seed in range(12):
        H, pb, ps, _ = special_tree_case(seed, batch=2)
        special(H, 2, 12, pb, ps, crossing_iterations(H))
    H, pmf, _, _ = large_qary_tree_case(250, 1, 2, seed=41)
    plain(H, 1, pmf, 80)
    H, pb, ps, _, _ = large_special_tree_case(16, 2, seed=70)
    special(H, 2, 12, pb, ps, H.shape[0] + 1)
    for H, B, pmf in (ref.q15_instance(4), ref.cyclic_instance(1, 6, seed=3), ref.cyclic_instance(2, 3, seed=5), ref.cyclic_instance(3, 2, seed=7)):
        for it in (1, 2, 5):
            plain(H, B, pmf, it)
    print(f"totals compared: {seen}")
    assert seen["finite"] > 3000 and seen["inf"] > 20, seen
    # a variable no check holds: its totals are its channel LLRs (nothing is added), through the same copy
    H, B, pmf = ref.cyclic_instance(2, 3, seed=11, R=4, N=9)
    H[:, 4] = 0
    plain(H, B, pmf, 2)


def test_margin_rule_on_hand_made_rows():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    f = lambda *x: ref.margin_of(np.array(x, dtype=np.float32))  # noqa: E731
    assert f(1.0, 3.0, 2.0) == 1.0 and f(2.0, 2.0, 5.0) == 0.0  # two equal minima: 0
    assert f(nan, 4.0, 1.0) == 3.0  # NaN never selected, never the runner-up
    assert f(1.0, inf, inf) == inf and f(1.0, nan, nan) == inf  # no candidate: +inf
    assert np.isnan(f(inf, inf, inf)) and f(nan, inf, 2.0) == inf
    assert ref.first_min(np.array([nan, inf, inf], dtype=np.float32)) == 0  # nothing selected: index 0 (decoder.rs:694-704)
    assert np.isnan(f(nan, inf, inf))  # ... and inf - NaN


# ------------------------------------------------------------------------------------------------------------------------ (c)
def test_the_interface_is_bound():
    """Header, library, ctypes binding and Python surface of the two soft entry points; the version is 104."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scaldpc.h")).read(), flags=re.S)
    L = importlib.import_module("sca-ldpc_amd._lib")
    lib = L.load()
    for name, nargs in (("scaldpc_qary_min_sum_batch_soft", 9), ("scaldpc_qary_special_min_sum_batch_soft", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/scaldpc.h"
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(lib, name), f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert lib.scaldpc_version() == 104 and "#define SCALDPC_VERSION 104" in hdr
    # NULL handle: an error code with a message, not a crash
    assert lib.scaldpc_qary_min_sum_batch_soft(None, None, 1, 0, None, None, None, None, None) == L.EINVAL
    assert lib.scaldpc_qary_special_min_sum_batch_soft(None, None, None, 1, 0, None, None, None, None, None, None) == L.EINVAL
    qary = importlib.import_module("sca-ldpc_amd.qary")
    drop = os.path.join(ROOT, "sca-ldpc_amd", "dropin")
    if drop not in sys.path:
        sys.path.insert(0, drop)
    import simulate_rs

    for cls in (qary.QaryDecoder, qary.QarySpecialDecoder, getattr(simulate_rs, "DecoderN1280R512SW6"),
                getattr(simulate_rs, "DecoderN450R150V3C7B1")):
        for meth in ("min_sum_soft", "min_sum_soft_batch", "min_sum_soft_batch_device"):
            assert callable(getattr(cls, meth))
