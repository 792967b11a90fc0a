"""Device-side Monte-Carlo trials of the q-ary decoders (scaldpc_mc_qary_run), what can be held without a GPU: the boundary
(header, export, binding, methods), the trial law restated in NumPy against the Bernoulli draw of oracle/mc_oracle.c, and
driver.qary_fer_sweep on a decoder double."""
import importlib
import os
import re

import numpy as np
import pytest

import qary_mc_ref as ref
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
qary = importlib.import_module("sca-ldpc_amd.qary")
driver = importlib.import_module("sca-ldpc_amd.driver")
L = importlib.import_module("sca-ldpc_amd._lib")


def test_the_boundary_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    assert "#define SCALDPC_VERSION 104" in src
    decl = re.search(r"\bint scaldpc_mc_qary_run\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert decl and len(decl.group(1).split(",")) == 17
    for word in ("Philox4x32-10", "x >> 2", "floor(p 2^32)", "smallest k with word < T_k", "never drawn"):
        assert word in src, word  # the trial law is written down next to K6's
    lib = L.load()
    assert lib.scaldpc_version() == 104
    fn = lib.scaldpc_mc_qary_run
    assert len(fn.argtypes) == 17 and fn.restype is not None
    # refused before anything touches a device: no handle
    assert fn(None, None, None, 2, None, None, 0, 0, 1, 0, 0, None, None, None, None, None, None) == L.EINVAL


def test_both_decoder_classes_have_the_methods():
    plain, special = qary.decoder_class("DecoderN450R150V3C7B1"), qary.decoder_class("DecoderN1280R512SW6")
    for cls in (plain, special):
        assert callable(cls.mc_run) and callable(cls.mc_run_device)
    assert plain.mc_run is qary.QaryDecoder.mc_run and special.mc_run is qary.QarySpecialDecoder.mc_run


# --------------------------------------------------------------------------------------------------------------- the trial law
@pytest.mark.parametrize("p", [0.0, 1.0, 0.3, 0.005, 0.5, 1e-12, 1.0 - 2.0**-40])
def test_two_levels_are_the_bernoulli_draw_of_the_oracle(p):
    """K = 2, weights (p, 1 - p): level 0 ("bad") sits exactly where oracle.mc_bernoulli flips -- for p = 0 (never), p = 1
    (always), products with 2^32 that are no integers (0.3, 0.005), one that is (0.5), and the two ends of the word range."""
    seed, first, batch, n = 0x1234567890ABCDEF, (1 << 33) + 3, 9, 14
    lv = ref.draw(seed, first, batch, n, [p, 1.0 - p])
    assert np.array_equal(lv == 0, pyoracle.mc_bernoulli(seed, first, batch, n, None, p).astype(bool))
    assert set(np.unique(lv)) <= {0, 1}


def test_thresholds():
    assert ref.thr(0.3) == 1288490188 and ref.thr(0.3) != 0.3 * 2**32  # floor of a product that is no integer
    assert ref.thresholds([0.0, 1.0]) == [0, 1 << 32] and ref.thresholds([1.0, 0.0]) == [1 << 32, 1 << 32]
    assert ref.thresholds([0.0, 0.25, 0.75]) == [0, 1 << 30, 1 << 32]
    # left to right in float64: 0.1 + 0.2 is not 0.3, and the last threshold is 2^32 whatever the sum rounds to
    T = ref.thresholds([0.1, 0.2, 0.3, 0.4 - 1e-7])
    assert T[1] == int((np.float64(0.1) + np.float64(0.2)) * 4294967296.0) and T[-1] == 1 << 32
    # a level of weight 0 is never drawn, wherever it stands
    w = ref.words(5, 0, 40, 16)
    for weights, never in (([0.0, 0.25, 0.75], 0), ([0.5, 0.0, 0.5], 1), ([0.5, 0.5 - 1e-7, 0.0], 2)):
        lv = ref.levels_of(w, weights)
        assert never not in lv and len(np.unique(lv)) == 2


# ------------------------------------------------------------------------------------------------------------------- the sweep
class FakeDecoder:
    """`mc_run` of a decoder whose channel law is the oracle's Bernoulli draw and that corrects up to two bad symbols (and
    every frame whose global index is a multiple of 7)."""

    calls = []

    def __init__(self, H, iterations):
        self.n = H.shape[1]
        assert H.dtype == np.int8 and iterations == 5

    def mc_run(self, runs, seed, levels, weights, first_trial=0, want_levels=False, want_symbols=False):
        assert np.array_equal(levels, ref.reference_rows()) and levels.dtype == np.float32
        FakeDecoder.calls.append((first_trial, runs))
        errs = pyoracle.mc_bernoulli(seed, first_trial, runs, self.n, None, weights[0]).sum(axis=1).astype(np.int32)
        ok = (errs <= 2) | ((first_trial + np.arange(runs)) % 7 == 0)
        return {"success": ok.astype(np.uint8), "errs": errs, "wrong": np.where(ok, 0, 1).astype(np.int32)}


def fake_class(name):
    assert name == "DecoderN40R20V2C3B1"
    return FakeDecoder


def sweep_H():
    H = np.zeros((20, 40), dtype=np.int8)
    for r in range(20):
        H[r, [r, r + 20, (r + 1) % 20]] = [1, -1, 1]
    return H


def test_the_sweep_counts_the_first_frames_with_a_bad_symbol_whatever_the_chunk():
    H, rate, runs, seed = sweep_H(), 0.04, 150, 77
    errs = pyoracle.mc_bernoulli(seed, 0, 4096, 40, None, rate).sum(axis=1)
    idx = np.flatnonzero(errs > 0)[:runs]
    assert len(idx) == runs and (errs[: idx[-1]] == 0).sum() > 20  # frames are skipped inside the counted range
    ok = (errs[idx] <= 2) | (idx % 7 == 0)
    want = dict(successes=int(ok.sum()), max_errs_success=int(errs[idx][ok].max()), min_errs_fail=int(errs[idx][~ok].min()),
                trials_drawn=int(idx[-1]) + 1)
    assert 0 < want["successes"] < runs and want["max_errs_success"] >= want["min_errs_fail"] >= 3
    for chunk in (64, 100, 4096):
        FakeDecoder.calls = []
        got = driver.qary_fer_sweep(H, 1, rate, runs, seed, chunk=chunk, decoder_class=fake_class)
        assert got == want, chunk
        assert FakeDecoder.calls == [(i * chunk, chunk) for i in range(-(-want["trials_drawn"] // chunk))]
    # nothing failed: None, as the reference leaves it (decode.py:267)
    got = driver.qary_fer_sweep(H, 1, 0.002, 5, seed, chunk=100, decoder_class=fake_class)
    assert got["min_errs_fail"] is None and got["successes"] == 5 and got["max_errs_success"] >= 1
    assert driver.qary_fer_sweep(H, 1, rate, 0, seed, decoder_class=fake_class) == dict(successes=0, max_errs_success=0,
                                                                                          min_errs_fail=None, trials_drawn=0)
    with pytest.raises(ValueError):
        driver.qary_fer_sweep(H, 1, 0.0, 5, seed, decoder_class=fake_class)
