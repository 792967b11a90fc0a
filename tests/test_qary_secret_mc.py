"""Monte-Carlo trials of DecoderSpecial on drawn secrets (scaldpc_mc_qary_run_secret), what can be held without a GPU: the
boundary, `trials.oracle_posterior_table` against numbers minted from the reference (tests/golden/kyber_posteriors.json), the
trial law restated in NumPy (tests/qary_secret_ref.py), the host header that validates the tables and builds the law
(csrc/scaldpc_mc_law.h, driven by tests/qary_secret_law_main.cc under the address and undefined-behaviour sanitizers where the
toolchain has their runtimes), and driver.kyber_fer_sweep on a decoder double."""
import importlib
import json
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import qary_mc_ref as mc
import qary_secret_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
trials = importlib.import_module("sca-ldpc_amd.trials")
driver = importlib.import_module("sca-ldpc_amd.driver")
qary = importlib.import_module("sca-ldpc_amd.qary")
L = importlib.import_module("sca-ldpc_amd._lib")


def test_the_boundary_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    assert "#define SCALDPC_VERSION 104" in src
    decl = re.search(r"\bint scaldpc_mc_qary_run_secret\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert decl and len(decl.group(1).split(",")) == 19
    for word in ("v >> 2, 1, trial_lo, trial_hi", "word v & 3", "t_r = -h_{r,id} * sum_j h_{r,j} s_j", "smallest k with word < T^s_k",
                 "never drawn under that symbol", "Defining property", "Reduction", "4 (2 K Q + Q) > 65536"):
        assert word in src, word  # the trial law is written down next to the others
    lib = L.load()
    assert lib.scaldpc_version() == 104
    fn = lib.scaldpc_mc_qary_run_secret
    assert len(fn.argtypes) == 19 and fn.restype is not None
    # refused before anything touches a device: no handle
    assert fn(None, None, None, None, 2, None, None, 2, 0, 1, 0, 0, None, None, None, None, None, None, None) == L.EINVAL
    special = qary.decoder_class("DecoderN1280R512SW6")
    assert callable(special.mc_run_secret) and callable(special.mc_run_secret_device)
    assert not hasattr(qary.decoder_class("DecoderN450R150V3C7B1"), "mc_run_secret")  # a drawn secret needs the row-sum variables


# ------------------------------------------------------------------------------------------------- the oracle's posterior table
with open(os.path.join(ROOT, "tests", "golden", "kyber_posteriors.json")) as _fh:
    GOLDEN = json.load(_fh)["cases"]


def _accuracy(c):
    return c["accuracy"] if isinstance(c["accuracy"], float) else [tuple(p) for p in c["accuracy"]]


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['name']}-{c['accuracy'] if isinstance(c['accuracy'], float) else 'positional'}" for c in GOLDEN])
def test_oracle_posterior_table_is_the_reference(case):
    """pr_cond_yx and s_distribution_from_hard_y, restated with the same order of float64 operations: equal, not close."""
    coding = [tuple(c) for c in case["coding"]]
    t = trials.oracle_posterior_table(coding, case["prior"], _accuracy(case))
    assert [list(y) for y in t["answers"]] == case["answers"]
    assert t["levels"].dtype == np.float64 and t["weights"].dtype == np.float64
    assert np.array_equal(t["levels"], np.array(case["levels"])) and np.array_equal(t["weights"], np.array(case["weights_by_answer"]).T)
    Q, K = len(coding), len(case["answers"])
    assert t["levels"].shape == (K, Q) and t["weights"].shape == (Q, K)
    assert np.abs(t["weights"].sum(axis=1) - 1.0).max() <= 1e-12 and np.abs(t["levels"].sum(axis=1) - 1.0).max() <= 1e-12
    # the table of t = -s: the symbol axis reversed, nothing else
    r = trials.oracle_posterior_table(coding, case["prior"], _accuracy(case), reverse=True)
    assert r["answers"] == t["answers"] and np.array_equal(r["levels"], t["levels"][:, ::-1]) and np.array_equal(r["weights"], t["weights"][::-1])
    assert r["levels"].flags.c_contiguous and r["weights"].flags.c_contiguous


def test_answers_of_probability_zero_are_dropped():
    """At accuracy 1.0 only the code words themselves are answered: 5 of 8 and 13 of 16 answers remain, the others (which make
    the reference divide by zero) are the ones the golden file lists as dropped."""
    seen = 0
    for c in GOLDEN:
        if c["accuracy"] == 1.0:
            t = trials.oracle_posterior_table([tuple(x) for x in c["coding"]], c["prior"], 1.0)
            all_answers = {tuple(a) for a in c["answers"]} | {tuple(d) for d in c["dropped"]}
            assert len(all_answers) == 2 ** len(c["coding"][0]) and len(t["answers"]) == len(set(map(tuple, c["coding"])))
            assert set(t["answers"]) == set(map(tuple, c["coding"])) and ((t["weights"] == 0) | (t["weights"] == 1)).all()
            seen += len(c["dropped"])
        else:
            assert not c["dropped"]
    assert seen == 3 + 3


def test_oracle_posterior_table_refuses_what_does_not_fit():
    pr = trials.centered_binomial(2)
    with pytest.raises(ValueError):
        trials.oracle_posterior_table(ref.expansion(5, 6), pr, 0.9)  # 64 outcomes
    assert trials.oracle_posterior_table(ref.expansion(5, 5), pr, 0.9)["levels"].shape == (32, 5)
    with pytest.raises(ValueError):
        trials.oracle_posterior_table(ref.PARITY_5, pr[:4], 0.9)
    with pytest.raises(ValueError):
        trials.oracle_posterior_table(ref.PARITY_5, pr, 1.5)
    with pytest.raises(ValueError):
        trials.oracle_posterior_table(ref.SHARED_5, pr, [(0.1, 0.1)])  # one pair for two bits
    with pytest.raises(ValueError):
        trials.oracle_posterior_table([(0, 0), (1,), (0, 1), (1, 1), (0, 0)], pr, 0.9)
    # a single bit may be given bare
    assert np.array_equal(trials.oracle_posterior_table([0, 1, 0, 1, 0], pr, 0.9)["levels"], trials.oracle_posterior_table(ref.PARITY_5, pr, 0.9)["levels"])


def test_centered_binomial_is_the_secret_distribution():
    assert trials.centered_binomial(2).tolist() == [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16]  # kyber.py:60-64 with ETA = 2
    assert trials.centered_binomial(3).tolist() == [x / 64 for x in (1, 6, 15, 20, 15, 6, 1)]
    w = trials.centered_binomial(2, 3)
    assert w.shape == (13,) and w.sum() == 1.0 and w[6] == 924 / 4096 and np.array_equal(w, w[::-1])
    with pytest.raises(ValueError):
        trials.centered_binomial(0)


# --------------------------------------------------------------------------------------------------------------- the trial law
def toy_H():
    """5 x 13 = [H' | +-I] over 8 coefficients: rows of 3, 2, 0, 3 and 1 coefficient edges, two identity entries -1."""
    H = np.zeros((5, 13), dtype=np.int8)
    H[0, [0, 3, 5]] = [1, -1, 1]
    H[1, [1, 7]] = [-1, -1]
    H[3, [2, 4, 6]] = [1, 1, -1]
    H[4, [5]] = [-1]
    H[np.arange(5), 8 + np.arange(5)] = [1, -1, 1, -1, 1]
    return H


def toy_tables():
    prior = np.array([0.0, 0.3, 0.45, 0.25, 0.0])  # the values -2 and +2 are never the secret
    wb = np.array([[1.0, 0.0, 0.0], [0.5, 0.0, 0.5], [0.0, 0.25, 0.75], [0.1, 0.9, 0.0], [0.0, 0.0, 1.0]])  # weight 0 in every place
    ws = np.random.RandomState(4).dirichlet(np.ones(4), size=13)
    ws[:, 1] = 0.0
    ws /= ws.sum(axis=1, keepdims=True)
    return prior, wb, ws


def test_every_drawn_word_is_a_code_word_and_zero_weights_are_never_drawn():
    H = toy_H()
    prior, wb, ws = toy_tables()
    sec, lv = ref.draw(H, 2, 6, 77, (1 << 32) - 1000, 2000, prior, wb, ws)
    assert sec.dtype == np.int8 and lv.dtype == np.uint8 and sec.shape == lv.shape == (2000, 13)
    assert not (H.astype(np.int64) @ sec.T.astype(np.int64)).any()  # H x = 0 over the integers
    assert (sec[:, 10] == 0).all() and np.array_equal(sec[:, 12], sec[:, 5])  # no coefficient edge; -(+1)(-1) s_5
    assert np.array_equal(sec[:, 9], -sec[:, 1] - sec[:, 7])  # t = -(-1)(-s_1 - s_7)
    # 2000 trials x 8 variables: symbols of prior 0 and outcomes of weight 0 under the variable's own symbol never appear
    s = sec[:, :8] + 2
    assert set(np.unique(s)) == {1, 2, 3}
    assert (wb[s, lv[:, :8]] > 0).all() and (ws[sec[:, 8:] + 6, lv[:, 8:]] > 0).all() and 1 not in lv[:, 8:]
    for sym, drawn in ((1, {0, 2}), (2, {1, 2}), (3, {0, 1})):
        assert set(np.unique(lv[:, :8][s == sym])) == drawn
    # frequencies within 5 sigma of the prior
    n = s.size
    for sym in (1, 2, 3):
        p = prior[sym]
        assert abs((s == sym).sum() - n * p) <= 5 * np.sqrt(n * p * (1 - p)), sym
    # a trial is its global index: any split, and another seed differs
    a, b = ref.draw(H, 2, 6, 77, (1 << 32) - 1000, 30, prior, wb, ws), ref.draw(H, 2, 6, 77, (1 << 32) - 970, 20, prior, wb, ws)
    assert np.array_equal(np.concatenate([a[0], b[0]]), sec[:50]) and np.array_equal(np.concatenate([a[1], b[1]]), lv[:50])
    assert not np.array_equal(ref.draw(H, 2, 6, 78, (1 << 32) - 1000, 30, prior, wb, ws)[0], sec[:30])


def test_equal_rows_and_a_point_mass_prior_are_the_plain_draw():
    H = toy_H()
    wb, ws = np.array([0.2, 0.0, 0.8]), np.array([0.1, 0.15, 0.5, 0.25])
    point = np.array([0.0, 0.0, 1.0, 0.0, 0.0])
    sec, lv = ref.draw(H, 2, 6, 5, 123, 40, point, np.tile(wb, (5, 1)), np.tile(ws, (13, 1)))
    assert not sec.any() and np.array_equal(lv, mc.draw(5, 123, 40, 8, wb, 5, ws))


def test_results_follow_from_the_arrays():
    lb = np.array([[0.1, 0.2, 0.4, 0.2, 0.1], [0.3, 0.3, 0.2, 0.1, 0.1], [0.0, 0.0, 0.0, 0.5, 0.5]], dtype=np.float32)
    ls = np.eye(13, dtype=np.float32)[[6, 0]]
    assert ref.best_symbols(lb, 2).tolist() == [0, -2, 1] and ref.best_symbols(ls, 6).tolist() == [0, -6]  # the FIRST maximum
    secret = np.array([[0, -2, 1, 0, -6], [0, 0, 0, 0, 0]], dtype=np.int8)
    levels = np.array([[0, 1, 2, 0, 1], [0, 1, 2, 0, 1]], dtype=np.uint8)
    symbols = np.array([[0, -2, 1, 1, -6], [1, 0, 0, 0, 0]], dtype=np.int8)
    r = ref.results(secret, levels, symbols, 3, lb, ls, 2, 6)
    assert r["success"].tolist() == [1, 0] and r["wrong"].tolist() == [[0, 1], [1, 0]] and r["channel_wrong"].tolist() == [[0, 0], [2, 1]]
    assert (r["success"].dtype, r["wrong"].dtype, r["channel_wrong"].dtype) == (np.uint8, np.int32, np.int32)


# -------------------------------------------------------------------------------------------- the host header, under the sanitizers
@pytest.fixture(scope="module")
def law_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("secret_law") / "qary_secret_law_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "qary_secret_law_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: qary_secret_law_main is built without them")
        subprocess.check_call(cmd)

    def run(calls):
        """calls: [dict(prior, lb, wb, ls, ws, first=0, batch=1, async_=0, null=0)] -> one parsed line each, out of ONE process."""
        text = ""
        for c in calls:
            lb, wb, ls, ws = (np.asarray(c[k], dtype=np.float64) for k in ("lb", "wb", "ls", "ws"))
            head = [wb.shape[0], wb.shape[1], ws.shape[0], ws.shape[1], c.get("first", 0), c.get("batch", 1), c.get("async_", 0), c.get("null", 0)]
            nums = [x for a in (c["prior"], lb, wb, ls, ws) for x in np.asarray(a, dtype=np.float64).reshape(-1)]
            text += " ".join([str(int(x)) for x in head] + [repr(float(x)) for x in nums]) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        lines = out.stdout.splitlines()
        assert len(lines) == len(calls)
        res = []
        for ln in lines:
            kind = int(ln.split()[0].split("=")[1])
            if kind:
                res.append(dict(refused=kind, why=ln.split(" ", 1)[1]))
                continue
            p = dict(kv.split("=") for kv in ln.split()[1:])
            res.append(dict(refused=0, **{k: [int(x) for x in v.split(",")] for k, v in p.items()}))
        return res

    return run


def random_call(seed, Qb, Kb, Qs, Ks):
    rng = np.random.RandomState(seed)
    wb, ws = rng.dirichlet(np.ones(Kb), size=Qb), rng.dirichlet(np.ones(Ks), size=Qs)
    wb[rng.rand(Qb, Kb) < 0.3] = 0.0  # zero weights in the middle and at the end of rows
    ws[rng.rand(Qs, Ks) < 0.3] = 0.0
    wb[:, 0] += 1e-3
    ws[:, 0] += 1e-3
    wb, ws = wb / wb.sum(axis=1, keepdims=True), ws / ws.sum(axis=1, keepdims=True)
    prior = rng.dirichlet(np.ones(Qb))
    prior[-1] = 0.0
    lb, ls = rng.dirichlet(np.ones(Qb), size=Kb).astype(np.float32), rng.dirichlet(np.ones(Qs), size=Ks).astype(np.float32)
    lb[0, :2] = lb[0].max() + 0.25  # two equal maxima: the first one decides
    lb[0] /= lb[0].sum()
    return dict(prior=prior / prior.sum(), lb=lb, wb=wb, ls=ls, ws=ws)


def test_the_program_takes_only_the_law_header():
    src = open(os.path.join(ROOT, "tests", "qary_secret_law_main.cc")).read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include \"")] == ['"../sca-ldpc_amd/csrc/scaldpc_mc_law.h"']
    hdr = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_mc_law.h")).read()
    assert "mc_qary_secret_law" in hdr and not [ln for ln in hdr.splitlines() if ln.startswith("#include") and "hip" in ln.lower()]


def test_the_law_the_host_builds(law_program):
    calls = [random_call(1, 5, 4, 13, 16), random_call(2, 3, 1, 7, 32), random_call(3, 7, 32, 37, 9), random_call(4, 5, 2, 255, 31)]
    for c, got in zip(calls, law_program(calls)):
        assert got["refused"] == 0
        assert got["prior"] == mc.thresholds(c["prior"]) and got["prior"][-1] == 1 << 32
        assert got["tb"] == [t for row in c["wb"] for t in mc.thresholds(row)]
        assert got["ts"] == [t for row in c["ws"] for t in mc.thresholds(row)]
        B, BSUM = (c["wb"].shape[0] - 1) // 2, (c["ws"].shape[0] - 1) // 2
        assert got["bestb"] == ref.best_symbols(c["lb"], B).tolist() and got["bests"] == ref.best_symbols(c["ls"], BSUM).tolist()
        assert got["bestb"][0] == -B  # the first of two equal maxima


def test_every_refusal(law_program):
    base = random_call(9, 5, 3, 13, 4)
    EINVAL, EPMF, EDEGREE = 1, 2, 3

    def tab(K, Q):
        return np.tile(np.full(Q, 1.0 / Q), (K, 1)), np.tile(np.full(K, 1.0 / K), (Q, 1)) if K else np.zeros((Q, 0))

    def with_b(K):
        lb, wb = tab(K, 5)
        return dict(base, lb=lb, wb=wb)

    def with_s(K, Q=13):
        ls, ws = tab(K, Q)
        return dict(base, ls=ls, ws=ws)

    def row(key, r, values):
        a = np.array(base[key], dtype=np.float64)
        a[r] = values
        return dict(base, **{key: a})

    refusals = {
        "NULL prior": (dict(base, null=1), EINVAL, "NULL"), "NULL levels_b": (dict(base, null=2), EINVAL, "NULL"),
        "NULL weights_b": (dict(base, null=4), EINVAL, "NULL"), "NULL levels_s": (dict(base, null=8), EINVAL, "NULL"),
        "NULL weights_s": (dict(base, null=16), EINVAL, "NULL"),
        "no level": (with_b(0), EINVAL, "levels_b"), "33 levels": (with_b(33), EINVAL, "levels_b"),
        "no sum level": (with_s(0), EINVAL, "levels_s"), "33 sum levels": (with_s(33), EINVAL, "levels_s"),
        "a negative prior": (dict(base, prior=[-0.1, 0.5, 0.6, 0.0, 0.0]), EINVAL, "prior_b"),
        "a NaN prior": (dict(base, prior=[np.nan, 0.5, 0.5, 0.0, 0.0]), EINVAL, "prior_b"),
        "a prior that does not sum to 1": (dict(base, prior=[0.2, 0.2, 0.2, 0.2, 0.2 - 1e-5]), EINVAL, "prior_b"),
        "a weight above 1": (row("wb", 3, [1.5, 0.0, 0.0]), EINVAL, "weights_b[3]"),
        "an infinite weight": (row("wb", 0, [np.inf, 0.0, 0.0]), EINVAL, "weights_b[0]"),
        "a row that does not sum to 1": (row("wb", 4, [0.5, 0.25, 0.25 + 1e-5]), EINVAL, "weights_b[4]"),
        "a negative sum weight": (row("ws", 12, [-0.5, 0.5, 0.5, 0.5]), EINVAL, "weights_s[12]"),
        "a sum row of zeros": (row("ws", 7, [0.0, 0.0, 0.0, 0.0]), EINVAL, "weights_s[7]"),
        "a level that does not sum to 1": (row("lb", 1, [0.3, 0.3, 0.3, 0.0, 0.0]), EPMF, "levels_b: level 1"),
        "a NaN level": (row("ls", 2, [np.nan] * 13), EPMF, "levels_s: level 2"),
        "a negative first trial": (dict(base, first=-1), EINVAL, "first_trial"), "no trial": (dict(base, batch=0), EINVAL, "batch"),
        "a negative batch": (dict(base, batch=-3), EINVAL, "batch"), "asynchronous": (dict(base, async_=1), EINVAL, "SCALDPC_F_ASYNC"),
        "more than 64 KB of LDS": (with_s(32, 253), EDEGREE, "LDS"),
    }
    names = list(refusals)
    for n, got in zip(names, law_program([refusals[n][0] for n in names])):
        assert got["refused"] == refusals[n][1] and refusals[n][2] in got["why"], (n, got)
    # ... and their neighbours that are taken: 32 levels, sums within 1e-6, the largest table that fits (4 (2 K Q + Q) <= 65536)
    ok = law_program([with_b(32), with_s(32), row("wb", 4, [0.5, 0.25, 0.25 + 5e-7]), with_s(31, 255), with_s(32, 251), dict(base, first=1 << 40)])
    assert [g["refused"] for g in ok] == [0] * 6
    assert 4 * (2 * 32 * 251 + 251) <= 65536 < 4 * (2 * 32 * 253 + 253)


# ------------------------------------------------------------------------------------------------------------------- the sweep
class FakeSpecial:
    """`mc_run_secret` of a decoder double: trial i has i % 4 wrong coefficients after decoding (recovered iff that is 0),
    i % 3 wrong row sums, and 5 + i % 2 coefficients its rows alone get wrong."""

    calls = []

    def __init__(self, H, iterations):
        assert H.dtype == np.int8 and H.shape == (5, 13) and iterations == 3
        self.closed = False
        FakeSpecial.last = self

    def mc_run_secret(self, runs, seed, prior, levels, weights, levels_sum, weights_sum, first_trial=0, want_secret=False,
                      want_levels=False, want_symbols=False):
        assert seed == 21 and len(prior) == 5 and np.shape(levels) == (4, 5) and np.shape(weights_sum) == (13, 16)
        FakeSpecial.calls.append((first_trial, runs))
        i = first_trial + np.arange(runs)
        return {"success": (i % 4 == 0).astype(np.uint8), "wrong": np.stack([i % 4, i % 3], axis=1).astype(np.int32),
                "channel_wrong": np.stack([5 + i % 2, i % 5], axis=1).astype(np.int32)}

    def close(self):
        self.closed = True


def test_the_sweep_does_not_depend_on_the_chunk():
    prior = trials.centered_binomial(2)
    tb = trials.oracle_posterior_table(ref.SHARED_5, prior, 0.95)
    ts = trials.oracle_posterior_table(ref.expansion(13, 4), trials.centered_binomial(2, 3), 0.95, reverse=True)
    runs = 1001
    i = np.arange(runs)
    want = dict(runs=runs, successes=int((i % 4 == 0).sum()), channel_wrong=int((5 + i % 2).sum()), wrong=int((i % 4).sum()))
    hist = np.bincount(i % 4, minlength=9)

    def fake_class(name):
        assert name == "DecoderN13R5SW3"
        return FakeSpecial

    for chunk in (7, 64, 1000):
        FakeSpecial.calls = []
        got = driver.kyber_fer_sweep(toy_H(), "DecoderN13R5SW3", 3, prior, tb, ts, runs, 21, chunk=chunk, decoder_class=fake_class)
        assert np.array_equal(got.pop("wrong_hist"), hist) and FakeSpecial.last.closed
        assert got == want, chunk
        assert FakeSpecial.calls == [(f, min(chunk, runs - f)) for f in range(0, runs, chunk)]
    got = driver.kyber_fer_sweep(toy_H(), "DecoderN13R5SW3", 3, prior, tb, ts, 0, 21, decoder_class=fake_class)
    assert got["successes"] == 0 and got["wrong"] == 0 and not got["wrong_hist"].any()
    with pytest.raises(ValueError):
        driver.kyber_fer_sweep(toy_H(), "DecoderN13R5SW3", 3, prior, tb, ts, 10, 21, chunk=0, decoder_class=fake_class)
