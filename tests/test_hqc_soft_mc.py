"""HQC trials whose checks are answered by the attack's oracle on the device (scaldpc_mc_hqc_run_soft), what can be held without
a GPU: the boundary, `trials.wrapped_oracle_table` against a brute-force walk of the reference's loop, the trial law restated
in NumPy against the Bernoulli draw of oracle/mc_oracle.c, the host header that validates the tables and builds the law
(csrc/scaldpc_mc_law.h, driven by tests/mc_law_main.cc under the address and undefined-behaviour sanitizers where the toolchain
has their runtimes), and driver.hqc_oracle_sweep on a decoder double."""
import ctypes
import importlib
import math
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import hqc_soft_mc_ref as ref
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
trials = importlib.import_module("sca-ldpc_amd.trials")
driver = importlib.import_module("sca-ldpc_amd.driver")
bp = importlib.import_module("sca-ldpc_amd.bp")
L = importlib.import_module("sca-ldpc_amd._lib")
S = importlib.import_module("sca-ldpc_amd")


def test_the_boundary_has_the_entry_point():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    assert "#define SCALDPC_VERSION 104" in src
    decl = re.search(r"\bint scaldpc_mc_hqc_run_soft\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert decl and len(decl.group(1).split(",")) == 22
    for word in ("r >> 2", "word r & 3", "smallest k with word < T^b_k", "never drawn", "Reductions", "Defining property"):
        assert word in src, word  # the trial law is written down next to K6's
    lib = L.load()
    fn = lib.scaldpc_mc_hqc_run_soft
    assert len(fn.argtypes) == 22 and fn.restype is not None
    # refused before anything touches a device: no handle
    assert fn(*[None if t is ctypes.c_void_p else 0 for t in fn.argtypes]) == L.EINVAL
    assert callable(bp.BpDecoder.mc_hqc_run_soft)


# ------------------------------------------------------------------------------------------------------ the wrapped oracle's table
def walk_the_wrapped_oracle(accuracy, require, b):
    """simulate/hqc.py:782-871 for a check whose true value is b, every path of the loop with its probability: a try answers
    right with probability accuracy[b] (hqc.py:830-831,864) and its certainty accuracy[b] joins the list of the answer it gave
    (hqc.py:798); that answer's certainty is 1.0 - prod(1.0 - p for p in its list) (hqc.py:800), and the loop returns it once the
    certainty reaches require[answer] (hqc.py:801-806).  Returns {(answer, tries): [probability, certainty]}."""
    a = accuracy[b]
    done = {}

    def step(lists, tries, prob):
        assert tries < 64
        for answer in (0, 1):
            p = a if answer == b else 1.0 - a
            if p == 0.0:
                continue
            grown = (lists[0] + [a], lists[1]) if answer == 0 else (lists[0], lists[1] + [a])
            certainty = 1.0 - math.prod([1.0 - q for q in grown[answer]])
            if certainty >= require[answer]:
                slot = done.setdefault((answer, tries + 1), [0.0, certainty])
                slot[0] += prob * p
                assert slot[1] == certainty
            else:
                step(grown, tries + 1, prob * p)

    step(([], []), 0, 1.0)
    return done


@pytest.mark.parametrize("accuracy, require", [((0.98, 0.9), (0.999, 0.99)), ((0.9, 0.8), (0.95, 0.9)), ((1.0, 0.75), (0.5, 0.99)),
                                               ((0.7, 0.95), (0.9, 0.999))])
def test_wrapped_oracle_table_is_the_reference_loop(accuracy, require):
    t = trials.wrapped_oracle_table(accuracy=accuracy, require=require)
    K = len(t["flips"])
    assert t["weights"].shape == (2, K) and t["probs"].shape == (K,) and t["costs"].shape == (K,) and K <= 32
    assert np.abs(t["weights"].sum(axis=1) - 1.0).max() <= 1e-12
    seen = 0
    for b in (0, 1):
        want = walk_the_wrapped_oracle(accuracy, require, b)
        mine = np.flatnonzero(t["weights"][b] > 0)
        assert (t["weights"][1 - b][mine] == 0).all()  # an outcome belongs to one true value
        got = {(b ^ int(t["flips"][k]), int(t["costs"][k])): k for k in mine}
        assert len(got) == len(mine) and set(got) == set(want)
        for key, (prob, certainty) in want.items():
            k = got[key]
            assert abs(t["weights"][b, k] - prob) <= 1e-12 and abs(t["probs"][k] - (1.0 - certainty)) <= 1e-12
        seen += len(mine)
    assert seen == K
    if (accuracy, require) == ((0.98, 0.9), (0.999, 0.99)):
        assert K == 9


def test_wrapped_oracle_table_refuses_what_does_not_fit():
    with pytest.raises(ValueError):
        trials.wrapped_oracle_table((0.6, 0.6), (0.999999, 0.999999))  # 16 + 16 tries per true value: 64 outcomes
    with pytest.raises(ValueError):
        trials.wrapped_oracle_table((0.5, 0.9), (1.5, 0.9))
    with pytest.raises(ValueError):
        trials.wrapped_oracle_table((0.0, 0.9), (0.9, 0.9))  # certainty 0 per try: the loop never ends


def test_levels_table_is_the_law_of_hqc_soft_trials():
    t = trials.levels_table((1.0, 0.9, 0.7), (0.2, 0.4, 0.4))
    assert np.array_equal(t["weights"][0], t["weights"][1]) and t["costs"] is None
    assert np.allclose(t["weights"][0], [0.0, 0.2, 0.04, 0.36, 0.12, 0.28], rtol=0, atol=1e-15)
    assert t["flips"].tolist() == [1, 0, 1, 0, 1, 0]
    assert np.array_equal(t["probs"].astype(np.float32), (1.0 - np.repeat([1.0, 0.9, 0.7], 2)).astype(np.float32))
    with pytest.raises(ValueError):
        trials.levels_table((0.9, 1.1), (0.5, 0.5))


# ----------------------------------------------------------------------------------------------------------------- the trial law
@pytest.mark.parametrize("eps", [0.0, 1.0, 0.04, 0.5, 1e-12])
def test_the_two_outcome_table_is_the_bernoulli_draw_of_the_oracle(eps):
    """The reduction to scaldpc_mc_hqc_run: K = 2, both rows (eps, 1 - eps), flips (1, 0) -- outcome 0 sits exactly where
    oracle.mc_bernoulli flips, whatever the true bits."""
    seed, first, batch, R = 0x1234567890ABCDEF, (1 << 32) - 3, 7, 30
    t = ref.eps_table(eps)
    c = np.random.RandomState(3).randint(0, 2, size=(batch, R))
    out = ref.outcomes_of(ref.words(seed, first, batch, R), c, t["weights"])
    assert np.array_equal(t["flips"][out], pyoracle.mc_bernoulli(seed, first, batch, R, None, eps))


def test_an_outcome_of_weight_zero_is_never_drawn():
    """In the middle of a table and at its end, over 10^5 words (the two ends of the word range among them), per true bit."""
    w = np.concatenate([ref.words(9, 0, 25, 4000).reshape(-1), np.array([0, (1 << 32) - 1], dtype=np.uint64)])
    assert w.size >= 10**5
    weights = np.array([[0.5, 0.0, 0.25, 0.25 - 1e-7, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0]])
    for b, drawn in ((0, {0, 2, 3}), (1, {2})):
        out = ref.outcomes_of(w, np.full(w.size, b), weights)
        assert set(np.unique(out)) == drawn
    assert ref.outcomes_of(w[-1:], [0], weights)[0] == 3  # a sum that rounds below 1: the last outcome of weight > 0 takes the rest


def test_the_law_in_numpy_on_a_small_instance():
    """`draw` is what the GPU tests hold the device to: here its own consistency -- the secret's weight, the flips it counts,
    the costs it adds, and the table's frequencies on 260 x 40 checks."""
    from helpers import hqc_instance

    _, Hin, _, _, _ = hqc_instance(499, 7, 260, 5, 0.04, 1, seed=11, flip=False)
    t = trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))
    d = ref.draw(42, 1000, 40, Hin, 5, t)
    yv = np.zeros((40, 499), dtype=np.uint8)
    np.put_along_axis(yv, d["y"].astype(np.int64), 1, axis=1)
    c = Hin.syndrome(yv)
    assert (yv.sum(axis=1) == 5).all() and np.array_equal(d["msg"][:, 499:] ^ c, t["flips"][d["outcome"]])
    assert np.array_equal(d["flips"], (d["msg"][:, 499:] != c).sum(axis=1)) and not d["msg"][:, :499].any()
    assert np.array_equal(d["cost"], t["costs"][d["outcome"]].sum(axis=1)) and (d["cost"] >= 2 * 260).all()
    for b in (0, 1):  # an outcome is drawn under its own true bit only, the likeliest one most often
        drawn = d["outcome"][c == b]
        assert (t["weights"][b][np.unique(drawn)] > 0).all() and np.bincount(drawn).argmax() == t["weights"][b].argmax()
    assert np.array_equal(d["probs"], t["probs"].astype(np.float32)[d["outcome"]])


# -------------------------------------------------------------------------------------------- the host header, under the sanitizers
@pytest.fixture(scope="module")
def law_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mc_law") / "mc_law_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "mc_law_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: mc_law_main is built without them")
        subprocess.check_call(cmd)

    def run(tables):
        """tables: [(K, R, want_cost, w0, w1, flips, probs, costs or None)] -> one parsed line each, out of ONE process."""
        text = ""
        for K, R, want_cost, w0, w1, flips, probs, costs in tables:
            nums = [K, R, int(want_cost), int(costs is not None)] + list(w0) + list(w1) + list(flips) + list(probs) + list(costs or [])
            text += " ".join(repr(float(x)) if isinstance(x, float) else str(x) for x in nums) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        lines = out.stdout.splitlines()
        assert len(lines) == len(tables)
        res = []
        for ln in lines:
            if ln.startswith("refused=1"):
                res.append(dict(refused=1, why=ln[len("refused=1 "):]))
                continue
            p = dict(kv.split("=") for kv in ln.split())
            res.append(dict(refused=0, K=int(p["K"]), flips=int(p["flips"]), t=[[int(x) for x in p[f"t{b}"].split(",")] for b in (0, 1)],
                            llr=np.array([int(x, 16) for x in p["llr"].split(",")], dtype=np.uint32).view(np.float32),
                            cost=[int(x) for x in p["cost"].split(",")]))
        return res

    return run


def host_llr(probs):
    """logf((1.0f - p) / p) with the host's libm, float32 throughout: what prior_llrs computes for the decoder's own priors."""
    libm = ctypes.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    p = np.asarray(probs, dtype=np.float32)
    with np.errstate(divide="ignore"):
        x = (np.float32(1.0) - p) / p
    return np.array([libm.logf(float(v)) for v in x], dtype=np.float32)


def test_the_program_takes_only_the_law_header():
    src = open(os.path.join(ROOT, "tests", "mc_law_main.cc")).read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include \"")] == ['"../sca-ldpc_amd/csrc/scaldpc_mc_law.h"']
    hdr = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_mc_law.h")).read()
    assert not [ln for ln in hdr.splitlines() if ln.startswith("#include") and "hip" in ln.lower()]
    for unit in ("scaldpc_bp.hip", "scaldpc_qary.hip"):  # one rule for both entries, and for mc_fer_run's thresholds
        text = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", unit)).read()
        assert '#include "scaldpc_mc_law.h"' in text and "4294967296.0" not in text


def test_the_law_the_host_builds(law_program):
    t9 = trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))
    lv = trials.levels_table((1.0, 0.9, 0.7), (0.2, 0.4, 0.4))
    k32 = np.zeros(32)
    k32[[0, 5, 17, 29]] = [0.25, 0.5, 0.125, 0.125]  # weight 0 in the middle and at the end (outcomes 30 and 31)
    one = np.zeros(32)
    one[31] = 1.0
    p32 = np.linspace(0.0, 0.5, 32)
    tables = [
        (9, 260, True, t9["weights"][0], t9["weights"][1], t9["flips"], t9["probs"], t9["costs"].tolist()),
        (6, 4000, False, lv["weights"][0], lv["weights"][1], lv["flips"], lv["probs"], None),
        (1, 260, False, [1.0], [1.0], [0], [0.0], None),  # K = 1, p = 0: LLR +inf
        (1, 260, True, [1.0], [1.0], [1], [1.0], [65535]),  # p = 1: LLR -inf; the largest cost
        (2, 10, False, [0.04, 0.96], [0.04, 0.96], [1, 0], [0.04, 0.04], None),
        (32, 77, True, k32, one, [k & 1 for k in range(32)], p32, list(range(32))),  # K = 32
        (3, 5, False, [0.1, 0.2, 0.7], [0.5, 0.5 - 1e-7, 0.0], [0, 1, 0], [0.5, 0.25, 0.125], None),
    ]
    res = law_program(tables)
    for (K, R, _, w0, w1, flips, probs, costs), got in zip(tables, res):
        assert got["refused"] == 0 and got["K"] == K
        assert got["t"] == [ref.thresholds(w0), ref.thresholds(w1)]
        assert got["flips"] == sum(int(f) << k for k, f in enumerate(flips))
        assert np.array_equal(got["llr"].view(np.uint32), host_llr(probs).view(np.uint32))
        assert got["cost"] == (list(costs) if costs is not None else [0] * K)
    # threshold forcing: 2^32 from the last outcome of nonzero weight on, equal neighbours where a weight is 0
    assert res[5]["t"][0][29:] == [1 << 32] * 3 and res[5]["t"][0][28] < 1 << 32 and res[5]["t"][0][1] == res[5]["t"][0][0]
    assert res[5]["t"][1][:31] == [0] * 31 and res[5]["t"][1][31] == 1 << 32
    assert res[6]["t"][1] == [1 << 31, 1 << 32, 1 << 32]  # a sum that rounds below 1
    assert res[6]["t"][0][1] == int((np.float64(0.1) + np.float64(0.2)) * 4294967296.0)  # left to right in float64
    assert res[2]["llr"][0] == np.inf and res[3]["llr"][0] == -np.inf and res[4]["t"][0][0] == int(0.04 * 4294967296.0)


REFUSALS = {  # name -> (K, R, want_cost, w0, w1, flips, probs, costs), a word of the reason
    "no outcome": ((0, 10, False, [], [], [], [], None), "outcomes"),
    "33 outcomes": ((33, 10, False, [1.0] + [0.0] * 32, [1.0] + [0.0] * 32, [0] * 33, [0.1] * 33, None), "outcomes"),
    "a negative weight": ((2, 10, False, [-0.1, 1.1], [0.5, 0.5], [1, 0], [0.1, 0.1], None), "weights[0]"),
    "a weight above 1": ((2, 10, False, [0.5, 0.5], [1.5, 0.0], [1, 0], [0.1, 0.1], None), "weights[1]"),
    "a NaN weight": ((2, 10, False, [0.5, 0.5], [float("nan"), 0.5], [1, 0], [0.1, 0.1], None), "weights[1]"),
    "an infinite weight": ((2, 10, False, [float("inf"), 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], None), "weights[0]"),
    "row 0 does not sum to 1": ((2, 10, False, [0.5, 0.5 - 1e-5], [0.5, 0.5], [1, 0], [0.1, 0.1], None), "sum"),
    "row 1 does not sum to 1": ((2, 10, False, [0.5, 0.5], [0.5, 0.5 + 1e-5], [1, 0], [0.1, 0.1], None), "sum"),
    "a flip of 2": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [2, 0], [0.1, 0.1], None), "flips[0]"),
    "a negative probability": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, -0.1], None), "probs[1]"),
    "a probability above 1": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [1.5, 0.1], None), "probs[0]"),
    "a NaN probability": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [float("nan"), 0.1], None), "probs[0]"),
    "a negative cost": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], [1, -1]), "costs[1]"),
    "a cost above 65535": ((2, 10, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], [65536, 1]), "costs[0]"),
    "a trial's cost past int32": ((2, 32769, False, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], [65535, 1]), "int32"),
    "out_cost without costs": ((2, 10, True, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], None), "out_cost"),
}


def test_every_refusal(law_program):
    names = list(REFUSALS)
    res = law_program([REFUSALS[n][0] for n in names])
    for n, got in zip(names, res):
        assert got["refused"] == 1 and REFUSALS[n][1] in got["why"], (n, got)
    # ... and their neighbours that are taken: sums within 1e-6, the largest trial cost that fits
    ok = law_program([(2, 10, False, [0.5, 0.5 - 5e-7], [0.5, 0.5 + 5e-7], [1, 0], [0.0, 1.0], None),
                      (2, 32768, True, [0.5, 0.5], [0.5, 0.5], [1, 0], [0.1, 0.1], [65535, 0])])
    assert [g["refused"] for g in ok] == [0, 0]


# ------------------------------------------------------------------------------------------------------------------- the sweep
class FakeBp:
    """A decoder double with `mc_hqc_run_soft`'s surface: trial i succeeds unless i % 5 == 0, takes 1 + i % 7 iterations,
    reports i % 3 wrong checks and spends 1000 + i oracle calls."""

    calls = []

    def __init__(self, H, max_iter, bp_method, channel_probs):
        assert H.n == 30 + 12 and len(channel_probs) == H.n and max_iter == 9 and bp_method == "min_sum"
        assert np.allclose(channel_probs[:30], 4 / 30)
        self.closed = False
        FakeBp.last = self

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, max_iter=None, early_exit=True, want_inputs=False):
        assert omega == 4 and seed == 77 and max_iter == 9 and early_exit and not want_inputs
        FakeBp.calls.append((first_trial, runs))
        i = first_trial + np.arange(runs)
        cost = (1000 + i).astype(np.int32) if table.get("costs") is not None else None
        return {"success": (i % 5 != 0).astype(np.uint8), "iters": (1 + i % 7).astype(np.int32), "flips": (i % 3).astype(np.int32),
                "cost": cost, "msg": None, "y": None, "outcome": None}

    def close(self):
        self.closed = True


def test_the_sweep_does_not_depend_on_the_chunk():
    Hin = S.TannerGraph.from_dense((np.random.RandomState(1).rand(12, 30) < 0.2).astype(np.int8))
    t = trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))
    runs = 230
    i = np.arange(runs)
    ok = i % 5 != 0
    want = dict(runs=runs, successes=int(ok.sum()), flips=int((i % 3).sum()), oracle_calls=int((1000 + i).sum()),
                oracle_calls_mean=float((1000 + i).mean()), oracle_calls_success=int((1000 + i)[ok].sum()),
                oracle_calls_success_mean=float((1000 + i)[ok].mean()))
    hist = np.bincount(1 + i % 7, minlength=10)
    for chunk in (64, 100, 230, 4096):
        FakeBp.calls = []
        got = driver.hqc_oracle_sweep(Hin, 30, 4, t, runs, 77, chunk=chunk, bp_method="min_sum", max_iter=9, bp_decoder=FakeBp)
        assert np.array_equal(got.pop("iter_hist"), hist) and FakeBp.last.closed
        assert got.keys() == want.keys() and all(got[k] == pytest.approx(want[k], rel=1e-15) for k in want), chunk
        assert FakeBp.calls == [(f, min(chunk, runs - f)) for f in range(0, runs, chunk)]
    got = driver.hqc_oracle_sweep(Hin, 30, 4, dict(t, costs=None), runs, 77, bp_method="min_sum", max_iter=9, bp_decoder=FakeBp)
    assert got["oracle_calls"] is None and got["oracle_calls_success_mean"] is None and got["successes"] == want["successes"]
    got = driver.hqc_oracle_sweep(Hin, 30, 4, t, 0, 77, bp_method="min_sum", max_iter=9, bp_decoder=FakeBp)
    assert got["successes"] == 0 and got["oracle_calls"] == 0 and got["oracle_calls_mean"] is None and not got["iter_hist"].any()
    with pytest.raises(ValueError):
        driver.hqc_oracle_sweep(Hin, 31, 4, t, 5, 77, bp_decoder=FakeBp)
