"""The float64 Monte-Carlo sweeps (scaldpc_mc_fer_run_f64, scaldpc_mc_hqc_run_f64, scaldpc_mc_hqc_run_stats_f64), what can be held
without a GPU: the boundary and its device-free refusals, the `precision` keyword of the Python surface (and
`driver.sweeps_in` for the driver whose parameter list is pinned), the preconditions of
tests/test_ref64_mc_gpu.py derived again from the CPU oracle, the host header that builds the float64 law of an outcome table
(csrc/scaldpc_mc_law.h, driven by tests/mc_law64_main.cc under the address and undefined-behaviour sanitizers where the
toolchain has their runtimes), and the three drivers on a decoder double backed by the oracle."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import hqc_soft_mc_ref
import mc_ref
import ref64_mc_cases as cases
from ref64_mc_cases import MAX_ITER, RUNS, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
driver = importlib.import_module("sca-ldpc_amd.driver")
bp = importlib.import_module("sca-ldpc_amd.bp")
L = importlib.import_module("sca-ldpc_amd._lib")

CXX = os.environ.get("CXX", "g++")
ENTRIES = ("scaldpc_mc_fer_run_f64", "scaldpc_mc_hqc_run_f64", "scaldpc_mc_hqc_run_stats_f64")


# --------------------------------------------------------------------------------------------------------------- the boundary
def test_the_boundary_has_the_three_entry_points():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    assert "#define SCALDPC_VERSION 104" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    norm = lambda s: re.sub(r"\s+", " ", s).replace(" ,", ",").strip()  # noqa: E731
    args = {name: norm(re.search(rf"\bint {name}\(([^;]*)\);", code).group(1)) for name in ENTRIES}
    fp32 = {name: norm(re.search(rf"\bint {name[:-4]}\(([^;]*)\);", code).group(1)) for name in ENTRIES}
    # the fp32 entries' arguments without method and alpha; the table's probabilities are doubles
    for name in ENTRIES:
        want = fp32[name].replace(" int32_t method, float alpha,", "").replace("const float *probs", "const double *probs")
        assert args[name] == want, name
    # every comment that declares one carries the version line, and the defining properties are stated
    comment = [c for c in re.findall(r"/\*.*?\*/", src, flags=re.S) if "scaldpc_mc_hqc_run_stats_f64  scaldpc_mc_hqc_run_stats's trials" in c]
    assert len(comment) == 1
    for word in ("(entry points added under SCALDPC_VERSION 104: nothing that existed changed)", "Defining properties",
                 "precision is a property of the decode, not of the trial", "scaldpc_bp_last_compacted", "DOUBLE [K]"):
        assert word in comment[0], word
    assert src.index("scaldpc_mc_fer_run_f64 / scaldpc_mc_hqc_run_f64 / scaldpc_mc_hqc_run_stats_f64") < src.index("#ifndef SCALDPC_H")
    lib = L.load()
    assert lib.scaldpc_version() == 104
    vp = ctypes.c_void_p
    for name in ENTRIES:
        fn, old = getattr(lib, name), getattr(lib, name[:-4])
        assert fn.restype is ctypes.c_int
        drop = [i for i, t in enumerate(old.argtypes) if t is ctypes.c_float]  # alpha, and the method before it
        assert len(drop) == 1 and fn.argtypes == old.argtypes[: drop[0] - 1] + old.argtypes[drop[0] + 1 :], name
    assert lib.scaldpc_mc_hqc_run_stats_f64.argtypes[-2:] == [vp, vp]


def _call(name, **change):
    """An entry with no handle and every pointer NULL but out_success; integers 0 but batch = 1."""
    lib = L.load()
    fn = getattr(lib, name)
    keep = np.full(4, 0x5A, dtype=np.uint8)
    names = {"scaldpc_mc_fer_run_f64": ["h", "first", "batch", "seed", "max_iter", "flags", "stream", "success"],
             "scaldpc_mc_hqc_run_f64": ["h", "omega", "eps", "first", "batch", "seed", "max_iter", "flags", "stream", "success"],
             "scaldpc_mc_hqc_run_stats_f64": ["h", "omega", "weights", "flips", "probs", "costs", "K", "first", "batch", "seed", "max_iter",
                                              "flags", "stream", "success"]}[name]  # fmt: skip
    values = dict(dict(batch=1, success=L.ptr(keep)), **change)
    args = [values.get(n, None if t is ctypes.c_void_p else 0) for n, t in zip(names, fn.argtypes)]
    args += [None] * (len(fn.argtypes) - len(args))
    rc = fn(*args)
    assert (keep == 0x5A).all()
    return rc, lib.scaldpc_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_that_need_no_device(name):
    """Refused with nothing built: there is no handle at all, and each refusal still names its own reason."""
    for change, why in ((dict(first=-1), "first_trial"), (dict(batch=0), "batch"), (dict(batch=-3), "batch"),
                        (dict(flags=L.F_ASYNC), "flags"), (dict(flags=1 << 9), "flags"), (dict(success=None), "NULL"),
                        (dict(), "NULL")):  # (the last: everything in order but the handle)
        rc, msg = _call(name, **change)
        assert rc == L.EINVAL and why in msg, (change, msg)


# -------------------------------------------------------------------------------------------- the host header, under the sanitizers
@pytest.fixture(scope="module")
def law_program(tmp_path_factory):
    """tests/mc_law64_main.cc, built as tests/test_hqc_soft_mc.py builds its sibling: a stand-alone host program, no HIP in it."""
    exe = str(tmp_path_factory.mktemp("mc_law64") / "mc_law64_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "mc_law64_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: mc_law64_main is built without them")
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
            q = dict(kv.split("=") for kv in ln.split())
            res.append(dict(refused=0, K=int(q["K"]), flips=int(q["flips"]), t=[[int(x) for x in q[f"t{b}"].split(",")] for b in (0, 1)],
                            ratio=np.array([int(x, 16) for x in q["ratio"].split(",")], dtype=np.uint64).view(np.float64),
                            cost=[int(x) for x in q["cost"].split(",")], same32=int(q["same32"])))
        return res

    return run


def test_the_float64_law_of_the_table(law_program):
    """mc_hqc_law64: the ratios are p / (1 - p) of the probabilities AS THEY ARE, by the IEEE double division (p = 0 -> 0,
    p = 1 -> inf); thresholds, flips and costs are the fp32 entry's: the trial law does not know the precision."""
    t = cases.t9()
    p = cases.probs64()
    K = len(p)
    edge = [0.0, 1.0, 5e-324, 1.0 - 2.0**-53, 0.5, 2.0**-60]
    got = law_program([(K, 70, 1, t["weights"][0].tolist(), t["weights"][1].tolist(), t["flips"].tolist(), p.tolist(), t["costs"].tolist()),
                       (6, 45, 0, [1 / 6] * 6, [0.5, 0.5, 0, 0, 0, 0], [0, 1, 0, 1, 0, 1], edge, None),
                       (32, 4000, 0, [1 / 32] * 32, [1 / 32] * 32, [0] * 32, [k / 31 for k in range(32)], None)])
    with np.errstate(divide="ignore"):
        for r, probs in zip(got, (p, np.array(edge), np.arange(32) / 31)):
            assert r["refused"] == 0 and r["same32"] == 1 and r["K"] == len(probs)
            assert np.array_equal(r["ratio"].view(np.uint64), (probs / (1.0 - probs)).view(np.uint64))
    assert got[0]["cost"] == t["costs"].tolist() and got[0]["flips"] == int(sum(int(f) << k for k, f in enumerate(t["flips"])))
    assert got[1]["ratio"][0] == 0.0 and np.isinf(got[1]["ratio"][1]) and got[1]["ratio"][2] == 5e-324 and got[1]["ratio"][5] > 0.0
    # t9's float64 ratios are not those of its probabilities rounded to float32
    rounded = p.astype(np.float32).astype(np.float64)
    assert (got[0]["ratio"] != rounded / (1.0 - rounded)).sum() >= 3


def test_the_float64_law_refuses_what_the_fp32_law_refuses(law_program):
    """... and a probability that is one only after rounding to float32; nothing is read past K (the sanitizers' to report)."""
    good = ([0.5, 0.5], [0.25, 0.75], [1, 0])
    bad = {
        "no outcome": (0, 70, 0, [], [], [], [], None),
        "33 outcomes": (33, 70, 0, [1.0] + [0.0] * 32, [1.0] + [0.0] * 32, [0] * 33, [0.0] * 33, None),
        "a negative weight": (2, 70, 0, [-0.5, 1.5], good[1], good[2], [0.1, 0.2], None),
        "a NaN weight": (2, 70, 0, good[0], [float("nan"), 0.75], good[2], [0.1, 0.2], None),
        "row 1 does not sum to 1": (2, 70, 0, good[0], [0.25, 0.75 - 1e-5], good[2], [0.1, 0.2], None),
        "a negative probability": (2, 70, 0, *good, [-0.1, 0.2], None),
        "a probability above 1": (2, 70, 0, *good, [0.1, 1.5], None),
        "a probability that only rounds to 1": (2, 70, 0, *good, [0.1, 1.0 + 1e-12], None),
        "a probability that only rounds to 0": (2, 70, 0, *good, [-1e-300, 0.2], None),
        "a NaN probability": (2, 70, 0, *good, [float("nan"), 0.2], None),
        "a flip of 2": (2, 70, 0, good[0], good[1], [2, 0], [0.1, 0.2], None),
        "a negative cost": (2, 70, 0, *good, [0.1, 0.2], [2, -1]),
        "a cost above 65535": (2, 70, 0, *good, [0.1, 0.2], [65536, 1]),
        "out_cost without costs": (2, 70, 1, *good, [0.1, 0.2], None),
        "a trial's cost past int32": (2, 40000, 0, *good, [0.1, 0.2], [65535, 1]),
    }
    for name, r in zip(bad, law_program(list(bad.values()))):
        assert r["refused"] == 1 and r["why"], name
    ok = law_program([(2, 70, 1, *good, [0.1, 0.2], [2, 1])])[0]
    assert ok["refused"] == 0 and ok["cost"] == [2, 1] and ok["flips"] == 1 and ok["t"] == [[2**31, 2**32], [2**30, 2**32]]


def test_the_program_takes_only_the_law_header():
    src = open(os.path.join(ROOT, "tests", "mc_law64_main.cc")).read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include \"")] == ['"../sca-ldpc_amd/csrc/scaldpc_mc_law.h"']


# ---------------------------------------------------------------------------------------------------------------- the keywords
def test_the_keyword_is_bound():
    for f in (bp.BpDecoder.mc_fer_run, bp.BpDecoder.mc_hqc_run, bp.BpDecoder.mc_hqc_run_soft):
        p = inspect.signature(f).parameters["precision"]
        assert p.default == "float32" and "WHATEVER the decoder's own" in f.__doc__  # the default is fp32, and says so
    assert inspect.signature(driver.hqc_oracle_sweep).parameters["precision"].default is None
    # the curve's own parameter list is pinned (tests/test_hqc_stats.py) and stays: its float64 form comes with the decoder class
    assert "precision" not in inspect.signature(driver.hqc_attack_curve).parameters
    assert list(inspect.signature(driver.sweeps_in).parameters) == ["precision", "bp_decoder"]
    for bad in ("float16", None, 64):
        with pytest.raises(ValueError, match="is invalid"):
            driver.sweeps_in(bad, bp_decoder=_NoLibrary)
    cls = driver.sweeps_in("float64", bp_decoder=bp.BpDecoder)
    assert issubclass(cls, bp.BpDecoder) and cls.decode_batch is bp.BpDecoder.decode_batch and "Float64" in cls.__name__

    class Recorder:
        def mc_fer_run(self, *a, **kw):
            return ("fer", a, kw)

        def mc_hqc_run(self, *a, **kw):
            return ("hqc", a, kw)

        def mc_hqc_run_soft(self, *a, **kw):
            return ("soft", a, kw)

    d = driver.sweeps_in("float64", bp_decoder=Recorder)()
    assert d.mc_fer_run(4, 1) == ("fer", (4, 1), {"precision": "float64"})
    assert d.mc_hqc_run(4, 2, 0.1, seed=1) == ("hqc", (4, 2, 0.1), {"precision": "float64", "seed": 1})
    assert d.mc_hqc_run_soft(4, 2, None, 1, want_stats=True) == ("soft", (4, 2, None, 1), {"precision": "float64", "want_stats": True})
    assert d.mc_fer_run(4, 1, precision="float32")[2] == {"precision": "float32"}  # a call's own keyword wins
    assert list(inspect.signature(driver.hqc_precision_audit).parameters) == [
        "Hin", "N", "omega", "table", "runs", "seed", "chunk", "max_iter", "bp_decoder"]  # fmt: skip
    p = inspect.signature(driver.hqc_precision_audit).parameters
    assert p["chunk"].default == 4096 and p["max_iter"].default == 100 and p["bp_decoder"].default is None


class _NoLibrary:
    """A min-sum (or product-sum) decoder as far as the keyword looks: any library call is an AttributeError."""

    def __init__(self, method):
        self._method, self.max_iter, self.n, self.m = method, 5, 8, 3
        self.ms_scaling_factor = 1.0


@pytest.mark.parametrize("call", [lambda d, p: bp.BpDecoder.mc_fer_run(d, 4, 1, precision=p),
                                  lambda d, p: bp.BpDecoder.mc_hqc_run(d, 4, 2, 0.1, 1, precision=p),
                                  lambda d, p: bp.BpDecoder.mc_hqc_run(d, 4, 2, 0.1, 1, want_stats=True, precision=p),
                                  lambda d, p: bp.BpDecoder.mc_hqc_run_soft(d, 4, 2, hqc_soft_mc_ref.eps_table(0.1), 1, precision=p)])
def test_float64_on_a_min_sum_decoder_and_an_invalid_value_raise_before_any_library_call(call):
    with pytest.raises(ValueError, match="no min-sum form"):
        call(_NoLibrary(L.BP_MIN_SUM), "float64")
    for method in (L.BP_MIN_SUM, L.BP_PRODUCT_SUM):
        with pytest.raises(ValueError, match="is invalid"):
            call(_NoLibrary(method), "float16")
    with pytest.raises(AttributeError):  # a valid value reaches the library
        call(_NoLibrary(L.BP_PRODUCT_SUM), "float64")


# ------------------------------------------------------------------------------------------ the preconditions of the GPU tests
@pytest.mark.parametrize("name, soft", sorted(cases.PRECONDITIONS))
def test_the_preconditions_are_the_oracles(name, soft):
    """(converged, success, running after 2, running after 4) of the float64 oracle with early exit.  A hand-over at 2 fills one to
    two compact tiles with a ragged last one; at 4 one tile, or two with a tail of 5."""
    d = cases.soft_oracle(name) if soft else cases.shared_oracle(name)
    got = (int(d["converged"].sum()), int(d["success"].sum()), cases.running_after(d, 2), cases.running_after(d, 4))
    print(name, "t9" if soft else "shared priors", got)
    assert got == cases.PRECONDITIONS[(name, soft)]
    assert 0 < got[3] < got[2] < RUNS and got[2] % 64 != 0 and got[3] % 64 != 0
    assert 0 < got[1] < RUNS and MAX_ITER > 4
    fixed = cases.soft_oracle(name, False) if soft else cases.shared_oracle(name, False)
    assert (fixed["iters"] == MAX_ITER).all() and (d["iters"] < MAX_ITER).any()  # the two modes differ in what they report


def test_the_ragged_tiles_are_among_them():
    assert cases.handed_over("H2", False, 4) == 64 + 5 and cases.handed_over("H1", True, 4) == 3
    assert [cases.handed_over(n, False, 2) for n in cases.SHARED] == [65, 113, 119]
    assert [cases.handed_over(n, False, 4) for n in cases.SHARED] == [24, 47, 69]
    assert [cases.handed_over(n, True, k) for k in (2, 4) for n in cases.SOFT] == [23, 60, 3, 14]
    assert cases.handed_over("F", False, 0) == cases.handed_over("F", False, 40) == 0


def test_t9_is_not_a_float32_table():
    t = cases.t9()
    p = cases.probs64()
    assert t["weights"].shape == (2, 9) and p.dtype == np.float64
    for v in (0.0004, 0.01, 0.001):
        assert np.isclose(p, v, rtol=1e-12).any() and float(np.float32(v)) != v
    assert (p.astype(np.float32).astype(np.float64) != p).sum() >= 3
    law = cases.soft_law("H2")
    assert len(np.unique(law["outcome"])) >= 4 and law["probs64"].shape == (RUNS, 70)


@pytest.mark.parametrize("name", cases.SHARED)
def test_both_precisions_agree_on_the_shared_instances(name):
    """On F / H1 / H2 the f32 oracle in the fp32 kernels' order and the float64 oracle agree on all 130 successes and iteration
    counts: the audit's expected answer there is 0."""
    a, b = mc_ref.oracle_decode(name, "product_sum"), cases.shared_oracle(name)
    assert np.array_equal(a["success"], b["success"]) and np.array_equal(a["iters"], b["iters"])


# ----------------------------------------------------------------------------------------- the drivers on an oracle-backed double
class OracleSoftBp:
    """A decoder double in the style of tests/fakes.OracleBp with the surface the three drivers use: a graph [Hin | I] that grows
    by `append_rows`, and `mc_hqc_run_soft(precision=)` answered by the NumPy law and the CPU oracle per codeword -- float64 in
    the reference's own arithmetic on the table's probabilities as they are, float32 in the fp32 kernels' order on the rounded
    ones.  The double's trial i is the law's trial FIRST + i."""

    log = []

    def __init__(self, H, max_iter, bp_method, channel_probs):
        assert bp_method == "product_sum" and len(channel_probs) == H.n
        self.m, self.n, self.max_iter = H.m, H.n, max_iter
        self.row_ptr, self.col_idx = np.asarray(H.row_ptr).copy(), np.asarray(H.col_idx).copy()
        self.closed = False
        OracleSoftBp.last = self

    def append_rows(self, row_ptr, col_idx, new_n, channel_probs_tail):
        assert row_ptr[0] == 0 and len(col_idx) == row_ptr[-1] and len(channel_probs_tail) == new_n - self.n == len(row_ptr) - 1
        self.row_ptr = np.concatenate([self.row_ptr, self.row_ptr[-1] + np.asarray(row_ptr[1:])])
        self.col_idx = np.concatenate([self.col_idx, col_idx])
        self.m += len(row_ptr) - 1
        self.n = new_n

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, max_iter=None, want_stats=False, precision="float32"):
        assert not self.closed and precision in ("float32", "float64") and seed == SEED and table is cases.t9()
        OracleSoftBp.log.append((self.m, first_trial, runs, precision))
        N = self.n - self.m
        H, Hin = cases.h2_cut(self.m)  # the graph the driver built must be H2 cut to its first m rows
        assert self.n == H.n and np.array_equal(self.row_ptr, H.row_ptr) and np.array_equal(self.col_idx, H.col_idx)
        assert max_iter == MAX_ITER
        d = cases.h2_cut_oracle(self.m, "f64" if precision == "float64" else "f32")
        law = cases.h2_cut_law(self.m)
        sl = slice(first_trial, first_trial + runs)
        res = {"success": d["success"][sl], "iters": d["iters"][sl].astype(np.int32), "flips": law["flips"][sl].astype(np.int32),
               "cost": law["cost"][sl].astype(np.int32), "msg": None, "y": None, "outcome": None}
        return dict(res, stats=d["stats"][sl], bits=None) if want_stats else res

    def close(self):
        self.closed = True


CHUNKS = (64, 100, 4096)


def _sweep(precision, chunk, **kw):
    i = mc_ref.instance("H2")
    OracleSoftBp.log = []
    got = driver.hqc_oracle_sweep(i["Hin"], i["N"], i["omega"], cases.t9(), RUNS, SEED, chunk=chunk, max_iter=MAX_ITER,
                                  bp_decoder=OracleSoftBp, precision=precision, **kw)
    assert OracleSoftBp.last.closed
    return got


def test_the_sweep_hands_the_keyword_through():
    key = cases.h2_cut_oracle(70)
    assert np.array_equal(key["success"], cases.soft_oracle("H2")["success"])  # (the cut at 70 rows is H2)
    for chunk in CHUNKS:
        got = _sweep("float64", chunk, want_stats=True)
        assert OracleSoftBp.log == [(70, f, min(chunk, RUNS - f), "float64") for f in range(0, RUNS, chunk)]
        assert got["successes"] == int(key["success"].sum()) == 99
        assert np.array_equal(got["iter_hist"], np.bincount(key["iters"], minlength=MAX_ITER + 1))
        assert got["stats"] == dict(zip(driver.HQC_STATS_COLUMNS, key["stats"].astype(np.int64).sum(axis=0).tolist()))
    assert {p for *_, p in (_sweep("float32", 64), OracleSoftBp.log)[1]} == {"float32"}
    # None leaves the call as it is: the double is not given the keyword at all
    seen = {}

    class Plain(OracleSoftBp):
        def mc_hqc_run_soft(self, *a, **kw):
            seen.update(kw)
            return super().mc_hqc_run_soft(*a, **kw)

    i = mc_ref.instance("H2")
    driver.hqc_oracle_sweep(i["Hin"], i["N"], i["omega"], cases.t9(), RUNS, SEED, max_iter=MAX_ITER, bp_decoder=Plain)
    assert "precision" not in seen


def _curve(precision, chunk=4096):
    sup, rows = cases.h2_code()
    i = mc_ref.instance("H2")
    OracleSoftBp.log = []
    got = driver.hqc_attack_curve(sup, i["N"], rows, i["omega"], cases.t9(), RUNS, SEED, cases.CURVE_STEP, chunk=chunk, max_iter=MAX_ITER,
                                  bp_decoder=OracleSoftBp if precision is None else driver.sweeps_in(precision, bp_decoder=OracleSoftBp))
    assert OracleSoftBp.last.closed
    return got


@pytest.mark.parametrize("precision, dtype", [("float64", "f64"), ("float32", "f32"), (None, "f32")])
def test_the_attack_curve_follows_its_decoder_class(precision, dtype):
    """hqc_attack_curve(bp_decoder=sweeps_in(precision)): every sweep of the live decoder runs in that precision; the plain
    class is called as before."""
    need, successes = cases.curve_key(dtype)
    want = _curve(precision)
    assert {p for *_, p in OracleSoftBp.log} == {precision or "float32"}
    assert want["steps"].tolist() == list(cases.CURVE_STEPS) and np.array_equal(want["successes"], successes)
    assert np.array_equal(want["checks_needed"], need) and 0 < (need > 0).sum() < RUNS
    for chunk in CHUNKS[:2]:
        got = _curve(precision, chunk)
        assert OracleSoftBp.log == [(r, f, min(chunk, RUNS - f), precision or "float32") for r in cases.CURVE_STEPS
                                    for f in range(0, RUNS, chunk)]
        assert got["decoder_stats"] == want["decoder_stats"]
        for k in ("steps", "successes", "checks_needed", "oracle_calls_needed"):
            assert np.array_equal(got[k], want[k]), (chunk, k)


def test_the_audit_counts_the_differences():
    i = mc_ref.instance("H2")
    a, b = cases.h2_cut_oracle(70, "f32"), cases.h2_cut_oracle(70, "f64")
    want = None
    for chunk in CHUNKS:
        OracleSoftBp.log = []
        got = driver.hqc_precision_audit(i["Hin"], i["N"], i["omega"], cases.t9(), RUNS, SEED, chunk=chunk, max_iter=MAX_ITER,
                                         bp_decoder=OracleSoftBp)
        assert OracleSoftBp.last.closed
        assert OracleSoftBp.log == [(70, f, min(chunk, RUNS - f), p) for f in range(0, RUNS, chunk) for p in ("float32", "float64")]
        assert sorted(got) == sorted(["runs", "successes32", "successes64", "success_differs", "iters_differ", "iter_hist32", "iter_hist64"])
        assert got["runs"] == RUNS and got["successes32"] == int(a["success"].sum()) and got["successes64"] == int(b["success"].sum())
        assert np.array_equal(got["success_differs"], np.flatnonzero(a["success"] != b["success"]))
        assert got["iters_differ"] == int((a["iters"] != b["iters"]).sum())
        assert np.array_equal(got["iter_hist32"], np.bincount(a["iters"], minlength=MAX_ITER + 1))
        assert np.array_equal(got["iter_hist64"], np.bincount(b["iters"], minlength=MAX_ITER + 1))
        if want is not None:
            for k in got:
                assert np.array_equal(got[k], want[k]), (chunk, k)
        want = got
    empty = driver.hqc_precision_audit(i["Hin"], i["N"], i["omega"], cases.t9(), 0, SEED, bp_decoder=OracleSoftBp)
    assert empty["runs"] == 0 and empty["success_differs"].size == 0 and empty["iter_hist64"].sum() == 0
    with pytest.raises(ValueError):
        driver.hqc_precision_audit(i["Hin"], i["N"] + 1, i["omega"], cases.t9(), 4, SEED, bp_decoder=OracleSoftBp)
    with pytest.raises(ValueError):
        driver.hqc_precision_audit(i["Hin"], i["N"], i["omega"], cases.t9(), 4, SEED, chunk=0, bp_decoder=OracleSoftBp)
