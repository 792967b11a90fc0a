"""The float64 Monte-Carlo sweeps on the GPU (scaldpc_mc_fer_run_f64, scaldpc_mc_hqc_run_f64, scaldpc_mc_hqc_run_stats_f64): the
three sweep families decoded by scaldpc_bp_decode_batch_f64's recursion on trials drawn on the device, stragglers re-decoded in
dense tiles.

Held to (1) the float64 CPU oracle on all 130 trials of F / H1 / H2 (tests/ref64_mc_cases.py; tests/test_ref64_mc.py pins what
makes the instances hard enough); (2) the fp32 entries' trials and the NumPy laws, bit for bit; (3) the defining property:
decode_batch(precision="float64") on the exported inputs of the same handle; (4) the hand-over: invisible and counted.
Every test goes through a new entry point or keyword, so every one fails on a library without them."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hqc_soft_mc_ref
import mc_ref
import ref64_cases
import ref64_mc_cases as cases
from helpers import S
from ref64_mc_cases import FIRST, MAX_ITER, RUNS, SEED

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
driver = importlib.import_module("sca-ldpc_amd.driver")
lib = importlib.import_module("sca-ldpc_amd._lib")

INPUTS = ("errors", "msg", "y", "outcome", "flips", "cost")  # what a trial is, whatever decodes it
SOFT_OUT = ("success", "iters", "msg", "y", "outcome", "flips", "cost")  # the soft entry's outputs, in the order of the C ABI


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER", "SCALDPC_PRECISION"):
        monkeypatch.delenv(v, raising=False)


def _decoder(name, method="product_sum", H=None, probs=None, max_iter=MAX_ITER, **knobs):
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(i["H"] if H is None else H, max_iter=max_iter, bp_method=method, channel_probs=i["probs"] if probs is None else probs)
    if knobs:
        dec.configure(**knobs)
    return dec


def _sweep(dec, name, soft=False, runs=RUNS, first=FIRST, seed=SEED, precision="float64", early=True, **kw):
    """The sweep of the instance: F through mc_fer_run, H1 / H2 through mc_hqc_run, or under t9 through mc_hqc_run_soft."""
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):
        if soft:
            kw = dict(dict(want_inputs=True, want_stats=True, want_bits=True), **kw)
            return dec.mc_hqc_run_soft(runs, i["omega"], cases.t9(), seed, first_trial=first, early_exit=early, precision=precision, **kw)
        if name == "F":
            return dec.mc_fer_run(runs, seed, first_trial=first, early_exit=early, want_errors=True, precision=precision, **kw)
        kw = dict(dict(want_inputs=True), **kw)
        return dec.mc_hqc_run(runs, i["omega"], i["eps"], seed, first_trial=first, early_exit=early, precision=precision, **kw)


def _same(a, b, keys=None):
    for k in keys or a.keys() | b.keys():
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


CASES = [(n, False) for n in cases.SHARED] + [(n, True) for n in cases.SOFT]
IDS = [f"{n}{'-t9' if s else ''}" for n, s in CASES]


# ------------------------------------------------------------------------------------------------ 1. against the oracle, all 130
@pytest.mark.parametrize("early", [True, False], ids=["early", "fixed"])
@pytest.mark.parametrize("name, soft", CASES, ids=IDS)
def test_against_the_oracle(name, soft, early):
    """Iterations, success (and under t9 bits and the five counters) of all 130 trials are the float64 CPU recursion's."""
    ref = cases.soft_oracle(name, early) if soft else cases.shared_oracle(name, early)
    dec = _decoder(name)
    got = _sweep(dec, name, soft, early=early)
    assert got["iters"].dtype == np.int32 and got["success"].dtype == np.uint8
    assert np.array_equal(got["iters"], ref["iters"]), "iteration counts"
    assert np.array_equal(got["success"], ref["success"]), "success"
    if soft:
        assert np.array_equal(got["bits"], ref["bits"]), "bits"
        ok, stats = cases.count(mc_ref.instance(name)["N"], got["bits"], got["msg"], got["y"])
        assert got["stats"].dtype == np.int32 and np.array_equal(got["stats"], stats) and np.array_equal(got["success"], ok)
        assert np.array_equal(got["stats"], ref["stats"])
    if early:
        assert int(got["success"].sum()) == cases.PRECONDITIONS[(name, soft)][1]
    else:
        assert (got["iters"] == MAX_ITER).all() and dec.last_compacted() == 0
    dec.close()


# ---------------------------------------------------------------------------------------------- 2. trials are precision-blind
@pytest.mark.parametrize("name, soft", CASES, ids=IDS)
def test_trials_are_precision_blind(name, soft):
    """Every exported input of the float64 call equals the fp32 call's and the NumPy law's, bit for bit."""
    dec = _decoder(name)
    a, b = _sweep(dec, name, soft, precision="float32"), _sweep(dec, name, soft, precision="float64")
    law = cases.soft_law(name) if soft else cases.shared_law(name)
    seen = 0
    for k in INPUTS:
        if k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            assert np.array_equal(b[k], law[k]), k
            seen += 1
    assert seen == (5 if soft else 1 if name == "F" else 2)
    assert set(a) == set(b)
    dec.close()


# ------------------------------------------------------------------------------- 3. the defining property, device against device
@pytest.mark.parametrize("early", [True, False], ids=["early", "fixed"])
@pytest.mark.parametrize("name, soft", CASES, ids=IDS)
def test_defining_property(name, soft, early):
    """Success, iterations and bits are decode_batch(precision="float64") on the exported inputs of the same handle (a call
    without hand-over); the soft case gives it probs64[outcome] as the last R columns."""
    i = mc_ref.instance(name)
    dec = _decoder(name)
    got = _sweep(dec, name, soft, early=early)
    with np.errstate(divide="ignore"):
        if name == "F":
            d = dec.decode_batch(i["H"].syndrome(got["errors"]), early_exit=early, precision="float64", input_vector_type="syndrome")
            success = (d["bits"] == got["errors"]).all(axis=1)
        else:
            cp = cases.probs64()[got["outcome"]] if soft else None
            d = dec.decode_batch(got["msg"], early_exit=early, precision="float64", channel_probs=cp)
            success = mc_ref.hqc_success(d["bits"], got["y"], i["N"])
    assert dec.last_compacted() == 0
    assert np.array_equal(got["iters"], d["iters"]) and np.array_equal(got["success"], success.astype(np.uint8))
    if soft:
        assert np.array_equal(got["bits"], d["bits"])
    dec.close()


# ------------------------------------------------------------------------------------- 4. compaction is invisible and counted
@pytest.mark.parametrize("name, soft", CASES, ids=IDS)
def test_compaction_is_invisible_and_counted(name, soft):
    """compact_after 0, 2, 4 and 40 (>= max_iter) give identical outputs; last_compacted() is the oracle's "running after k";
    fixed-iteration runs never hand over.  H2 at 4 is a whole compact tile and a ragged one (64 + 5), H1 under t9 at 4 a single
    compact tile of 3."""
    dec = _decoder(name, compact_after=0)
    flat = _sweep(dec, name, soft)
    assert dec.last_compacted() == 0 and dec.last_stats()["levels"] == 0
    for k in (2, 4, 40):
        dec.configure(compact_after=k)
        got = _sweep(dec, name, soft)
        st = dec.last_stats()
        print(f"{name}{' t9' if soft else ''} compact_after = {k}: {st}")
        assert dec.last_compacted() == st["compacted"] == cases.handed_over(name, soft, k), k
        assert st["levels"] == (1 if st["compacted"] else 0) and st["row_parallel"] == 0
        _same(got, flat)
        fixed = _sweep(dec, name, soft, early=False)
        assert dec.last_compacted() == 0 and dec.last_stats()["levels"] == 0 and (fixed["iters"] == MAX_ITER).all()
    dec.close()
    default = _decoder(name)  # the default hands over at 4
    _same(_sweep(default, name, soft), flat)
    assert default.last_compacted() == cases.handed_over(name, soft, 4)
    default.close()


# ----------------------------------------------------------------------------------------------------------- 5. cuts and groups
@pytest.mark.parametrize("name, soft", [("F", False), ("H2", False), ("H2", True)], ids=["F", "H2", "H2-t9"])
def test_cuts_and_groups(name, soft):
    dec = _decoder(name, compact_after=2)
    whole = _sweep(dec, name, soft)
    parts = [_sweep(dec, name, soft, runs=r, first=FIRST + f) for f, r in ((0, 63), (63, 64), (127, 3))]
    for k in whole:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    for batch in (1, 63, 64, 65):  # one lane, a ragged tile, a full one, a second tile of one lane
        part = _sweep(dec, name, soft, runs=batch)
        for k in whole:
            assert np.array_equal(part[k], whole[k][:batch]), (batch, k)
    dec.set_tile_group(1)
    _same(_sweep(dec, name, soft), whole)
    assert dec.last_compacted() == cases.handed_over(name, soft, 2)
    dec.set_tile_group(0)
    # a second seed with the high key word set: as a fresh handle decodes it, and other trials than the first seed's
    other = _sweep(dec, name, soft, seed=SEED + 2**32)
    fresh = _decoder(name)
    _same(other, _sweep(fresh, name, soft, seed=SEED + 2**32))
    assert not np.array_equal(other["errors" if name == "F" else "msg"], whole["errors" if name == "F" else "msg"])
    fresh.close()
    dec.close()


# ------------------------------------------------------------------------------------------------------------------ 6. reduction
def test_the_two_outcome_table_is_the_plain_sweep():
    """mc_hqc_run(want_stats=True, precision="float64") goes through the two-outcome table with probs = (eps, eps) as doubles:
    H2 at its own eps, success and iterations of mc_hqc_run(precision="float64") -- and of the oracle."""
    i = mc_ref.instance("H2")
    dec = _decoder("H2")
    plain = _sweep(dec, "H2")
    a = _sweep(dec, "H2", want_stats=True, want_bits=True)
    assert set(a) == set(plain) | {"stats", "bits"}
    _same(a, plain, plain.keys())
    b = dec.mc_hqc_run_soft(RUNS, i["omega"], hqc_soft_mc_ref.eps_table(i["eps"]), SEED, first_trial=FIRST, want_inputs=True, want_stats=True,
                            want_bits=True, precision="float64")
    _same(a, b, a.keys())
    ok, stats = cases.count(i["N"], a["bits"], a["msg"], a["y"])
    assert np.array_equal(a["stats"], stats) and np.array_equal(a["success"], ok) and 0 < ok.sum() < RUNS
    assert np.array_equal(a["bits"], cases.shared_oracle("H2")["bits"])
    only = dec.mc_hqc_run_soft(RUNS, i["omega"], cases.t9(), SEED, first_trial=FIRST, precision="float64")  # out_stats = NULL: the soft sweep
    assert "stats" not in only and only["msg"] is None
    _same(only, _sweep(dec, "H2", True), ("success", "iters", "flips", "cost"))
    dec.close()


# ------------------------------------------------------------------------------------------------------------------ 7. the handle
def test_invisible_to_the_fp32_sweeps():
    """An fp32 mc_hqc_run, a float64 one, the fp32 one again, on one handle: each is a fresh handle's."""
    dec = _decoder("H2")
    first32 = _sweep(dec, "H2", precision="float32")
    got64 = _sweep(dec, "H2")
    again32 = _sweep(dec, "H2", precision="float32")
    fresh = _decoder("H2")
    _same(got64, _sweep(fresh, "H2"))
    fresh.close()
    fresh = _decoder("H2")
    want32 = _sweep(fresh, "H2", precision="float32")
    _same(first32, want32)
    _same(again32, want32)
    fresh.close()
    ms = _decoder("H2", method="min_sum")  # float64 has no min-sum form: refused by the keyword, and the decoder goes on
    with pytest.raises(ValueError, match="no min-sum form"):
        _sweep(ms, "H2")
    assert _sweep(ms, "H2", precision="float32")["success"].shape == (RUNS,)
    ms.close()
    dec.close()


@pytest.mark.parametrize("soft", [False, True], ids=["eps", "t9"])
def test_a_growing_handle(soft):
    """H2's graph grown from 40 to 70 rows in steps of 10 (append_rows): at every step the float64 sweep is a fresh decoder's."""
    i = mc_ref.instance("H2")
    H, probs, N = i["H"], i["probs"], i["N"]

    def part(r):
        return S.TannerGraph.from_csr(r, N + r, H.row_ptr[: r + 1].copy(), H.col_idx[: H.row_ptr[r]].copy()), np.concatenate([probs[:N], probs[N : N + r]])

    g0, p0 = part(40)
    live = _decoder("H2", H=g0, probs=p0, compact_after=2)
    _sweep(live, "H2", soft)  # (its workspace and compact level exist before the graph grows)
    for r in (50, 60, 70):
        rp = H.row_ptr[r - 10 : r + 1].astype(np.int64)
        live.append_rows((rp - rp[0]).astype(np.int32), H.col_idx[rp[0] : rp[-1]], N + r, probs[N + r - 10 : N + r])
        g, p = part(r)
        got = _sweep(live, "H2", soft)
        fresh = _decoder("H2", H=g, probs=p)
        _same(got, _sweep(fresh, "H2", soft))
        fresh.close()
    ref = cases.soft_oracle("H2") if soft else cases.shared_oracle("H2")
    assert np.array_equal(got["iters"], ref["iters"]) and np.array_equal(got["success"], ref["success"])
    live.close()


class FromFirst(bp.BpDecoder):
    """The drivers count trials from 0; the oracle's keys are of trials FIRST .. FIRST + RUNS - 1."""

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, **kw):
        return super().mc_hqc_run_soft(runs, omega, table, seed, first_trial=FIRST + first_trial, **kw)


@pytest.mark.parametrize("chunk", [4096, 70])
def test_the_attack_curve_in_float64_is_the_oracles(chunk):
    """driver.hqc_attack_curve(bp_decoder=driver.sweeps_in("float64")) on H2's rows, ten at a time: the curve computed from the
    per-step float64 oracle decodes, and every row of decoder_stats."""
    sup, rows = cases.h2_code()
    i = mc_ref.instance("H2")
    got = driver.hqc_attack_curve(sup, i["N"], rows, i["omega"], cases.t9(), RUNS, SEED, cases.CURVE_STEP, chunk=chunk, max_iter=MAX_ITER,
                                  bp_decoder=driver.sweeps_in("float64", bp_decoder=FromFirst))
    need, successes = cases.curve_key()
    assert got["steps"].tolist() == list(cases.CURVE_STEPS) and np.array_equal(got["successes"], successes)
    assert np.array_equal(got["checks_needed"], need)
    for r in cases.CURVE_STEPS:
        assert np.array_equal(got["oracle_calls_needed"][need == r], cases.h2_cut_law(r)["cost"][need == r])
    for row in got["decoder_stats"]:
        key = cases.h2_cut_oracle(row["checks"])
        t = row["trial"]
        assert [row[c] for c in driver.HQC_STATS_COLUMNS] == key["stats"][t].tolist() and row["success"] == bool(key["success"][t])


# ------------------------------------------------------------------------------------------------- 8. device I/O and refusals
@pytest.mark.parametrize("optional", [True, False], ids=["all outputs", "required only"])
def test_device_outputs_between_guard_rows(optional):
    """SCALDPC_F_DEVICE_IO on the caller's stream, the three entries: every output is a torch tensor between guard rows that stay
    as they were; 70 trials leave 58 lanes of the second tile unwritten."""
    import torch

    runs = 70
    dev = "cuda"
    stream = torch.cuda.Stream()
    flags = lib.F_EARLY_EXIT | lib.F_DEVICE_IO

    def guarded(cols, dtype, fill):
        shape = (runs + 2,) + ((cols,) if cols else ())
        return torch.full(shape, fill, dtype=dtype, device=dev)

    def check(t, want, fill, k):
        t = t.cpu().numpy()
        assert np.array_equal(t[1:-1], want) and (t[[0, -1]] == fill).all(), k

    def ptr(t, wanted=True):
        return C.c_void_p(t[1:].data_ptr()) if wanted else None

    # F
    dec = _decoder("F", compact_after=2)
    host = _sweep(dec, "F", runs=runs)
    succ, iters, err = guarded(0, torch.uint8, 0xAA), guarded(0, torch.int32, -7), guarded(dec.n, torch.uint8, 0xAA)
    torch.cuda.synchronize()
    lib.check(dec._lib.scaldpc_mc_fer_run_f64(dec._h, FIRST, runs, SEED, MAX_ITER, flags, C.c_void_p(stream.cuda_stream), ptr(succ),
                                               ptr(iters, optional), ptr(err, optional)))
    stream.synchronize()
    check(succ, host["success"], 0xAA, "success")
    if optional:
        check(iters, host["iters"], -7, "iters"), check(err, host["errors"], 0xAA, "errors")
    else:
        assert (iters == -7).all() and (err == 0xAA).all()
    dec.close()
    # H2, plain and under t9
    i = mc_ref.instance("H2")
    dec = _decoder("H2", compact_after=2)
    host = _sweep(dec, "H2", runs=runs)
    succ, iters = guarded(0, torch.uint8, 0xAA), guarded(0, torch.int32, -7)
    msg, y = guarded(dec.n, torch.uint8, 0xAA), guarded(i["omega"], torch.int32, -7)
    torch.cuda.synchronize()
    lib.check(dec._lib.scaldpc_mc_hqc_run_f64(dec._h, i["omega"], i["eps"], FIRST, runs, SEED, MAX_ITER, flags, C.c_void_p(stream.cuda_stream),
                                               ptr(succ), ptr(iters, optional), ptr(msg, optional), ptr(y, optional)))
    stream.synchronize()
    check(succ, host["success"], 0xAA, "success")
    if optional:
        check(iters, host["iters"], -7, "iters"), check(msg, host["msg"], 0xAA, "msg"), check(y, host["y"], -7, "y")
    else:
        assert (iters == -7).all() and (msg == 0xAA).all() and (y == -7).all()
    host = _sweep(dec, "H2", True, runs=runs)
    t = cases.t9()
    out = dict(success=guarded(0, torch.uint8, 0xAA), iters=guarded(0, torch.int32, -7), msg=guarded(dec.n, torch.uint8, 0xAA),
               y=guarded(i["omega"], torch.int32, -7), outcome=guarded(i["R"], torch.uint8, 0xAA), flips=guarded(0, torch.int32, -7),
               cost=guarded(0, torch.int32, -7), stats=guarded(5, torch.int32, -7), bits=guarded(dec.n, torch.uint8, 0xAA))
    fill = {k: (-7 if v.dtype == torch.int32 else 0xAA) for k, v in out.items()}
    torch.cuda.synchronize()
    w, pr = np.ascontiguousarray(t["weights"], dtype=np.float64), cases.probs64()
    lib.check(dec._lib.scaldpc_mc_hqc_run_stats_f64(
        dec._h, i["omega"], lib.ptr(w), lib.ptr(t["flips"]), lib.ptr(pr), lib.ptr(t["costs"]), len(pr), FIRST, runs, SEED, MAX_ITER, flags,
        C.c_void_p(stream.cuda_stream), *[ptr(out[k], optional or k == "success") for k in SOFT_OUT + ("stats", "bits")]))
    stream.synchronize()
    for k, v in out.items():
        if optional or k == "success":
            check(v, host[k], fill[k], k)
        else:
            assert (v == fill[k]).all(), k
    dec.close()


def _table(**change):
    t = dict(weights=np.array([[0.5, 0.5], [0.25, 0.75]]), flips=np.array([1, 0]), probs=np.array([0.1, 0.2]), costs=np.array([2, 1]))
    t.update(change)
    return t


BAD_TABLES = {  # the validation list of scaldpc_mc_hqc_run_soft (include/scaldpc.h), probs in double
    "no outcome": _table(weights=np.zeros((2, 0)), flips=np.zeros(0), probs=np.zeros(0), costs=None),
    "33 outcomes": _table(weights=np.array([[1.0] + [0.0] * 32] * 2), flips=np.zeros(33), probs=np.zeros(33), costs=None),
    "a negative weight": _table(weights=np.array([[-0.5, 1.5], [0.25, 0.75]])),
    "a weight above 1": _table(weights=np.array([[0.5, 0.5], [1.5, 0.0]])),
    "a NaN weight": _table(weights=np.array([[0.5, 0.5], [np.nan, 0.75]])),
    "row 0 does not sum to 1": _table(weights=np.array([[0.5, 0.5 + 1e-5], [0.25, 0.75]])),
    "row 1 does not sum to 1": _table(weights=np.array([[0.5, 0.5], [0.25, 0.75 - 1e-5]])),
    "a negative probability": _table(probs=np.array([-0.1, 0.2])),
    "a probability above 1": _table(probs=np.array([0.1, 1.5])),
    "a probability that only rounds to 1": _table(probs=np.array([0.1, 1.0 + 1e-12])),
    "a probability that only rounds to 0": _table(probs=np.array([-1e-300, 0.2])),
    "a NaN probability": _table(probs=np.array([np.nan, 0.2])),
    "a flip of 2": _table(flips=np.array([2, 0])),
    "a negative cost": _table(costs=np.array([2, -1])),
    "a cost above 65535": _table(costs=np.array([65536, 1])),
}


def test_refusals_write_nothing_and_leave_the_handle_as_new():
    """Every refusal of the three entries: the status of the fp32 entry, no output touched (host arrays full of a sentinel), and
    the handle then sweeps exactly as a fresh one does."""
    runs = 70
    i = mc_ref.instance("H2")
    N, R, omega = i["N"], i["R"], i["omega"]
    dec = _decoder("H2")
    outs = dict(success=np.full(runs, 0x5A, np.uint8), iters=np.full(runs, -7, np.int32), msg=np.full((runs, dec.n), 0x5A, np.uint8),
                y=np.full((runs, 300), -7, np.int32), outcome=np.full((runs, R), 0x5A, np.uint8), flips=np.full(runs, -7, np.int32),
                cost=np.full(runs, -7, np.int32), stats=np.full((runs, 5), -7, np.int32), bits=np.full((runs, dec.n), 0x5A, np.uint8))
    sentinel = {k: v.copy() for k, v in outs.items()}
    L = dec._lib

    def soft(table=None, omega=omega, first=0, batch=runs, flags=lib.F_EARLY_EXIT, drop=()):
        t = table or _table()
        w = np.ascontiguousarray(t["weights"], dtype=np.float64)
        fl = np.ascontiguousarray(t["flips"], dtype=np.uint8)
        pr = np.ascontiguousarray(t["probs"], dtype=np.float64)
        cs = None if t["costs"] is None else np.ascontiguousarray(t["costs"], dtype=np.int32)
        ptrs = [None if k in drop else lib.ptr(outs[k]) for k in SOFT_OUT + ("stats", "bits")]
        return L.scaldpc_mc_hqc_run_stats_f64(dec._h, omega, lib.ptr(w), lib.ptr(fl), lib.ptr(pr), lib.ptr(cs), w.shape[1], first, batch, SEED,
                                              MAX_ITER, flags, None, *ptrs)

    def hqc(omega=omega, eps=0.06, first=0, batch=runs, flags=lib.F_EARLY_EXIT, drop=()):
        ptrs = [None if k in drop else lib.ptr(outs[k]) for k in ("success", "iters", "msg", "y")]
        return L.scaldpc_mc_hqc_run_f64(dec._h, omega, eps, first, batch, SEED, MAX_ITER, flags, None, *ptrs)

    def fer(first=0, batch=runs, flags=lib.F_EARLY_EXIT, drop=()):
        ptrs = [None if k in drop else lib.ptr(outs[k]) for k in ("success", "iters", "bits")]
        return L.scaldpc_mc_fer_run_f64(dec._h, first, batch, SEED, MAX_ITER, flags, None, *ptrs)

    common = {"a negative first trial": dict(first=-1), "no trial": dict(batch=0), "out_success = NULL": dict(drop=("success",)),
              "SCALDPC_F_ASYNC": dict(flags=lib.F_EARLY_EXIT | lib.F_ASYNC), "an unknown flag": dict(flags=1 << 9)}
    shape = {"omega below 0": dict(omega=-1), "omega above N": dict(omega=N + 1)}
    refused = [(fer, name, how, lib.EINVAL) for name, how in common.items()]
    refused += [(hqc, name, how, lib.EINVAL) for name, how in {**common, **shape, "eps above 1": dict(eps=1.5), "eps below 0": dict(eps=-0.1),
                                                               "a NaN eps": dict(eps=float("nan"))}.items()]
    refused += [(soft, name, how, lib.EINVAL) for name, how in {**common, **shape, "out_cost without costs": dict(table=_table(costs=None))}.items()]
    refused += [(soft, name, dict(table=t), lib.EINVAL) for name, t in BAD_TABLES.items()]
    for call, name, how, status in refused:
        assert call(**how) == status, (call.__name__, name)
        assert L.scaldpc_last_error(), name
        for k in outs:
            assert np.array_equal(outs[k], sentinel[k]), (call.__name__, name, k)
    # the sampler keeps a trial's positions in LDS: omega > 256 is SCALDPC_EDEGREE, on a graph that has that many columns
    wide = _decoder("S499")
    i499 = mc_ref.instance("S499")
    succ = np.full(4, 0x5A, np.uint8)
    assert L.scaldpc_mc_hqc_run_f64(wide._h, 257, 0.04, 0, 4, SEED, MAX_ITER, lib.F_EARLY_EXIT, None, lib.ptr(succ), None, None, None) == lib.EDEGREE
    t = _table()
    fl = t["flips"].astype(np.uint8)
    assert L.scaldpc_mc_hqc_run_stats_f64(wide._h, 257, lib.ptr(t["weights"]), lib.ptr(fl), lib.ptr(t["probs"]), None, 2, 0, 4,
                                          SEED, MAX_ITER, lib.F_EARLY_EXIT, None, lib.ptr(succ), *[None] * 8) == lib.EDEGREE
    assert (succ == 0x5A).all() and i499["N"] == 499
    wide.close()
    # no [Hin | I]: refused by both HQC entries, taken by the FER one
    rep = bp.bp_decoder(S.codes.rep_code_graph(9), error_rate=0.1)
    with pytest.raises(ValueError, match="Hin"):
        rep.mc_hqc_run(4, 2, 0.1, seed=1, precision="float64")
    with pytest.raises(ValueError, match="Hin"):
        rep.mc_hqc_run_soft(4, 2, _table(), seed=1, precision="float64")
    assert rep.mc_fer_run(4, seed=1, precision="float64")["success"].shape == (4,)
    rep.close()
    # the handle is as new: out_stats = NULL is taken (the soft sweep), and the next sweeps are a fresh handle's
    assert soft(drop=("stats",)) == lib.OK and (outs["stats"] == -7).all() and not (outs["iters"] == -7).any()
    after = _sweep(dec, "H2", True, runs=runs)
    fresh = _decoder("H2")
    _same(after, _sweep(fresh, "H2", True, runs=runs))
    _same(_sweep(dec, "H2", runs=runs), _sweep(fresh, "H2", runs=runs))
    fresh.close()
    dec.close()


def test_lifetime_and_allocation_failures():
    """create / float64 sweep with a hand-over / close returns every block; with the k-th allocation of the sweep failing the call
    returns SCALDPC_ENOMEM (MemoryError), leaks nothing, and the next call on the same handle succeeds."""
    L = lib.load()
    keys = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")
    base = lib.live_blocks()
    for _ in range(2):
        dec = _decoder("H2", compact_after=2)
        good = _sweep(dec, "H2", True)
        assert dec.last_compacted() == cases.handed_over("H2", True, 2) and lib.live_blocks()["device_blocks"] > base["device_blocks"]
        dec.close()
        assert all(lib.live_blocks()[k] == base[k] for k in keys)
    assert L.scaldpc_debug_fail_alloc(0) == 0
    failed = succeeded = 0
    try:
        for k in range(1, 100):
            dec = _decoder("H2", compact_after=2)
            assert L.scaldpc_debug_fail_alloc(k) == 0  # (armed: SCALDPC_DEBUG=1, tests/conftest.py)
            try:
                got = _sweep(dec, "H2", True)
                succeeded += 1
            except MemoryError:
                failed += 1
                L.scaldpc_debug_fail_alloc(0)
                got = _sweep(dec, "H2", True)  # the handle is usable: the next call succeeds
            L.scaldpc_debug_fail_alloc(0)
            _same(got, good)
            dec.close()
            assert all(lib.live_blocks()[k2] == base[k2] for k2 in keys), k
            if succeeded >= 2:
                break
    finally:
        L.scaldpc_debug_fail_alloc(0)
    # ratios, planes, both message arrays, counters, the ratio plane, trial planes, staging, the compact level's planes
    assert failed >= 12 and succeeded >= 2, (failed, succeeded)


# ------------------------------------------------------------------------------------------------------------ 9. full size, once
def test_full_size_once():
    """The HQC-128 graph at R = 2000 of ref64_cases.full_size_case (its eps = 0 priors: trials of this point stay stuck), 130
    trials = three tiles, 50 iterations, early exit, the default compact_after: success and iterations of all 130 are
    decode_batch(precision="float64") on the exported inputs, and last_compacted() is the count that call's iteration counts
    and converged flags give."""
    H, probs, _ = ref64_cases.full_size_case()
    N = H.n - H.m
    omega = int(round(float(probs[0]) * N))
    it = ref64_cases.FULL_SIZE_ITERS
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(H, max_iter=it, bp_method="product_sum", channel_probs=probs)
        got = dec.mc_hqc_run(RUNS, omega, float(probs[-1]), SEED, first_trial=FIRST, want_inputs=True, precision="float64")
        handed = dec.last_compacted()
        d = dec.decode_batch(got["msg"], early_exit=True, precision="float64")
    assert dec.last_compacted() == 0
    late = (d["iters"] > 4) | (d["converged"] == 0)
    print(f"full size: {int(got['success'].sum())} of {RUNS} recovered, {handed} handed over, {int((d['converged'] == 0).sum())} stuck")
    assert np.array_equal(got["iters"], d["iters"]) and np.array_equal(got["success"], mc_ref.hqc_success(d["bits"], got["y"], N))
    assert handed == int(late.sum()) and (d["converged"] == 0).any() and 0 < handed
    dec.close()


# ------------------------------------------------------------------------------------------------------------------ 10. the audit
def test_the_audit_is_the_two_sweeps():
    """hqc_precision_audit on H2 under t9, 130 trials (the drivers count from 0): its fields are what the two sweeps return
    separately, whatever the chunk."""
    i = mc_ref.instance("H2")
    dec = _decoder("H2")
    with np.errstate(divide="ignore"):
        a = dec.mc_hqc_run_soft(RUNS, i["omega"], cases.t9(), SEED, precision="float32")
        b = dec.mc_hqc_run_soft(RUNS, i["omega"], cases.t9(), SEED, precision="float64")
    dec.close()
    for chunk in (4096, 64, 100):
        got = driver.hqc_precision_audit(i["Hin"], i["N"], i["omega"], cases.t9(), RUNS, SEED, chunk=chunk, max_iter=MAX_ITER)
        assert got["runs"] == RUNS and got["successes32"] == int(a["success"].sum()) and got["successes64"] == int(b["success"].sum())
        assert np.array_equal(got["success_differs"], np.flatnonzero(a["success"] != b["success"]))
        assert got["iters_differ"] == int((a["iters"] != b["iters"]).sum())
        assert np.array_equal(got["iter_hist32"], np.bincount(a["iters"], minlength=MAX_ITER + 1))
        assert np.array_equal(got["iter_hist64"], np.bincount(b["iters"], minlength=MAX_ITER + 1))
    print(f"audit on H2 under t9: {got['success_differs'].size} successes and {got['iters_differ']} iteration counts differ")
    assert 0 < got["successes64"] < RUNS
