"""scaldpc_mc_hqc_run_stats on the GPU: the HQC sweep that also returns, per trial, the counters tracking.add_decoder_stats keeps
(simulate/hqc.py:709-758) -- counted on the device by k_mc_hqc_stats from the planes the decode leaves -- and the decoded word;
and driver.hqc_attack_curve, the checks-needed curve on one growing decoder.

Held to (1) the defining property: stats, success and bits are driver.hqc_stats / decode_batch(channel_probs=) on the exported
inputs, integer for integer, on every path; (2) the plain sweep: everything it returns is returned unchanged; (3) the CPU oracle's
table (tests/hqc_stats_cases.py, recomputed and pinned by tests/test_hqc_stats.py); (4) fresh decoders on the prefix graphs.
Every test calls the new entry, so every one fails on a library without it."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hqc_soft_mc_ref as ref
import hqc_stats_cases as cases
import soft_cases
from helpers import compare
from hqc_stats_cases import FIRST, MAX_ITER, N, OMEGA, R, RUNS, SEED, STEP, STEPS

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
driver = importlib.import_module("sca-ldpc_amd.driver")
trials = importlib.import_module("sca-ldpc_amd.trials")
lib = importlib.import_module("sca-ldpc_amd._lib")

METHODS = ["min_sum", "product_sum"]
PLAIN = ("success", "iters", "msg", "y", "outcome", "flips", "cost")  # the plain sweep's outputs, in the order of the C ABI


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER"):
        monkeypatch.delenv(v, raising=False)


def _decoder(method, r=R, eps=0.04, cls=None, **knobs):
    H, _, probs = cases.cut(r)
    probs = np.concatenate([probs[:N], np.full(r, eps)])
    with np.errstate(divide="ignore"):
        dec = (cls or bp.bp_decoder)(H, max_iter=MAX_ITER, bp_method=method, channel_probs=probs)
    if knobs:
        dec.configure(**knobs)
    return dec


def _sweep(dec, runs=RUNS, table=None, omega=OMEGA, first=FIRST, **kw):
    kw = dict(dict(want_inputs=True, want_stats=True, want_bits=True), **kw)
    with np.errstate(divide="ignore"):
        return dec.mc_hqc_run_soft(runs, omega, table or cases.wrapped_table(), seed=SEED, first_trial=first, **kw)


def _same(a, b, keys=None):
    for k in keys or a.keys() | b.keys():
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


def _is_the_defining_property(dec, r, table=None):
    """stats, success and bits against the host route on the exported inputs: decode_batch(channel_probs=) + driver.hqc_stats."""
    probs = np.asarray((table or cases.wrapped_table())["probs"], dtype=np.float32)[r["outcome"]]
    with np.errstate(divide="ignore"):
        d = dec.decode_batch(r["msg"], early_exit=True, channel_probs=probs, want_llr=True)
    assert r["bits"].dtype == np.uint8 and np.array_equal(r["bits"], d["bits"]), "bits"
    success, stats = cases.count(d["bits"], r["msg"], r["y"])
    assert r["stats"].dtype == np.int32 and r["stats"].shape == (len(success), 5)
    for k, name in enumerate(cases.COLUMNS):
        assert np.array_equal(r["stats"][:, k], stats[:, k]), name
    assert np.array_equal(r["success"], success), "success"
    assert np.array_equal(r["iters"], d["iters"]), "iterations"
    return d


# ------------------------------------------------------------------------------------------ the defining property, on every path
@pytest.mark.parametrize("path, runs", [("auto", RUNS), ("stream", RUNS), ("edge", 5)])
@pytest.mark.parametrize("method", METHODS)
def test_defining_property(method, path, runs):
    """`auto` is the LDS-resident decoder, `stream` the 64-codeword tiles, `edge` the row-parallel kernels."""
    dec = _decoder(method, path=path)
    r = _sweep(dec, runs)
    assert dec.last_stats()["row_parallel"] == (runs if path == "edge" else 0)
    law = cases.law()
    for k in ("y", "outcome", "msg", "flips", "cost"):
        assert np.array_equal(r[k], law[k][:runs]), k
    d = _is_the_defining_property(dec, r)
    _same(dec.mc_hqc_run_soft(runs, OMEGA, cases.wrapped_table(), seed=SEED, first_trial=FIRST, want_inputs=True), r, PLAIN)
    print(f"{method} {path}: (successes, {', '.join(cases.COLUMNS)}) = {cases.table_row(r)}")
    if method == "min_sum" and runs == RUNS:
        assert cases.table_row(r) == cases.MIN_SUM_TABLE[R]
    # the first 24 trials against the oracle's own decode: min-sum everywhere, the tanh rule wherever no tie moved a decision
    k = min(24, runs)
    key = cases.oracle_step(R, method)
    compare(dict(soft_cases.take(d, slice(0, k)), iters=r["iters"][:k]),
            {q: key[q][:k] for q in ("bits", "llr", "iters", "converged")}, method)
    same = (r["bits"][:k] == key["bits"][:k]).all(axis=1)
    assert same.all() or method != "min_sum"
    assert np.array_equal(r["success"][:k][same], key["success"][:k][same])
    assert np.array_equal(r["stats"][:k][same], key["stats"][:k][same])
    dec.close()


@pytest.mark.parametrize("method", METHODS)
def test_counters_are_read_after_the_compact_pass(method):
    """64-codeword tiles, compact_after = 2: the 200 trials are one group of four tiles, and at the first poll point at which at
    most half of them still run (tests/test_hqc_stats.py: ten (min-sum) / eleven (tanh rule) are left after iteration 4, and they
    are the trials whose counters are not a recovered key's) the stragglers are decoded again in tiles of their own.  Their
    decisions are scattered back before the counters are read: equal to the run without a compaction level."""
    dec = _decoder(method, path="stream", compact_after=2)
    r = _sweep(dec)
    st = dec.last_stats()
    print(f"{method} compact_after=2: {st}")
    assert st["levels"] >= 1 and 0 < st["compacted"] <= RUNS // 2, st
    _is_the_defining_property(dec, r)
    late = r["iters"] > 4
    assert 0 < late.sum() <= st["compacted"] and (r["stats"][late, 2:] > 0).any()
    dec.configure(compact_after=0)
    flat = _sweep(dec)
    assert dec.last_stats()["levels"] == 0 and dec.last_stats()["compacted"] == 0
    _same(r, flat)
    if method == "min_sum":
        assert cases.table_row(r) == cases.MIN_SUM_TABLE[R]
    dec.close()


# ------------------------------------------------------------------------------------------------------------------------ cuts
@pytest.mark.parametrize("path", ["auto", "stream"])
def test_a_trial_depends_on_its_global_index_alone(path):
    dec = _decoder("min_sum", path=path)
    whole = _sweep(dec)
    a, b = _sweep(dec, 70), _sweep(dec, 130, first=FIRST + 70)
    for k in whole:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    for batch in (1, 63, 64, 65):  # one lane, a ragged tile, a full one, a second tile of one lane
        part = _sweep(dec, batch)
        for k in whole:
            assert np.array_equal(part[k], whole[k][:batch]), (batch, k)
    dec.close()


# ------------------------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("method", METHODS)
def test_mc_hqc_run_with_stats_is_the_two_outcome_table(method, path):
    dec = _decoder(method, path=path)
    a = dec.mc_hqc_run(RUNS, omega=OMEGA, eps=0.04, seed=SEED, first_trial=FIRST, want_inputs=True, want_stats=True, want_bits=True)
    b = _sweep(dec, table=ref.eps_table(0.04))
    plain = dec.mc_hqc_run(RUNS, omega=OMEGA, eps=0.04, seed=SEED, first_trial=FIRST, want_inputs=True)
    assert set(a) == set(plain) | {"stats", "bits"}
    _same(a, b, a.keys())
    _same(a, plain, plain.keys())
    _is_the_defining_property(dec, b, ref.eps_table(0.04))
    assert 0 < a["success"].sum() < RUNS and (a["stats"].sum(axis=0) > 0).all()
    only = dec.mc_hqc_run(RUNS, omega=OMEGA, eps=0.04, seed=SEED, first_trial=FIRST, want_stats=True)
    assert only["bits"] is None and only["msg"] is None and np.array_equal(only["stats"], a["stats"])
    dec.close()


def test_one_outcome_of_certainty_one():
    """No noise (an eps = 0 decoder, K = 1, p = 0): every check is reported right, so `unsatisfied` is the weight of Hin y and a
    recovered key has no bad flip and no check found bad."""
    dec = _decoder("product_sum", eps=0.0)
    one = dict(weights=np.ones((2, 1)), flips=np.zeros(1, dtype=np.uint8), probs=np.zeros(1), costs=np.array([3]))
    r = _sweep(dec, table=one)
    _is_the_defining_property(dec, r, one)
    yv = np.zeros((RUNS, N), dtype=np.uint8)
    np.put_along_axis(yv, r["y"].astype(np.int64), 1, axis=1)
    assert np.array_equal(r["stats"][:, 0], cases.cut(R)[1].syndrome(yv).sum(axis=1))
    ok = r["success"].astype(bool)
    assert ok.sum() > RUNS // 2 and (r["stats"][ok, 1] == OMEGA).all() and not r["stats"][ok, 2:].any()
    assert not r["stats"][:, 3:].any()  # p = 0: no check column is ever flipped
    dec.close()


# ----------------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("path", ["auto", "stream"])
def test_no_secret(path):
    """omega = 0: nothing to find -- good_flips is 0, and every reported 1 is a wrong answer."""
    dec = _decoder("min_sum", path=path)
    r = _sweep(dec, omega=0)
    assert r["y"].shape == (RUNS, 0) and np.array_equal(r["stats"][:, 0], r["flips"])
    _is_the_defining_property(dec, r)
    assert not r["stats"][:, 1].any() and not r["stats"][:, 3].any()
    assert np.array_equal(r["success"], (r["stats"][:, 2] == 0).astype(np.uint8)) and r["success"].sum() > RUNS // 2
    dec.close()


@pytest.mark.parametrize("path", ["auto", "stream"])
def test_every_check_reported_wrong_and_the_priors_say_so(path):
    """K = 1, flips = (1), probs = (1.0): every check arrives complemented with the prior LLR -inf, so the decoder flips all R
    check columns back -- every check is found bad, split by what it reported."""
    dec = _decoder("min_sum", path=path)
    wrong = dict(weights=np.ones((2, 1)), flips=np.ones(1, dtype=np.uint8), probs=np.ones(1), costs=None)
    r = _sweep(dec, table=wrong)
    assert (r["flips"] == R).all()
    _is_the_defining_property(dec, r, wrong)
    st = r["stats"]
    assert np.array_equal(st[:, 4], st[:, 0]) and np.array_equal(st[:, 3], R - st[:, 0])
    assert np.array_equal(st[:, 0], r["msg"][:, N:].sum(axis=1)) and r["success"].sum() > RUNS // 2
    dec.close()


@pytest.mark.parametrize("with_bits", [True, False])
def test_device_outputs_between_guard_rows(with_bits):
    """SCALDPC_F_DEVICE_IO on the caller's stream: the nine outputs are device pointers (torch tensors); out_stats and out_bits
    sit between guard rows that stay as they were, and 70 trials leave six lanes of the second tile unwritten."""
    import torch

    runs = 70
    t = cases.wrapped_table()
    dec = _decoder("min_sum", path="stream")
    host = _sweep(dec, runs, first=3)
    dev = "cuda"
    out = dict(success=torch.zeros(runs, dtype=torch.uint8, device=dev), iters=torch.zeros(runs, dtype=torch.int32, device=dev),
               msg=torch.zeros((runs, dec.n), dtype=torch.uint8, device=dev), y=torch.zeros((runs, OMEGA), dtype=torch.int32, device=dev),
               outcome=torch.zeros((runs, R), dtype=torch.uint8, device=dev), flips=torch.zeros(runs, dtype=torch.int32, device=dev),
               cost=torch.zeros(runs, dtype=torch.int32, device=dev))
    stats = torch.full((runs + 2, 5), -7, dtype=torch.int32, device=dev)
    bits = torch.full((runs + 2, dec.n), 0xAA, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    w = np.ascontiguousarray(t["weights"], dtype=np.float64)
    pr = np.ascontiguousarray(t["probs"], dtype=np.float32)
    lib.check(dec._lib.scaldpc_mc_hqc_run_stats(
        dec._h, OMEGA, lib.ptr(w), lib.ptr(t["flips"]), lib.ptr(pr), lib.ptr(t["costs"]), len(pr), 3, runs, SEED, MAX_ITER,
        lib.BP_MIN_SUM, 1.0, lib.F_EARLY_EXIT | lib.F_DEVICE_IO, C.c_void_p(stream.cuda_stream),
        *[C.c_void_p(out[k].data_ptr()) for k in PLAIN], C.c_void_p(stats[1:].data_ptr()),
        C.c_void_p(bits[1:].data_ptr()) if with_bits else None))
    stream.synchronize()
    for k, v in out.items():
        assert np.array_equal(v.cpu().numpy(), host[k]), k
    stats, bits = stats.cpu().numpy(), bits.cpu().numpy()
    assert np.array_equal(stats[1:-1], host["stats"]) and (stats[[0, -1]] == -7).all()
    if with_bits:
        assert np.array_equal(bits[1:-1], host["bits"]) and (bits[[0, -1]] == 0xAA).all()
    else:
        assert (bits == 0xAA).all()
    dec.close()


# -------------------------------------------------------------------------------------------------------------------- refusals
def _table(**change):
    t = dict(weights=np.array([[0.5, 0.5], [0.25, 0.75]]), flips=np.array([1, 0]), probs=np.array([0.1, 0.2]), costs=np.array([2, 1]))
    t.update(change)
    return t


BAD_TABLES = {  # the validation list of scaldpc_mc_hqc_run_soft (include/scaldpc.h)
    "no outcome": _table(weights=np.zeros((2, 0)), flips=np.zeros(0), probs=np.zeros(0), costs=None),
    "33 outcomes": _table(weights=np.array([[1.0] + [0.0] * 32] * 2), flips=np.zeros(33), probs=np.zeros(33), costs=None),
    "a negative weight": _table(weights=np.array([[-0.5, 1.5], [0.25, 0.75]])),
    "a weight above 1": _table(weights=np.array([[0.5, 0.5], [1.5, 0.0]])),
    "a NaN weight": _table(weights=np.array([[0.5, 0.5], [np.nan, 0.75]])),
    "an infinite weight": _table(weights=np.array([[np.inf, 0.5], [0.25, 0.75]])),
    "row 0 does not sum to 1": _table(weights=np.array([[0.5, 0.5 + 1e-5], [0.25, 0.75]])),
    "row 1 does not sum to 1": _table(weights=np.array([[0.5, 0.5], [0.25, 0.75 - 1e-5]])),
    "a negative probability": _table(probs=np.array([-0.1, 0.2])),
    "a probability above 1": _table(probs=np.array([0.1, 1.5])),
    "a NaN probability": _table(probs=np.array([np.nan, 0.2])),
    "a flip of 2": _table(flips=np.array([2, 0])),
    "a negative cost": _table(costs=np.array([2, -1])),
    "a cost above 65535": _table(costs=np.array([65536, 1])),
}


def test_refusals_write_nothing_and_leave_the_handle_as_new():
    """Every refusal of the soft entry, and out_stats = NULL: SCALDPC_EINVAL, no output touched (host arrays full of a sentinel),
    and the handle then sweeps exactly as a fresh one does."""
    runs = 70
    dec = _decoder("min_sum")
    outs = dict(success=np.full(runs, 0x5A, np.uint8), iters=np.full(runs, -7, np.int32), msg=np.full((runs, dec.n), 0x5A, np.uint8),
                y=np.full((runs, OMEGA), -7, np.int32), outcome=np.full((runs, R), 0x5A, np.uint8), flips=np.full(runs, -7, np.int32),
                cost=np.full(runs, -7, np.int32), stats=np.full((runs, 5), -7, np.int32), bits=np.full((runs, dec.n), 0x5A, np.uint8))
    sentinel = {k: v.copy() for k, v in outs.items()}

    def call(table=None, omega=OMEGA, first=0, batch=runs, method=lib.BP_MIN_SUM, alpha=1.0, flags=lib.F_EARLY_EXIT, drop=()):
        t = table or _table()
        w = np.ascontiguousarray(t["weights"], dtype=np.float64)
        fl = np.ascontiguousarray(t["flips"], dtype=np.uint8)
        pr = np.ascontiguousarray(t["probs"], dtype=np.float32)
        cs = None if t["costs"] is None else np.ascontiguousarray(t["costs"], dtype=np.int32)
        ptrs = [None if k in drop else lib.ptr(outs[k]) for k in PLAIN + ("stats", "bits")]
        return dec._lib.scaldpc_mc_hqc_run_stats(dec._h, omega, lib.ptr(w), lib.ptr(fl), lib.ptr(pr), lib.ptr(cs), w.shape[1], first, batch,
                                                 SEED, MAX_ITER, method, alpha, flags, None, *ptrs)

    refused = {name: dict(table=t) for name, t in BAD_TABLES.items()}
    refused.update({
        "out_stats = NULL": dict(drop=("stats",)), "out_success = NULL": dict(drop=("success",)),
        "out_cost without costs": dict(table=_table(costs=None)), "omega below 0": dict(omega=-1), "omega above N": dict(omega=N + 1),
        "a negative first trial": dict(first=-1), "no trial": dict(batch=0), "an unknown method": dict(method=7),
        "a negative alpha": dict(alpha=-1.0), "a NaN alpha": dict(alpha=float("nan")),
        "SCALDPC_F_ASYNC": dict(flags=lib.F_EARLY_EXIT | lib.F_ASYNC), "an unknown flag": dict(flags=1 << 9),
    })  # fmt: skip
    for name, how in refused.items():
        assert call(**how) == lib.EINVAL, name
        assert dec._lib.scaldpc_last_error(), name
        for k in outs:
            assert np.array_equal(outs[k], sentinel[k]), (name, k)
    assert b"out_stats" in (call(drop=("stats",)), dec._lib.scaldpc_last_error())[1]
    assert call() == lib.OK and not (outs["stats"] == -7).any()
    after = _sweep(dec, runs, table=_table(), first=0)
    fresh_dec = _decoder("min_sum")
    fresh = _sweep(fresh_dec, runs, table=_table(), first=0)
    _same(after, fresh)
    for k in outs:
        assert np.array_equal(outs[k], fresh[k]), k
    fresh_dec.close()
    dec.close()


def test_the_graph_must_end_in_an_identity_block():
    from helpers import S

    dec = bp.bp_decoder(S.codes.rep_code_graph(9), error_rate=0.1)
    with pytest.raises(ValueError, match="Hin"):
        dec.mc_hqc_run_soft(4, 2, _table(), seed=1, want_stats=True)
    dec.close()


def test_nothing_is_left_behind():
    """create / sweep / close: scaldpc_debug_live_blocks is back where it started (the counters' staging block is the handle's)."""
    before = lib.live_blocks()
    dec = _decoder("product_sum", path="stream")
    _sweep(dec)
    assert lib.live_blocks()["device_blocks"] > before["device_blocks"]
    dec.close()
    after = lib.live_blocks()
    for k in ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes"):
        assert after[k] == before[k], k


# ------------------------------------------------------------------------------------------------------------ the growing handle
def _new_rows(r):
    """CSR of rows r - STEP .. r - 1 of the instance (each with its identity column) and the block length afterwards."""
    H = cases.cut(r)[0]
    lo, hi = H.row_ptr[r - STEP], H.row_ptr[r]
    return H.row_ptr[r - STEP : r + 1] - lo, H.col_idx[lo:hi], H.n


@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("method", METHODS)
def test_a_growing_handle_follows_the_same_trials(method, path):
    """65 rows, then 65 more at a time (append_rows) with ONE seed: at every step the sweep is a fresh decoder's on the prefix
    graph, all keys, and the min-sum rows are the oracle's table -- the same 200 keys, seen through more and more checks."""
    dec = _decoder(method, STEPS[0], path=path)
    for r in STEPS:
        if r > STEPS[0]:
            rp, ci, new_n = _new_rows(r)
            dec.append_rows(rp, ci, new_n, np.full(STEP, 0.5))
        got = _sweep(dec)
        fresh_dec = _decoder(method, r, path=path)
        _same(got, _sweep(fresh_dec))
        fresh_dec.close()
        law = cases.law(r)
        for k in ("y", "outcome", "msg", "flips", "cost"):
            assert np.array_equal(got[k], law[k]), (r, k)
        print(f"{method} {path} R = {r}: {cases.table_row(got)}")
        if method == "min_sum":
            assert cases.table_row(got) == cases.MIN_SUM_TABLE[r], r
    dec.close()


class FromFirst(bp.BpDecoder):
    """The drivers count trials from 0; the oracle's table is of trials FIRST .. FIRST + RUNS - 1."""

    def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, **kw):
        return super().mc_hqc_run_soft(runs, omega, table, seed, first_trial=FIRST + first_trial, **kw)


@pytest.mark.parametrize("chunk", [4096, 70])
def test_the_attack_curve_is_the_oracles(chunk):
    """driver.hqc_attack_curve on the HIP class, min-sum: checks_needed of tests/test_hqc_stats.py's oracle-backed double, exactly."""
    sup, rows = cases.code()
    got = driver.hqc_attack_curve(sup, N, rows, OMEGA, cases.wrapped_table(), RUNS, SEED, STEP, chunk=chunk, bp_method="min_sum",
                                  max_iter=MAX_ITER, bp_decoder=FromFirst)
    need = got["checks_needed"]
    assert got["steps"].tolist() == list(STEPS) and got["successes"].tolist() == [1, 13, 115, 176]
    assert np.array_equal(need, cases.checks_needed())
    for r in STEPS:
        assert np.array_equal(got["oracle_calls_needed"][need == r], cases.law(r)["cost"][need == r])
    rows_of = {(row["trial"], row["checks"]): row for row in got["decoder_stats"]}
    assert len(rows_of) == len(got["decoder_stats"]) == sum(STEPS.index(r) + 1 if r > 0 else len(STEPS) for r in need.tolist())
    for (t, r), row in rows_of.items():
        key = cases.oracle_step(r)
        assert [row[c] for c in cases.COLUMNS] == key["stats"][t].tolist() and row["success"] == bool(key["success"][t]), (t, r)


def test_the_sweep_sums_the_counters():
    got = driver.hqc_oracle_sweep(cases.cut(R)[1], N, OMEGA, cases.wrapped_table(), RUNS, SEED, chunk=70, bp_method="min_sum",
                                  max_iter=MAX_ITER, bp_decoder=FromFirst, want_stats=True)
    assert got["successes"] == 176 and got["stats"] == dict(zip(cases.COLUMNS, cases.MIN_SUM_TABLE[R][1:]))
    assert got["stats_success"]["bad_flips"] == 0 and got["stats_success"]["good_flips"] == 176 * OMEGA
