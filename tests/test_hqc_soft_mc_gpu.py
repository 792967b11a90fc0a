"""scaldpc_mc_hqc_run_soft on the GPU: HQC trials whose checks are answered by an outcome of the attack's oracle, drawn on the
device conditional on the check's true value, each bringing its own certainty into the decode (simulate/hqc.py:782-871).

Held to (1) the trial law restated in NumPy on the oracle's Philox words and secret (tests/hqc_soft_mc_ref.py): secrets,
outcomes, messages, flip and cost counts, bit for bit; (2) the defining property: success and iterations are those of
`decode_batch(msg, channel_probs=probs[outcome])` on the exported inputs, exactly, on every path; (3) the CPU oracle, one
call per codeword with its own priors (tests/soft_cases.py), at `helpers.compare`'s existing tolerances; (4) the reductions
to `mc_hqc_run`.  Every test calls the new entry, so every one fails on a library without it."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import hqc_soft_mc_ref as ref
import soft_cases
from helpers import S, compare, hqc_instance

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
trials = importlib.import_module("sca-ldpc_amd.trials")
lib = importlib.import_module("sca-ldpc_amd._lib")

N, W, R, OMEGA = 499, 7, 260, 5  # R is no multiple of 16 or 64; E = 2080: the LDS-resident decoder on `auto`
SEED, FIRST, RUNS, MAX_ITER = 42, 1000, 200, 40  # 200 trials: a ragged fourth tile
METHODS = ["min_sum", "product_sum"]


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER"):
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def instance(eps=0.04):
    H, Hin, probs, _, _ = hqc_instance(N, W, R, OMEGA, eps, 1, seed=11, flip=False)
    return H, Hin, probs


@functools.lru_cache(maxsize=None)
def wrapped_table():
    return trials.wrapped_oracle_table((0.98, 0.9), (0.999, 0.99))


@functools.lru_cache(maxsize=None)
def law(first=FIRST, runs=RUNS):
    """The NumPy law on the wrapped oracle's table (computed once per session, shared, left unchanged)."""
    return ref.draw(SEED, first, runs, instance()[1], OMEGA, wrapped_table())


def _decoder(method, eps=0.04, max_iter=MAX_ITER, **knobs):
    H, _, probs = instance(eps)
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(H, max_iter=max_iter, bp_method=method, channel_probs=probs)
    if knobs:
        dec.configure(**knobs)
    return dec


def _is_the_law(r, want, runs=None):
    for k in ("y", "outcome", "msg", "flips", "cost"):
        assert np.array_equal(r[k], want[k][:runs]), k


def _is_the_soft_decode(dec, r, probs):
    """The defining property: success and iterations of the exported inputs under decode_batch(channel_probs=)."""
    d = dec.decode_batch(r["msg"], early_exit=True, channel_probs=probs, want_llr=True)
    assert np.array_equal(r["success"], trials.success(d["bits"], r["y"], dec.n - dec.m).astype(np.uint8)), "success"
    assert np.array_equal(r["iters"], d["iters"]), "iterations"
    return d


# ----------------------------------------------------------------------------------------- law, defining property, oracle sample
@pytest.mark.parametrize("path, runs", [("auto", RUNS), ("stream", RUNS), ("edge", 5)])
@pytest.mark.parametrize("method", METHODS)
def test_law_and_defining_property(oracle, method, path, runs):
    """`auto` is the LDS-resident kernel's plane form with per-codeword priors (k_bp_small<M, true, SoftPrior>), `stream` the
    64-codeword-tile kernels, `edge` the row-parallel ones.  The CPU oracle on exactly these 200 trials succeeds on 175 (tanh
    rule) and 176 (min-sum)."""
    dec = _decoder(method, path=path)
    r = dec.mc_hqc_run_soft(runs, OMEGA, wrapped_table(), seed=SEED, first_trial=FIRST, want_inputs=True)
    st = dec.last_stats()
    assert st["row_parallel"] == (runs if path == "edge" else 0)
    _is_the_law(r, law(), runs)
    d = _is_the_soft_decode(dec, r, law()["probs"][:runs])
    if runs == RUNS:
        assert 0 < r["success"].sum() < RUNS
    # the oracle sample: the first 24 trials, each decoded with its own priors
    k = min(24, runs)
    H, _, probs = instance()
    key = soft_cases.oracle_per_codeword(oracle, H, probs, law()["probs"][:k], law()["msg"][:k], 1, MAX_ITER, method)
    got = dict(soft_cases.take(d, slice(0, k)), iters=r["iters"][:k])  # (the entry's own iteration counts)
    compare(got, key, method)
    # success against the oracle's decisions: min-sum everywhere, the tanh rule wherever no tie moved a decision (compare)
    same = (d["bits"][:k, :N] == key["bits"][:, :N]).all(axis=1)
    assert same.all() or method != "min_sum"
    assert np.array_equal(r["success"][:k][same], trials.success(key["bits"], law()["y"][:k], N)[same].astype(np.uint8))
    dec.close()


# ----------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("method", METHODS)
def test_two_outcomes_are_mc_hqc_run(method, path):
    dec = _decoder(method, path=path)
    a = dec.mc_hqc_run(RUNS, omega=OMEGA, eps=0.04, seed=SEED, first_trial=FIRST, want_inputs=True)
    b = dec.mc_hqc_run_soft(RUNS, OMEGA, ref.eps_table(0.04), seed=SEED, first_trial=FIRST, want_inputs=True)
    for k in ("success", "iters", "msg", "y"):
        assert np.array_equal(a[k], b[k]), k
    assert b["cost"] is None and np.array_equal(b["flips"], (b["outcome"] == 0).sum(axis=1))
    assert 0 < b["flips"].sum() and b["success"].mean() > 0.3
    dec.close()


def test_one_outcome_of_certainty_one_is_mc_hqc_run_without_noise():
    dec = _decoder("product_sum", eps=0.0)
    a = dec.mc_hqc_run(RUNS, omega=OMEGA, eps=0.0, seed=SEED, first_trial=FIRST, want_inputs=True)
    one = dict(weights=np.ones((2, 1)), flips=np.zeros(1, dtype=np.uint8), probs=np.zeros(1), costs=np.array([3]))
    b = dec.mc_hqc_run_soft(RUNS, OMEGA, one, seed=SEED, first_trial=FIRST, want_inputs=True)
    for k in ("success", "iters", "msg", "y"):
        assert np.array_equal(a[k], b[k]), k
    assert not b["outcome"].any() and not b["flips"].any() and (b["cost"] == 3 * R).all()
    dec.close()


# ----------------------------------------------------------------------------------------------------------------------- cuts
@pytest.mark.parametrize("path", ["auto", "stream"])
def test_a_trial_depends_on_its_global_index_alone(path):
    dec = _decoder("min_sum", path=path)
    whole = dec.mc_hqc_run_soft(RUNS, OMEGA, wrapped_table(), seed=SEED, first_trial=FIRST, want_inputs=True)
    a = dec.mc_hqc_run_soft(70, OMEGA, wrapped_table(), seed=SEED, first_trial=FIRST, want_inputs=True)
    b = dec.mc_hqc_run_soft(130, OMEGA, wrapped_table(), seed=SEED, first_trial=FIRST + 70, want_inputs=True)
    for k in whole:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    dec.close()


def test_the_trial_index_crosses_32_bits_inside_a_call():
    first = 2**32 - 100
    dec = _decoder("min_sum", path="stream")
    r = dec.mc_hqc_run_soft(RUNS, OMEGA, wrapped_table(), seed=SEED, first_trial=first, want_inputs=True)
    want = law(first)
    _is_the_law(r, want)
    assert not np.array_equal(want["msg"][:100], law()["msg"][:100])
    _is_the_soft_decode(dec, r, want["probs"])
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- table edges
def edge_table():
    """K = 32: outcomes of weight 0 in the middle and at the end; one outcome with p = 0 (LLR +inf, reported right), one with
    p = 0.5 (LLR 0); the row of true bit 1 has all its weight on ONE outcome."""
    w = np.zeros((2, 32))
    w[0, [0, 5, 17, 29]] = [0.5, 0.3, 0.15, 0.05]
    w[1, 5] = 1.0
    flips = np.zeros(32, dtype=np.uint8)
    flips[[17, 29, 30]] = 1
    probs = np.linspace(0.01, 0.4, 32)
    probs[[0, 5, 17, 29]] = [0.0, 0.05, 0.2, 0.5]
    return dict(weights=w, flips=flips, probs=probs, costs=np.arange(32, dtype=np.int32) * 2000)


@pytest.mark.parametrize("path", ["auto", "stream"])
def test_table_edges(path):
    t = edge_table()
    _, Hin, _ = instance()
    want = ref.draw(SEED, FIRST, RUNS, Hin, OMEGA, t)
    assert set(np.unique(want["outcome"])) == {0, 5, 17, 29}
    dec = _decoder("product_sum", path=path)
    with np.errstate(divide="ignore"):
        r = dec.mc_hqc_run_soft(RUNS, OMEGA, t, seed=SEED, first_trial=FIRST, want_inputs=True)
    _is_the_law(r, want)
    true_bits = r["msg"][:, N:] ^ t["flips"][r["outcome"]]
    assert (r["outcome"][true_bits == 1] == 5).all() and (true_bits == 1).sum() > 100
    assert r["cost"].max() > 2**16  # sums of costs, not bytes
    _is_the_soft_decode(dec, r, want["probs"])
    dec.close()


# ------------------------------------------------------------------------------------------------------------ full size, once
def test_full_size_trials_go_through_the_compact_pass():
    """HQC-128, W 50, R 4000 (tests/soft_cases.py's point), the law of its host-drawn trials as a table, 4096 trials, tanh rule,
    early exit, max_iter 100: equal to decode_batch(channel_probs=) on the exported inputs, stragglers re-decoded in dense
    tiles -- the prior plane the generator wrote is gathered for them (k_gather_prior).  (The CPU oracle on the first 256 of
    these trials: 227 need more than 4 iterations, 58 never converge -- so a compact pass there must be.)"""
    label = "hqc128_W50_R4000_soft"
    H, Hin, N128, omega = soft_cases.soft_graph(label)
    p = soft_cases.SOFT_POINTS[label]
    t = trials.levels_table(p["levels"], p["weights"])
    dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=soft_cases.shared_priors(label))
    runs = 4096
    r = dec.mc_hqc_run_soft(runs, omega, t, seed=7, want_inputs=True)
    assert dec.last_stats()["compacted"] > 0
    assert r["cost"] is None and r["outcome"].max() == 5 and 0 not in r["outcome"]  # certainty 1.0 is never reported wrong
    y = np.zeros((runs, N128), dtype=np.uint8)
    np.put_along_axis(y, r["y"].astype(np.int64), 1, axis=1)
    assert np.array_equal(r["msg"][:, N128:], Hin.syndrome(y) ^ t["flips"][r["outcome"]]) and not r["msg"][:, :N128].any()
    assert np.array_equal(r["flips"], (r["outcome"] % 2 == 0).sum(axis=1))
    freq = np.bincount(r["outcome"].reshape(-1), minlength=6) / r["outcome"].size
    assert np.abs(freq - t["weights"][0]).max() < 1e-3  # 16 M draws: a standard deviation of at most 1.3e-4 per outcome
    d = dec.decode_batch(r["msg"], early_exit=True, channel_probs=t["probs"].astype(np.float32)[r["outcome"]])
    assert dec.last_stats()["compacted"] > 0
    assert np.array_equal(r["iters"], d["iters"])
    assert np.array_equal(r["success"], trials.success(d["bits"], r["y"], N128).astype(np.uint8))
    assert (r["iters"] > 4).mean() > 0.5 and 0 < r["success"].sum() < runs
    dec.close()


# ------------------------------------------------------------------------------------------------------------------------ also
def test_device_outputs():
    """SCALDPC_F_DEVICE_IO: the seven outputs are device pointers (torch tensors)."""
    import torch

    t = wrapped_table()
    dec = _decoder("min_sum", path="stream")
    host = dec.mc_hqc_run_soft(RUNS, OMEGA, t, seed=9, first_trial=3, want_inputs=True)
    dev = dict(success=torch.zeros(RUNS, dtype=torch.uint8, device="cuda"), iters=torch.zeros(RUNS, dtype=torch.int32, device="cuda"),
               msg=torch.zeros((RUNS, dec.n), dtype=torch.uint8, device="cuda"),
               y=torch.zeros((RUNS, OMEGA), dtype=torch.int32, device="cuda"),
               outcome=torch.zeros((RUNS, R), dtype=torch.uint8, device="cuda"),
               flips=torch.zeros(RUNS, dtype=torch.int32, device="cuda"), cost=torch.zeros(RUNS, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()  # stream = NULL below means the handle's own stream: order it after torch's fills
    w = np.ascontiguousarray(t["weights"], dtype=np.float64)
    pr = np.ascontiguousarray(t["probs"], dtype=np.float32)
    lib.check(dec._lib.scaldpc_mc_hqc_run_soft(
        dec._h, OMEGA, lib.ptr(w), lib.ptr(t["flips"]), lib.ptr(pr), lib.ptr(t["costs"]), len(pr), 3, RUNS, 9, MAX_ITER,
        lib.BP_MIN_SUM, 1.0, lib.F_EARLY_EXIT | lib.F_DEVICE_IO, None,
        *[C.c_void_p(dev[k].data_ptr()) for k in ("success", "iters", "msg", "y", "outcome", "flips", "cost")]))
    for k, v in dev.items():
        assert np.array_equal(v.cpu().numpy(), host[k]), k
    dec.close()


def _table(**change):
    t = dict(weights=np.array([[0.5, 0.5], [0.25, 0.75]]), flips=np.array([1, 0]), probs=np.array([0.1, 0.2]), costs=np.array([2, 1]))
    t.update(change)
    return t


BAD_TABLES = {
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


def test_refusals():
    """Every refusal of the validation list (include/scaldpc.h) is a ValueError and leaves the decoder usable.  (R * max cost
    >= 2^31 needs more than 32 768 checks: tests/test_hqc_soft_mc.py holds that one on the host header.)"""
    dec = _decoder("min_sum")
    good = dec.mc_hqc_run_soft(70, OMEGA, _table(), seed=1)
    for name, t in BAD_TABLES.items():
        with pytest.raises(ValueError):
            dec.mc_hqc_run_soft(70, OMEGA, t, seed=1)
            pytest.fail(name)
    for omega in (-1, N + 1):
        with pytest.raises(ValueError, match="omega"):
            dec.mc_hqc_run_soft(70, omega, _table(), seed=1)
    with pytest.raises(ValueError, match="first_trial"):
        dec.mc_hqc_run_soft(70, OMEGA, _table(), seed=1, first_trial=-1)
    # out_cost without costs; a flag the entry does not take (straight at the C ABI)
    w, fl, pr = np.array([[0.5, 0.5], [0.25, 0.75]]), np.array([1, 0], dtype=np.uint8), np.array([0.1, 0.2], dtype=np.float32)
    succ, cost = np.zeros(70, dtype=np.uint8), np.zeros(70, dtype=np.int32)
    for flags, out_cost, word in ((lib.F_EARLY_EXIT, cost, b"out_cost"), (lib.F_EARLY_EXIT | lib.F_ASYNC, None, b"flags")):
        rc = dec._lib.scaldpc_mc_hqc_run_soft(dec._h, OMEGA, lib.ptr(w), lib.ptr(fl), lib.ptr(pr), None, 2, 0, 70, 1, MAX_ITER,
                                              lib.BP_MIN_SUM, 1.0, flags, None, lib.ptr(succ), None, None, None, None, None,
                                              lib.ptr(out_cost))
        assert rc == lib.EINVAL and word in dec._lib.scaldpc_last_error()
    again = dec.mc_hqc_run_soft(70, OMEGA, _table(), seed=1)
    assert all(np.array_equal(good[k], again[k]) for k in ("success", "iters", "flips", "cost"))
    dec.close()


def test_the_graph_must_end_in_an_identity_block():
    g = S.codes.rep_code_graph(9)
    dec = bp.bp_decoder(g, error_rate=0.1)
    with pytest.raises(ValueError, match="Hin"):
        dec.mc_hqc_run_soft(4, 2, _table(), seed=1)
    dec.close()


def test_nothing_is_left_behind():
    """create / run / destroy: scaldpc_debug_live_blocks is back where it started (the accumulators, the prior plane and the
    outcome staging block are the handle's)."""
    before = lib.live_blocks()
    dec = _decoder("product_sum", path="stream")
    dec.mc_hqc_run_soft(RUNS, OMEGA, wrapped_table(), seed=SEED, want_inputs=True)
    during = lib.live_blocks()
    assert during["device_blocks"] > before["device_blocks"]
    dec.close()
    after = lib.live_blocks()
    for k in ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes"):
        assert after[k] == before[k], k
