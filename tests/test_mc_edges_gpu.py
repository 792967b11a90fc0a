"""scaldpc_mc_fer_run and scaldpc_mc_hqc_run on the GPU, at their edges (the instances and what makes them hard enough:
tests/mc_ref.py, pinned on the CPU in tests/test_mc_edges.py).

Held, in this order of authority, to (1) the generators of oracle/mc_oracle.c through tests/mc_ref.py: exported errors, secrets
and messages bit for bit; (2) the defining property: success and iterations are those of the same handle's `decode_batch` on
the exported inputs, exactly, for both methods on every path; (3) the f32 CPU decoder on the first 24 trials of an instance,
at `helpers.compare`'s existing tolerances (min-sum bit-exact, posteriors included)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import mc_ref
from helpers import compare, prefix_graph
from mc_ref import FIRST, MAX_ITER, RUNS, SAMPLE, SEED

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")

METHODS = ["min_sum", "product_sum"]
PATHS = [("auto", RUNS), ("stream", RUNS), ("edge", 5)]  # LDS-resident decoder; 64-codeword-tile kernels; row-parallel kernels
MIN_SUM_WON = {"F": 54, "H1": 75}  # of the 130 trials, on the CPU decoder (tests/test_mc_edges.py)
GUARD = 0xA5


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER", "SCALDPC_SPLIT"):
        monkeypatch.delenv(v, raising=False)


def _decoder(name, method, probs=None, graph=None, **knobs):
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):  # (p = 0 and p = 1 among the priors)
        dec = bp.bp_decoder(i["H"] if graph is None else graph, max_iter=MAX_ITER, bp_method=method,
                            channel_probs=i["probs"] if probs is None else probs)
    if knobs:
        dec.configure(**knobs)
    return dec


def _run(dec, name, runs=RUNS, first=FIRST, seed=SEED, **kw):
    """The entry of the instance, inputs exported; omega and eps are the instance's unless given."""
    i = mc_ref.instance(name)
    if name == "F":
        return dec.mc_fer_run(runs, seed=seed, first_trial=first, want_errors=True, **kw)
    kw.setdefault("omega", i["omega"])
    kw.setdefault("eps", i["eps"])
    return dec.mc_hqc_run(runs, seed=seed, first_trial=first, want_inputs=True, **kw)


def _law(name, **kw):
    return mc_ref.fer_law(**kw) if name == "F" else mc_ref.hqc_law(name, **kw)


def _is_the_law(name, r, law, runs=None):
    for k in ("errors",) if name == "F" else ("y", "msg"):
        assert np.array_equal(r[k], law[k][:runs]), k


def _is_the_decode(dec, name, r, early_exit=True, max_iter=None):
    """The defining property: success and iterations of the exported inputs under the same handle's decode_batch."""
    N = mc_ref.instance(name)["N"]
    if name == "F":
        d = dec.decode_batch(mc_ref.instance(name)["H"].syndrome(r["errors"]), early_exit=early_exit, max_iter=max_iter,
                             want_llr=True, input_vector_type="syndrome")
        want = (d["bits"] == r["errors"]).all(axis=1)
    else:
        d = dec.decode_batch(r["msg"], early_exit=early_exit, max_iter=max_iter, want_llr=True, input_vector_type="received")
        want = mc_ref.hqc_success(d["bits"], r["y"], N)
    assert np.array_equal(r["success"], want.astype(np.uint8)), "success"
    assert np.array_equal(r["iters"], d["iters"]), "iterations"
    return d


def _is_the_oracle_sample(name, method, r, d, **how):
    """The first 24 trials against the f32 CPU decoder, as test_hqc_soft_mc_gpu.py::test_law_and_defining_property holds them."""
    k = min(SAMPLE, len(r["success"]))
    key = {f: v[:k] for f, v in mc_ref.oracle_decode(name, method, runs=SAMPLE, **how).items()}
    got = dict({f: v[:k] for f, v in d.items()}, iters=r["iters"][:k])  # (the entry's own iteration counts)
    compare(got, {f: key[f] for f in ("bits", "llr", "iters", "converged")}, method)
    # success against the oracle's decisions: min-sum everywhere, the tanh rule wherever no tie moved a decision (compare)
    cols = slice(None) if name == "F" else slice(0, mc_ref.instance(name)["N"])
    same = (d["bits"][:k, cols] == key["bits"][:, cols]).all(axis=1)
    assert same.all() or method != "min_sum"
    assert np.array_equal(r["success"][:k][same], key["success"][same])


def _same(a, b, keys=None):
    for k in keys or a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


# ----------------------------------------------------------------------------- 1. law, defining property, oracle: every path
@pytest.mark.parametrize("path, runs", PATHS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["F", "H1"])
def test_law_and_defining_property(name, method, path, runs):
    dec = _decoder(name, method, path=path)
    r = _run(dec, name, runs)
    assert dec.last_stats()["row_parallel"] == (runs if path == "edge" else 0)
    _is_the_law(name, r, _law(name), runs)
    d = _is_the_decode(dec, name, r)
    _is_the_oracle_sample(name, method, r, d)
    if runs == RUNS:
        assert 0 < r["success"].sum() < RUNS and len(set(r["iters"].tolist())) >= 4
        if method == "min_sum":
            assert int(r["success"].sum()) == MIN_SUM_WON[name]
    dec.close()


@pytest.mark.parametrize("how", [dict(early_exit=False), dict(max_iter=7)], ids=["fixed", "max_iter_7"])
@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["F", "H1"])
def test_fixed_iterations_and_max_iter_per_call(name, method, path, how):
    dec = _decoder(name, method, path=path)
    r = _run(dec, name, **how)
    _is_the_law(name, r, _law(name))
    d = _is_the_decode(dec, name, r, **how)
    _is_the_oracle_sample(name, method, r, d, **how)
    assert r["iters"].max() == how.get("max_iter", MAX_ITER) and 0 < r["success"].sum() < RUNS
    if "max_iter" in how:
        assert len(set(r["iters"].tolist())) >= 4
    else:
        assert (r["iters"] == MAX_ITER).all()
    dec.close()


# --------------------------------------------------------------------------------------- 2. a compaction level at small size
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["F", "H2"])
def test_stragglers_go_through_a_compaction_level(name, method):
    """64-codeword-tile kernels, compact_after = 2: the 130 trials are one group of three tiles, and at the first poll point
    from iteration 2 on at which at most half of them still run (iteration 4 or 8: tests/test_mc_edges.py) the stragglers
    are gathered into one tile and decoded again from their inputs.  Equal to the run without a compact pass."""
    dec = _decoder(name, method, path="stream", compact_after=2)
    r = _run(dec, name)
    st = dec.last_stats()
    print(f"{name} {method} compact_after=2: {st}")
    assert st["levels"] >= 1 and 0 < st["compacted"] <= RUNS // 2, st
    _is_the_law(name, r, _law(name))
    d = _is_the_decode(dec, name, r)
    _is_the_oracle_sample(name, method, r, d)
    late = r["iters"] > 4
    assert late[:SAMPLE].any() and not late[:SAMPLE].all()  # the oracle sample holds codewords of both kinds
    dec.configure(compact_after=0)
    flat = _run(dec, name)
    assert dec.last_stats()["levels"] == 0 and dec.last_stats()["compacted"] == 0
    _same(r, flat)
    dec.close()


# ------------------------------------------------------------------------------------------------ 3. counter and key words
@pytest.mark.parametrize("name", ["F", "H1"])
def test_the_high_key_word_and_the_high_counter_word(name):
    dec = _decoder(name, "min_sum")
    a = _run(dec, name, 70)
    b = _run(dec, name, 70, seed=SEED + (1 << 32))
    key = "errors" if name == "F" else "y"
    assert not np.array_equal(a[key], b[key])
    _is_the_law(name, b, _law(name, runs=70, seed=SEED + (1 << 32)))
    c = _run(dec, name, 70, first=2**40 + 7)
    _is_the_law(name, c, _law(name, runs=70, first=2**40 + 7))
    assert not np.array_equal(c[key], _law(name, runs=70, first=7)[key])
    _is_the_decode(dec, name, c)
    dec.close()


@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("name", ["F", "H2"])
def test_a_split_at_the_32_bit_crossing_is_the_whole(name, path):
    dec = _decoder(name, "min_sum", path=path)
    whole = _run(dec, name)
    a = _run(dec, name, 30)  # trials 2^32 - 30 .. 2^32 - 1
    b = _run(dec, name, 100, first=2**32)
    for k in whole:
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    _is_the_law(name, whole, _law(name))
    dec.close()


def test_a_batch_is_the_first_rows_of_a_larger_one():
    dec = _decoder("F", "product_sum", path="stream")
    whole = _run(dec, "F")
    for runs in (1, 63, 64, 65, RUNS):
        r = _run(dec, "F", runs)
        for k in whole:
            assert np.array_equal(r[k], whole[k][:runs]), (k, runs)
    dec.close()


# ------------------------------------------------------------------------------------------------------ 4. threshold cache
def _fer_is(dec, probs, graph):
    r = dec.mc_fer_run(RUNS, seed=SEED, first_trial=FIRST, want_errors=True)
    err, synd = mc_ref.fer(SEED, FIRST, RUNS, graph, probs)
    assert np.array_equal(r["errors"], err)
    d = dec.decode_batch(synd, input_vector_type="syndrome")  # (the priors in force are the decode's too)
    assert np.array_equal(r["success"], (d["bits"] == err).all(axis=1).astype(np.uint8)) and np.array_equal(r["iters"], d["iters"])
    return r


def test_thresholds_follow_the_priors():
    """The thresholds of the Bernoulli draw are cached on the device: scaldpc_bp_set_channel_probs and
    scaldpc_bp_set_channel_probs_tail must each drop them."""
    i = mc_ref.instance("F")
    p1 = i["probs"]
    dec = _decoder("F", "min_sum")
    first = _fer_is(dec, p1, i["H"])
    p2 = 0.6 * p1 + 0.013  # every value changed: p = 0 and p = 1 gone from their places ...
    p2[[7, 199]] = [1.0, 0.0]  # ... and put elsewhere
    assert (p2 != p1).all()
    with np.errstate(divide="ignore"):
        dec.update_channel_probs(p2)
    second = _fer_is(dec, p2, i["H"])
    assert not np.array_equal(first["errors"], second["errors"])
    p3 = p2.copy()
    p3[i["N"]:] = np.linspace(0.0, 0.12, i["R"])  # the last 70 columns only
    tail = np.ascontiguousarray(p3[i["N"]:])
    with np.errstate(divide="ignore"):
        lib.check(dec._lib.scaldpc_bp_set_channel_probs_tail(dec._h, i["N"], i["R"], lib.ptr(tail)))
    third = _fer_is(dec, p3, i["H"])
    assert np.array_equal(third["errors"][:, : i["N"]], second["errors"][:, : i["N"]])
    assert not np.array_equal(third["errors"][:, i["N"]:], second["errors"][:, i["N"]:])
    dec.close()


def test_thresholds_follow_a_graph_that_grows():
    """scaldpc_bp_append_rows drops the thresholds and their buffer (n grows): 50 checks, a run, 20 checks more."""
    i = mc_ref.instance("F")
    N, H, p = i["N"], i["H"], i["probs"]
    small = prefix_graph(i["Hin"], 50)
    p50 = p[: N + 50]
    dec = _decoder("F", "min_sum", probs=p50, graph=small)
    _fer_is(dec, p50, small)
    rp = H.row_ptr[50:71].astype(np.int64)
    dec.append_rows((rp - rp[0]).astype(np.int32), H.col_idx[rp[0] : rp[-1]], N + 70, p[N + 50 :])
    assert (dec.m, dec.n) == (70, 201)
    grown = _fer_is(dec, p, H)
    fresh = _decoder("F", "min_sum")
    _same(grown, fresh.mc_fer_run(RUNS, seed=SEED, first_trial=FIRST, want_errors=True))
    _is_the_law("F", grown, _law("F"))
    dec.close()
    fresh.close()


# ------------------------------------------------------------------------------------------- 5. one handle, many calls
@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("name", ["H2", "F"])
def test_one_handle_many_calls(name, path):
    """130 trials, 5 trials (stale planes in the higher tiles), a decode_batch of 70 words, 130 trials again: every call
    equal to a fresh handle's."""
    law = _law(name)
    words = law["synd"][:70] if name == "F" else law["msg"][:70]
    dec = _decoder(name, "product_sum", path=path)
    got = [_run(dec, name), _run(dec, name, 5, first=FIRST + 40), dec.decode_batch(words, want_llr=True), _run(dec, name)]
    _same(got[0], got[3])
    _is_the_law(name, got[0], law)
    _is_the_law(name, got[1], {k: v[40:45] for k, v in law.items()})
    for step, call in enumerate((lambda h: _run(h, name), lambda h: _run(h, name, 5, first=FIRST + 40),
                                 lambda h: h.decode_batch(words, want_llr=True))):
        fresh = _decoder(name, "product_sum", path=path)
        want = call(fresh)
        fresh.close()
        for k in want:
            assert (want[k] is None and got[step][k] is None) or np.array_equal(want[k], got[step][k], equal_nan=(k == "llr")), (step, k)
    _is_the_decode(dec, name, got[3])
    dec.close()


# ------------------------------------------------------------------------------- 6. device outputs on the caller's stream
def _guarded(torch, rows, row_bytes):
    """A device buffer of rows + 2 rows of GUARD bytes; the output is rows 1 .. rows."""
    buf = torch.full(((rows + 2) * row_bytes,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + row_bytes


def _unguard(buf, rows, row_bytes, dtype, shape):
    a = buf.cpu().numpy()
    assert (a[:row_bytes] == GUARD).all() and (a[(rows + 1) * row_bytes :] == GUARD).all(), "guard row written"
    return a[row_bytes : (rows + 1) * row_bytes].view(dtype).reshape(shape)


@pytest.mark.parametrize("name", ["F", "H2"])
def test_device_outputs_on_the_callers_stream(name):
    import torch

    i = mc_ref.instance(name)
    n, omega = i["H"].n, i["omega"]
    dec = _decoder(name, "min_sum", path="stream")
    host = _run(dec, name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # (the fills are ordered before the call: same stream)
        succ, p_succ = _guarded(torch, RUNS, 1)
        its, p_its = _guarded(torch, RUNS, 4)
        bits, p_bits = _guarded(torch, RUNS, n)
        ys, p_ys = _guarded(torch, RUNS, 4 * omega)
    flags, sp = lib.F_EARLY_EXIT | lib.F_DEVICE_IO, C.c_void_p(stream.cuda_stream)

    def call(out_iters, out_bits, out_y):
        if name == "F":
            return dec._lib.scaldpc_mc_fer_run(dec._h, FIRST, RUNS, SEED, MAX_ITER, lib.BP_MIN_SUM, 1.0, flags, sp, lib.ptr(p_succ),
                                               lib.ptr(out_iters), lib.ptr(out_bits))
        return dec._lib.scaldpc_mc_hqc_run(dec._h, omega, i["eps"], FIRST, RUNS, SEED, MAX_ITER, lib.BP_MIN_SUM, 1.0, flags, sp,
                                           lib.ptr(p_succ), lib.ptr(out_iters), lib.ptr(out_bits), lib.ptr(out_y))

    lib.check(call(p_its, p_bits, p_ys))
    stream.synchronize()
    assert np.array_equal(_unguard(succ, RUNS, 1, np.uint8, (RUNS,)), host["success"])
    assert np.array_equal(_unguard(its, RUNS, 4, np.int32, (RUNS,)), host["iters"])
    assert np.array_equal(_unguard(bits, RUNS, n, np.uint8, (RUNS, n)), host["errors" if name == "F" else "msg"])
    if name == "F":
        assert (ys.cpu().numpy() == GUARD).all()
    else:
        assert np.array_equal(_unguard(ys, RUNS, 4 * omega, np.int32, (RUNS, omega)), host["y"])
    # out_iters = NULL (and no inputs exported): accepted, the same flags
    with torch.cuda.stream(stream):
        succ.fill_(GUARD)
        its.fill_(GUARD)
    lib.check(call(None, None, None))
    stream.synchronize()
    assert np.array_equal(_unguard(succ, RUNS, 1, np.uint8, (RUNS,)), host["success"])
    assert (its.cpu().numpy() == GUARD).all()
    dec.close()


# ----------------------------------------------------------------------------------------------------------- secret and eps edges
@pytest.mark.parametrize("name, omega, eps", [("S7", 7, None), ("S7", 6, None), ("S16", 16, None), ("S499", 256, None),
                                              ("S499", 0, None), ("S499", 0, 0.0)])
def test_secret_edges(name, omega, eps):
    """omega = N (every trial a permutation, most candidates duplicates, the candidate index runs across Philox blocks) with
    R below 4 and below 16; omega = 256, the LDS limit; omega = 0, where no secret kernel runs."""
    dec = _decoder(name, "min_sum")
    how = dict(omega=omega) if eps is None else dict(omega=omega, eps=eps)
    r = _run(dec, name, 70, **how)
    _is_the_law(name, r, mc_ref.hqc_law(name, runs=70, **how))
    assert r["y"].shape == (70, omega) and all(len(set(row)) == omega for row in r["y"].tolist())
    _is_the_decode(dec, name, r)
    if omega == 0 and eps == 0.0:
        assert r["success"].all() and (r["iters"] == 1).all()
    elif omega == 0:
        assert 0 < r["success"].sum() < 70
    dec.close()


def test_a_secret_of_257_positions_is_refused():
    N = mc_ref.instance("S499")["N"]
    dec = _decoder("S499", "min_sum")
    succ, its = np.full(70, GUARD, dtype=np.uint8), np.full(70, -7, dtype=np.int32)
    msg, y = np.full((70, dec.n), GUARD, dtype=np.uint8), np.full((70, 257), -7, dtype=np.int32)
    rc = dec._lib.scaldpc_mc_hqc_run(dec._h, 257, 0.04, FIRST, 70, SEED, MAX_ITER, lib.BP_MIN_SUM, 1.0, lib.F_EARLY_EXIT, None,
                                     lib.ptr(succ), lib.ptr(its), lib.ptr(msg), lib.ptr(y))
    assert rc == lib.EDEGREE and N >= 257
    assert (succ == GUARD).all() and (its == -7).all() and (msg == GUARD).all() and (y == -7).all()
    r = _run(dec, "S499", 70, omega=256)  # ... and the handle goes on
    _is_the_law("S499", r, mc_ref.hqc_law("S499", runs=70, omega=256))
    dec.close()


@pytest.mark.parametrize("method, won", [("min_sum", 58), ("product_sum", 60)])
def test_eps_edges(method, won):
    """H2 with priors built at eps = 1 (LLR -inf on every check column): eps = 1 flips every check, eps = 0 none."""
    name = "H2_eps1"
    N = mc_ref.instance(name)["N"]
    dec = _decoder(name, method)
    one = _run(dec, name, 70)
    _is_the_law(name, one, mc_ref.hqc_law(name, runs=70))
    d = _is_the_decode(dec, name, one)
    _is_the_oracle_sample(name, method, one, d)
    if method == "min_sum":
        assert int(one["success"].sum()) == won
    assert 0 < one["success"].sum() < 70
    zero = _run(dec, name, 70, eps=0.0)
    _is_the_law(name, zero, mc_ref.hqc_law(name, runs=70, eps=0.0))
    assert np.array_equal(zero["y"], one["y"]) and np.array_equal(zero["msg"][:, N:], one["msg"][:, N:] ^ 1)
    _is_the_decode(dec, name, zero)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def _raw(dec, entry, out, first=FIRST, batch=70, method=lib.BP_MIN_SUM, alpha=1.0, flags=lib.F_EARLY_EXIT, omega=4, eps=0.06,
         no_success=False):
    succ = None if no_success else lib.ptr(out["success"])
    if entry == "fer":
        return dec._lib.scaldpc_mc_fer_run(dec._h, first, batch, SEED, MAX_ITER, method, alpha, flags, None, succ,
                                           lib.ptr(out["iters"]), lib.ptr(out["bits"]))
    return dec._lib.scaldpc_mc_hqc_run(dec._h, omega, eps, first, batch, SEED, MAX_ITER, method, alpha, flags, None, succ,
                                       lib.ptr(out["iters"]), lib.ptr(out["bits"]), lib.ptr(out["y"]))


BOTH = {"batch 0": dict(batch=0), "batch -1": dict(batch=-1), "unknown method": dict(method=2), "alpha NaN": dict(alpha=float("nan")),
        "out_success NULL": dict(no_success=True), "first_trial -1": dict(first=-1), "unknown flag": dict(flags=lib.F_EARLY_EXIT | 8),
        "the asynchronous flag": dict(flags=lib.F_EARLY_EXIT | lib.F_ASYNC)}
HQC_ONLY = {"omega -1": dict(omega=-1), "omega N + 1": dict(omega=132), "eps -0.1": dict(eps=-0.1), "eps 1.1": dict(eps=1.1),
            "eps NaN": dict(eps=float("nan"))}


@pytest.mark.parametrize("entry", ["fer", "hqc"])
def test_refusals(entry):
    """Each refusal is SCALDPC_EINVAL, writes to no output, and leaves the handle as a fresh one."""
    name = "F" if entry == "fer" else "H2"
    assert mc_ref.instance("H2")["N"] == 131
    dec, fresh = _decoder(name, "min_sum"), _decoder(name, "min_sum")
    want = _run(fresh, name, 70)
    fresh.close()
    out = dict(success=np.full(70, GUARD, dtype=np.uint8), iters=np.full(70, -7, dtype=np.int32),
               bits=np.full((70, dec.n), GUARD, dtype=np.uint8), y=np.full((70, 4), -7, dtype=np.int32))
    assert _raw(dec, entry, out) == lib.OK  # (the call that the cases below each change in one argument is a valid one)
    for k in ("success", "iters"):
        assert np.array_equal(out[k], want[k]), k
    for case, change in dict(BOTH, **(HQC_ONLY if entry == "hqc" else {})).items():
        for k, v in out.items():
            v.fill(GUARD if v.dtype == np.uint8 else -7)
        rc = _raw(dec, entry, out, **change)
        assert rc == lib.EINVAL, (case, rc)
        assert dec._lib.scaldpc_last_error(), case
        for k, v in out.items():
            assert (v == (GUARD if v.dtype == np.uint8 else -7)).all(), (case, k)
        _same(_run(dec, name, 70), want)
    dec.close()
