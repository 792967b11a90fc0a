"""Monte-Carlo sweeps on chosen trials on the GPU: the six scaldpc_mc_*_at entries, their Python methods and the two drivers.

Held to the DEFINING PROPERTY (include/scaldpc.h): every output row i of an _at call on a list equals row trial_ids[i] - f of the
sibling's contiguous call from f, on the same handle with the same settings -- integer equality on every path (LDS-resident,
64-codeword tiles with a compact pass, row-parallel, the float64 hand-over) and in every q-ary kernel form -- and to the NumPy
trial laws of tests/mc_ref.py and tests/hqc_soft_mc_ref.py evaluated per index.  The list (tests/mc_trial_list_cases.py) is
shuffled, holds a duplicate, both ends of the window and both sides of a tile boundary, fills one tile and a ragged one, and
its window crosses 2^32; tests/test_mc_trial_list.py pins what makes it hard enough from the CPU oracle alone."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hqc_soft_mc_ref
import hqc_stats_cases
import mc_ref
import ref64_mc_cases
from mc_ref import FIRST, MAX_ITER, RUNS, SEED
from mc_trial_list_cases import FAR, IDS, OFFSETS, PREFIXES, rows, same
from test_hqc_stats_gpu import FromFirst
from test_qary_mc_gpu import RUNS4, SEED4, W4, config4_case, special_case
from test_qary_secret_mc_gpu import FIRST1, RUNS1, case1

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
qary = importlib.import_module("sca-ldpc_amd.qary")
driver = importlib.import_module("sca-ldpc_amd.driver")
lib = importlib.import_module("sca-ldpc_amd._lib")

METHODS = ["min_sum", "product_sum"]
PATHS = [("auto", IDS.size), ("stream", IDS.size), ("edge", 5)]  # the three of tests/test_mc_edges_gpu.py
FAMILIES = [("F", "fer"), ("H1", "hqc"), ("H2", "hqc"), ("H1", "soft"), ("H2", "soft")]
GUARD = 0xA5
T9 = ref64_mc_cases.t9  # nine outcomes, with costs


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER", "SCALDPC_SPLIT", "SCALDPC_PRECISION"):
        monkeypatch.delenv(v, raising=False)


def _decoder(name, method, cls=None, **knobs):
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):  # (p = 0 and p = 1 among F's priors)
        dec = (cls or bp.BpDecoder)(i["H"], max_iter=MAX_ITER, bp_method=method, channel_probs=i["probs"])
    if knobs:
        dec.configure(**knobs)
    return dec


def _range(dec, name, family, runs=RUNS, first=FIRST, **kw):
    """The sibling's contiguous call, every input exported."""
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):
        if family == "fer":
            return dec.mc_fer_run(runs, SEED, first_trial=first, want_errors=True, **kw)
        if family == "hqc":
            return dec.mc_hqc_run(runs, i["omega"], i["eps"], SEED, first_trial=first, want_inputs=True, want_stats=True, want_bits=True, **kw)
        return dec.mc_hqc_run_soft(runs, i["omega"], T9(), SEED, first_trial=first, want_inputs=True, want_stats=True, want_bits=True, **kw)


def _at(dec, name, family, ids=IDS, **kw):
    """The list call, every input exported."""
    i = mc_ref.instance(name)
    with np.errstate(divide="ignore"):
        if family == "fer":
            return dec.mc_fer_run_at(ids, SEED, want_errors=True, **kw)
        if family == "hqc":
            return dec.mc_hqc_run_at(ids, i["omega"], i["eps"], SEED, want_inputs=True, want_stats=True, want_bits=True, **kw)
        return dec.mc_hqc_run_soft_at(ids, i["omega"], T9(), SEED, want_inputs=True, want_stats=True, want_bits=True, **kw)


def _law(name, family, first=FIRST, runs=RUNS):
    """The exported inputs of trials first .. first + runs - 1 by the NumPy laws."""
    i = mc_ref.instance(name)
    if family == "fer":
        return dict(errors=mc_ref.fer(SEED, first, runs, i["H"], i["probs"])[0])
    if family == "hqc":
        y, msg = mc_ref.hqc(SEED, first, runs, i["Hin"], i["omega"], i["eps"])
        return dict(y=y, msg=msg)
    d = hqc_soft_mc_ref.draw(SEED, first, runs, i["Hin"], i["omega"], T9())
    return {k: d[k] for k in ("y", "outcome", "msg", "flips", "cost")}


# ------------------------------------------------------------------------------- 1. the defining property, family x path x setting
@pytest.mark.parametrize("early", [True, False], ids=["early", "fixed"])
@pytest.mark.parametrize("path, slots", PATHS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name, family", FAMILIES)
def test_defining_property(name, family, method, path, slots, early):
    knobs = dict(path=path, compact_after=4) if path == "stream" else dict(path=path)
    dec = _decoder(name, method, **knobs)
    ids, at = IDS[:slots], OFFSETS[:slots]
    if path == "edge":  # the row-parallel kernels take a handful of codewords: the sibling, five trials at a time
        parts = [_range(dec, name, family, 5, FIRST + f, early_exit=early) for f in range(0, RUNS, 5)]
        assert dec.last_stats()["row_parallel"] == 5
        whole = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in parts[0]}
    else:
        whole = _range(dec, name, family, early_exit=early)
    got = _at(dec, name, family, ids, early_exit=early)
    assert dec.last_stats()["row_parallel"] == (slots if path == "edge" else 0)
    if path == "stream" and early:
        print(f"{name} {family} {method}: compacted {dec.last_compacted()} of {slots}")
        # the list's stragglers went through the compact pass, a ragged tile of them (tests/test_mc_trial_list.py pins from the
        # CPU oracle that every family and method leaves some)
        assert 0 < dec.last_compacted() < slots
    same(got, rows(whole, at), f"{name} {family} {method} {path}")
    assert all(v is not None for v in got.values()) and len(got["success"]) == slots
    if slots == IDS.size:
        assert 0 < got["success"].sum() < slots
        if early:
            assert len(set(got["iters"].tolist())) >= 2
        else:
            assert (got["iters"] == MAX_ITER).all()
        dup = [100, 101]  # the duplicate: two slots with the same index give the same row
        for k, v in got.items():
            assert np.array_equal(v[dup[0]], v[dup[1]]), k
    dec.close()


# --------------------------------------------------------------------------------------- 2. the exported inputs against the law
@pytest.mark.parametrize("name, family", FAMILIES)
def test_exported_inputs_are_the_law_per_index(name, family):
    dec = _decoder(name, "min_sum")
    got, law = _at(dec, name, family), _law(name, family)
    for k, v in law.items():
        assert np.array_equal(got[k], v[OFFSETS]), k
    far = _at(dec, name, family, FAR)
    for slot, index in enumerate(FAR.tolist()):
        one = _law(name, family, index, 1)
        for k, v in one.items():
            assert np.array_equal(far[k][slot], v[0]), (index, k)
        same({k: v[slot : slot + 1] for k, v in far.items()}, _range(dec, name, family, 1, index), f"batch 1 at {index}")
    key = "errors" if family == "fer" else "y"
    assert len({far[key][s].tobytes() for s in range(3)}) == 3  # the high counter word is in the counter
    dec.close()


# ---------------------------------------------------------------------------------------------------------- 3. prefixes and splits
@pytest.mark.parametrize("path", ["auto", "stream"])
@pytest.mark.parametrize("name, family", [("F", "fer"), ("H2", "soft")])
def test_prefixes_and_a_split(name, family, path):
    dec = _decoder(name, "product_sum", path=path)
    whole = _at(dec, name, family)
    for n in PREFIXES:
        same(_at(dec, name, family, IDS[:n]), rows(whole, slice(0, n)), f"prefix {n}")
    a, b = _at(dec, name, family, IDS[:41]), _at(dec, name, family, IDS[41:])
    same({k: np.concatenate([a[k], b[k]]) for k in whole}, whole, "41 + 65")
    same(_at(dec, name, family, IDS.tolist()), whole, "a Python list")
    same(_at(dec, name, family, IDS.astype(np.uint64)), whole, "uint64")
    dec.close()


# ------------------------------------------------------------------------------------------------------------------- 4. float64
def _oracle64(name, soft):
    return ref64_mc_cases.soft_oracle(name) if soft else ref64_mc_cases.shared_oracle(name)


@pytest.mark.parametrize("name, family", [("F", "fer"), ("H1", "soft"), ("H2", "soft")])
def test_float64_rows_and_the_hand_over(name, family):
    """precision="float64" on the cases of tests/ref64_mc_cases.py: the rows of the contiguous _f64 call, the float64 oracle's
    iteration counts, and a hand-over of exactly the listed trials the oracle says still run after `compact_after`."""
    dec = _decoder(name, "product_sum", compact_after=4)
    whole = _range(dec, name, family, precision="float64")
    assert dec.last_compacted() == ref64_mc_cases.handed_over(name, family == "soft", 4)
    got = _at(dec, name, family, precision="float64")
    d = _oracle64(name, family == "soft")
    listed = int(((d["iters"] > 4) | (d["converged"] == 0))[OFFSETS].sum())
    assert dec.last_compacted() == listed > 0
    same(got, rows(whole), f"{name} {family} float64")
    assert np.array_equal(got["iters"], d["iters"][OFFSETS]) and np.array_equal(got["success"], d["success"][OFFSETS])
    fixed = _at(dec, name, family, precision="float64", early_exit=False)
    same(fixed, rows(_range(dec, name, family, precision="float64", early_exit=False)), "fixed iterations")
    assert dec.last_compacted() == 0 and (fixed["iters"] == MAX_ITER).all()
    # the trial does not know the decode's precision
    fp32 = _at(dec, name, family)
    for k in ("errors", "msg", "y", "outcome", "flips", "cost"):
        if k in got:
            assert np.array_equal(got[k], fp32[k]), k
    # ... and sweeps_in("float64") hands its default to the list methods
    sw = _decoder(name, "product_sum", cls=driver.sweeps_in("float64"), compact_after=4)
    same(_at(sw, name, family), got, "sweeps_in")
    sw.close()
    dec.close()


# --------------------------------------------------------------------------------------------------------------------- 5. q-ary
OFF70 = np.concatenate([np.random.RandomState(7).permutation(70)[:60], [7, 7, 69, 0, 64, 63]]).astype(np.int64)  # 66 slots of 70 trials
ALL = dict(want_levels=True, want_symbols=True)


@pytest.mark.parametrize("knobs", [dict(), dict(dp=0), dict(wave=0, unroll=0), dict(wave=1, unroll=0), dict(var_small=0), dict(llr_tiled=0)],
                         ids=["default", "dp0", "wave0", "wave1", "var_small0", "llr_tiled0"])
def test_qary_plain_decoder_in_every_kernel_form(knobs):
    H, pmf, lv, sym = config4_case()
    first = 2**32 - 30
    dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, 5)
    if knobs:
        dec.configure(**knobs)
    whole = dec.mc_run(RUNS, SEED4, pmf, W4, first_trial=first, **ALL)
    got = dec.mc_run_at(first + OFFSETS, SEED4, pmf, W4, **ALL)
    same(got, rows(whole), str(knobs))
    assert 0 < got["success"].sum() < OFFSETS.size
    same(dec.mc_run_at(first + OFFSETS, SEED4, pmf, W4), {k: got[k] for k in ("success", "errs", "wrong")}, "results only")
    far = dec.mc_run_at(FAR, SEED4, pmf, W4, **ALL)
    for slot, index in enumerate(FAR.tolist()):
        same({k: v[slot : slot + 1] for k, v in far.items()}, dec.mc_run(1, SEED4, pmf, W4, first_trial=index, **ALL), f"batch 1 at {index}")
    dec.close()


def test_qary_special_decoder_in_every_kernel_form():
    H, lb, ls, wb, ws, seed, first, batch, lv, sym = special_case()
    dec = qary.decoder_class("DecoderN80R32SW3")(H, 4)
    for kn in (dict(), dict(wave=0), dict(dp_any=1), dict(var_small=0, llr_tiled=0)):
        if kn:
            dec.configure(**kn)
        whole = dec.mc_run(batch, seed, lb, wb, ls, ws, first_trial=first, **ALL)
        got = dec.mc_run_at(first + OFF70, seed, lb, wb, ls, ws, **ALL)
        same(got, rows(whole, OFF70), str(kn))
        assert np.array_equal(got["levels"], lv[OFF70]) and np.array_equal(got["symbols"], sym[OFF70])
    dec.close()


def test_qary_secret_in_every_kernel_form():
    c, secret, levels, sym = case1()
    every = dict(want_secret=True, want_levels=True, want_symbols=True)
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    for kn in (dict(), dict(wave=0), dict(dp_any=1), dict(var_small=0, llr_tiled=0)):
        if kn:
            dec.configure(**kn)
        whole = c.run(dec, RUNS1, FIRST1)
        got = dec.mc_run_secret_at(FIRST1 + OFF70, c.seed, c.prior, c.lb, c.wb, c.ls, c.ws, **every)
        same(got, rows(whole, OFF70), str(kn))
        assert np.array_equal(got["secret"], secret[OFF70]) and np.array_equal(got["levels"], levels[OFF70])
        assert np.array_equal(got["symbols"], sym[OFF70])
    assert 0 < got["success"].sum() < OFF70.size
    far = dec.mc_run_secret_at(FAR, c.seed, c.prior, c.lb, c.wb, c.ls, c.ws, **every)
    for slot, index in enumerate(FAR.tolist()):
        same({k: v[slot : slot + 1] for k, v in far.items()}, c.run(dec, 1, index), f"batch 1 at {index}")
    dec.close()


def test_qary_device_pointers_against_the_host_call():
    import torch

    c, _, _, _ = case1()
    ids = FIRST1 + OFF70
    n, N = ids.size, c.N
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    host = dec.mc_run_secret_at(ids, c.seed, c.prior, c.lb, c.wb, c.ls, c.ws, want_secret=True, want_levels=True, want_symbols=True)
    t = dict(success=torch.zeros(n, dtype=torch.uint8, device="cuda"), wrong=torch.zeros((n, 2), dtype=torch.int32, device="cuda"),
             channel_wrong=torch.zeros((n, 2), dtype=torch.int32, device="cuda"), secret=torch.zeros((n, N), dtype=torch.int8, device="cuda"),
             levels=torch.zeros((n, N), dtype=torch.uint8, device="cuda"), symbols=torch.zeros((n, N), dtype=torch.int8, device="cuda"))
    torch.cuda.synchronize()
    dec.mc_run_secret_at_device(ids, c.seed, c.prior, c.lb, c.wb, c.ls, c.ws, *(t[k].data_ptr() for k in
                                ("success", "wrong", "channel_wrong", "secret", "levels", "symbols")))
    same({k: v.cpu().numpy() for k, v in t.items()}, host, "secret, device pointers")
    H, lb, ls, wb, ws, seed, first, batch, lv, sym = special_case()
    host = dec.mc_run_at(first + OFF70, seed, lb, wb, ls, ws, **ALL)
    u = dict(success=t["success"], errs=torch.zeros(n, dtype=torch.int32, device="cuda"), wrong=torch.zeros(n, dtype=torch.int32, device="cuda"),
             levels=t["levels"], symbols=t["symbols"])
    torch.cuda.synchronize()
    dec.mc_run_at_device(first + OFF70, seed, lb, wb, ls, ws, *(u[k].data_ptr() for k in ("success", "errs", "wrong", "levels", "symbols")))
    same({k: v.cpu().numpy() for k, v in u.items()}, host, "levels, device pointers")
    dec.close()


# ----------------------------------------------------------------------------------------------- 6. refusals through the C ABI
def _outs(n, cols, omega, R):
    return dict(success=np.full(n, GUARD, dtype=np.uint8), iters=np.full(n, -7, dtype=np.int32), bits_in=np.full((n, cols), GUARD, dtype=np.uint8),
                y=np.full((n, max(omega, 1)), -7, dtype=np.int32), outcome=np.full((n, R), GUARD, dtype=np.uint8),
                flips=np.full(n, -7, dtype=np.int32), cost=np.full(n, -7, dtype=np.int32), stats=np.full((n, 5), -7, dtype=np.int32),
                bits=np.full((n, cols), GUARD, dtype=np.uint8))


def _intact(out):
    return all((v == (GUARD if v.dtype == np.uint8 else -7)).all() for v in out.values())


def _raw_bp(dec, entry, out, ids, batch=None, method=lib.BP_MIN_SUM, alpha=1.0, flags=lib.F_EARLY_EXIT, omega=None, table=None,
            no_success=False, no_list=False):
    """scaldpc_mc_fer_run_at / _at_f64 (entry "fer" / "fer64"), scaldpc_mc_hqc_run_stats_at / _at_f64 ("soft" / "soft64")."""
    f64 = entry.endswith("64")
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    head = (dec._h,)
    tail = (None if no_list else lib.ptr(ids), len(ids) if batch is None else batch, SEED, MAX_ITER) + (() if f64 else (method, alpha)) + (
        flags, None, None if no_success else lib.ptr(out["success"]), lib.ptr(out["iters"]))
    if entry.startswith("fer"):
        fn = dec._lib.scaldpc_mc_fer_run_at_f64 if f64 else dec._lib.scaldpc_mc_fer_run_at
        return fn(*head, *tail, lib.ptr(out["bits_in"]))
    t = dict(T9(), **(table or {}))
    w = np.ascontiguousarray(t["weights"], dtype=np.float64)
    fl = np.ascontiguousarray(t["flips"], dtype=np.uint8)
    pr = np.ascontiguousarray(t["probs"], dtype=np.float64 if f64 else np.float32)
    cs = np.ascontiguousarray(t["costs"], dtype=np.int32)
    fn = dec._lib.scaldpc_mc_hqc_run_stats_at_f64 if f64 else dec._lib.scaldpc_mc_hqc_run_stats_at
    return fn(*head, mc_ref.instance("H2")["omega"] if omega is None else omega, lib.ptr(w), lib.ptr(fl), lib.ptr(pr), lib.ptr(cs),
              w.shape[1], *tail, lib.ptr(out["bits_in"]), lib.ptr(out["y"]), lib.ptr(out["outcome"]), lib.ptr(out["flips"]),
              lib.ptr(out["cost"]), lib.ptr(out["stats"]), lib.ptr(out["bits"]))


def _bad_list(pos, value, n=70):
    ids = (FIRST + np.arange(n)).astype(np.int64)
    ids[pos] = value
    return ids


SIBLINGS_REFUSE = {"batch 0": dict(batch=0), "batch -1": dict(batch=-1), "out_success NULL": dict(no_success=True),
                   "unknown flag": dict(flags=lib.F_EARLY_EXIT | 8), "the asynchronous flag": dict(flags=lib.F_EARLY_EXIT | lib.F_ASYNC)}
FP32_ONLY = {"unknown method": dict(method=2), "alpha NaN": dict(alpha=float("nan"))}
SOFT_ONLY = {"omega -1": dict(omega=-1), "omega N + 1": dict(omega=132), "a weight that is no probability": dict(table=dict(
    weights=np.array([[1.5] + [0.0] * 8, [1.0] + [0.0] * 8]))), "flips 2": dict(table=dict(flips=np.array([2] + [0] * 8))),
    "probs 1.5": dict(table=dict(probs=np.array([1.5] + [0.1] * 8)))}


@pytest.mark.parametrize("entry", ["fer", "soft", "fer64", "soft64"])
def test_refusals_of_the_binary_entries(entry):
    """SCALDPC_EINVAL before anything is queued: every guard byte intact, the handle as good as new, nothing left behind."""
    name, family = ("F", "fer") if entry.startswith("fer") else ("H2", "soft")
    precision = dict(precision="float64") if entry.endswith("64") else {}
    method = "product_sum" if entry.endswith("64") else "min_sum"
    before = lib.live_blocks()
    fresh = _decoder(name, method)
    want = _range(fresh, name, family, 70, **precision)
    fresh.close()
    dec = _decoder(name, method)
    i = mc_ref.instance(name)
    out = _outs(70, dec.n, i["omega"], dec.m)
    good = (FIRST + np.arange(70)).astype(np.int64)
    raw = dict(method=lib.BP_PRODUCT_SUM) if method == "product_sum" else {}
    assert _raw_bp(dec, entry, out, good, **raw) == lib.OK  # the call that every case below changes in one argument is valid
    assert np.array_equal(out["success"], want["success"]) and np.array_equal(out["iters"], want["iters"])
    assert lib.live_blocks()["device_blocks"] > before["device_blocks"]
    cases = {"trial_ids NULL": (dict(no_list=True), "trial_ids is NULL"),
             "a negative index at 0": (dict(ids=_bad_list(0, -1)), r"trial_ids[0] = -1 is negative"),
             "a negative index at 65": (dict(ids=_bad_list(65, -(2**40))), f"trial_ids[65] = {-(2**40)} is negative"),
             "a negative index in the last slot": (dict(ids=_bad_list(69, -(2**63))), f"trial_ids[69] = {-(2**63)} is negative")}
    cases.update({k: (v, None) for k, v in SIBLINGS_REFUSE.items()})
    if not entry.endswith("64"):
        cases.update({k: (v, None) for k, v in FP32_ONLY.items()})
    if entry.startswith("soft"):
        cases.update({k: (v, None) for k, v in SOFT_ONLY.items()})
    for case, (change, message) in cases.items():
        for v in out.values():
            v.fill(GUARD if v.dtype == np.uint8 else -7)
        rc = _raw_bp(dec, entry, out, **dict(dict(ids=good, **raw), **change))
        assert rc == lib.EINVAL, (case, rc)
        said = dec._lib.scaldpc_last_error().decode()
        assert said and (message is None or message in said), (case, said)
        assert _intact(out), case
        same(_range(dec, name, family, 70, **precision), want, f"the handle after {case}")
    same(_at(dec, name, family, good, **precision), want, "the list call after the refusals")
    dec.close()
    after = lib.live_blocks()
    for k in ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes"):
        assert after[k] == before[k], k


@pytest.mark.parametrize("entry", ["fer", "soft", "fer64", "soft64"])
def test_binary_device_pointers_against_the_host_call(entry):
    """SCALDPC_F_DEVICE_IO on the four binary list entries with every optional output asked for: each device array holds what
    the host-pointer call of the same entry returns (106 slots: a full tile and a ragged one), and an entry writes only its own."""
    import torch

    name = "F" if entry.startswith("fer") else "H2"
    dec = _decoder(name, "product_sum")
    raw = dict(method=lib.BP_PRODUCT_SUM)
    host = _outs(IDS.size, dec.n, mc_ref.instance(name)["omega"], dec.m)
    written = ("success", "iters", "bits_in") if entry.startswith("fer") else tuple(host)
    assert _raw_bp(dec, entry, host, IDS, **raw) == lib.OK
    assert not any(_intact({k: host[k]}) for k in written) and _intact({k: v for k, v in host.items() if k not in written})
    dev = {k: torch.from_numpy(v).cuda() for k, v in _outs(IDS.size, dec.n, mc_ref.instance(name)["omega"], dec.m).items()}
    torch.cuda.synchronize()  # stream = NULL means the handle's own stream: order it after torch's copies
    assert _raw_bp(dec, entry, {k: v.data_ptr() for k, v in dev.items()}, IDS, flags=lib.F_EARLY_EXIT | lib.F_DEVICE_IO, **raw) == lib.OK
    same({k: v.cpu().numpy() for k, v in dev.items()}, host, f"{entry}, device pointers")
    dec.close()


@pytest.mark.parametrize("entry", ["levels", "secret"])
def test_refusals_of_the_qary_entries(entry):
    c, _, _, _ = case1()
    H, lb, ls, wb, ws, seed, first, batch, lv, sym = special_case()
    before = lib.live_blocks()
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    n, N = 70, c.N
    good = (FIRST1 + np.arange(n)).astype(np.int64)
    out = dict(success=np.full(n, GUARD, dtype=np.uint8), a=np.full((n, 2), -7, dtype=np.int32), b=np.full((n, 2), -7, dtype=np.int32),
               secret=np.full((n, N), GUARD, dtype=np.uint8), levels=np.full((n, N), GUARD, dtype=np.uint8),
               symbols=np.full((n, N), GUARD, dtype=np.uint8))
    wbq, wsq = np.ascontiguousarray(wb, dtype=np.float64), np.ascontiguousarray(ws, dtype=np.float64)
    prior, cwb, cws = (np.ascontiguousarray(x, dtype=np.float64) for x in (c.prior, c.wb, c.ws))

    def call(ids=good, batch=None, flags=0, no_list=False, no_success=False, h=dec._h, t=None):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        mid = (None if no_list else lib.ptr(ids), len(ids) if batch is None else batch, seed, flags, None,
               None if no_success else lib.ptr(out["success"]))
        if entry == "levels":
            t = dict(dict(lb=lb, wb=wbq, kb=2, ls=ls, ws=wsq, ks=3), **(t or {}))
            return dec._lib.scaldpc_mc_qary_run_at(h, lib.ptr(t["lb"]), lib.ptr(t["wb"]), t["kb"], lib.ptr(t["ls"]), lib.ptr(t["ws"]), t["ks"],
                                                   *mid, lib.ptr(out["a"]), lib.ptr(out["b"]), lib.ptr(out["levels"]), lib.ptr(out["symbols"]))
        t = dict(dict(prior=prior, lb=c.lb, wb=cwb, kb=c.lb.shape[0], ls=c.ls, ws=cws, ks=c.ls.shape[0]), **(t or {}))
        return dec._lib.scaldpc_mc_qary_run_secret_at(h, lib.ptr(t["prior"]), lib.ptr(t["lb"]), lib.ptr(t["wb"]), t["kb"], lib.ptr(t["ls"]),
                                                      lib.ptr(t["ws"]), t["ks"], *mid, lib.ptr(out["a"]), lib.ptr(out["b"]),
                                                      lib.ptr(out["secret"]), lib.ptr(out["levels"]), lib.ptr(out["symbols"]))

    def changed(a, where, value):
        a = np.array(a, copy=True)
        a[where] = value
        return a

    def contiguous():
        if entry == "levels":
            return dec.mc_run(n, seed, lb, wb, ls, ws, first_trial=FIRST1, **ALL)
        return c.run(dec, n, FIRST1)

    want = contiguous()
    assert call() == lib.OK and np.array_equal(out["success"], want["success"])
    assert np.array_equal(out["levels"], want["levels"]) and np.array_equal(out["symbols"].view(np.int8), want["symbols"])
    assert lib.live_blocks()["device_blocks"] > before["device_blocks"]
    cases = {"trial_ids NULL": (dict(no_list=True), "trial_ids is NULL"),
             "a negative index at 3": (dict(ids=np.where(np.arange(n) == 3, -5, good)), "trial_ids[3] = -5 is negative"),
             "a negative index in the last slot": (dict(ids=_bad_list(69, -(2**63))), f"trial_ids[69] = {-(2**63)} is negative"),
             "batch 0": (dict(batch=0), None), "batch -1": (dict(batch=-1), None), "out_success NULL": (dict(no_success=True), None),
             "the asynchronous flag": (dict(flags=lib.F_DEVICE_IO | lib.F_ASYNC), None), "no handle": (dict(h=None), None)}
    # the sibling's table refusals (tests/test_qary_mc_gpu.py, tests/test_qary_secret_mc_gpu.py): the code each of them gets there
    tables = {"levels_b NULL": (dict(lb=None), lib.EINVAL, None), "weights_s NULL": (dict(ws=None), lib.EINVAL, None),
              "k_b 0": (dict(kb=0), lib.EINVAL, None), "k_s 0": (dict(ks=0), lib.EINVAL, None)}
    if entry == "levels":
        tables.update({"a weight that is no probability": (dict(wb=np.array([-0.1, 1.1])), lib.EINVAL, "levels_b"),
                       "weights that sum to 0.9": (dict(ws=np.array([0.5, 0.3, 0.1])), lib.EINVAL, "levels_s"),
                       "17 levels": (dict(kb=17, lb=np.tile(lb, (9, 1)), wb=np.full(17, 1 / 17)), lib.EINVAL, None),
                       "a level that is no pmf": (dict(lb=changed(lb, 1, lb[1] * 0.9)), lib.EPMF, "level 1"),
                       "a level of NaN": (dict(ls=changed(ls, 2, np.nan)), lib.EPMF, "level 2")})
    else:
        tables.update({"prior_b NULL": (dict(prior=None), lib.EINVAL, None),
                       "a prior that is no pmf": (dict(prior=np.array([-0.1, 0.5, 0.6, 0.0, 0.0])), lib.EINVAL, "prior_b"),
                       "a weight of 1.5": (dict(wb=changed(cwb, (3, 0), 1.5)), lib.EINVAL, "weights_b[3]"),
                       "a row of weights off by 2e-6": (dict(ws=changed(cws, (12, 0), cws[12, 0] + 2e-6)), lib.EINVAL, "weights_s[12]"),
                       "a level that is no pmf": (dict(lb=changed(c.lb, 1, c.lb[1] * 0.9)), lib.EPMF, "level 1"),
                       "a level of NaN": (dict(ls=changed(c.ls, 2, np.nan)), lib.EPMF, "level 2")})
    cases = {k: (v, lib.EINVAL, m) for k, (v, m) in cases.items()}
    cases.update({k: (dict(t=v), code, m) for k, (v, code, m) in tables.items()})
    for case, (change, code, message) in cases.items():
        for v in out.values():
            v.fill(GUARD if v.dtype == np.uint8 else -7)
        rc = call(**change)
        assert rc == code, (case, rc)
        said = dec._lib.scaldpc_last_error().decode()
        assert said and (message is None or message in said), (case, said)
        assert _intact(out), case
        same(contiguous(), want, f"the handle after {case}")
    dec.close()
    after = lib.live_blocks()
    for k in ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes"):
        assert after[k] == before[k], k


# ----------------------------------------------------------------------------------------------- 7. the drivers on the HIP class
class FromFirstAt(FromFirst):
    """The drivers count trials from 0; the oracle's table is of trials FIRST .. FIRST + RUNS - 1 of tests/hqc_stats_cases.py."""

    def mc_hqc_run_soft_at(self, trial_ids, *args, **kw):
        return super().mc_hqc_run_soft_at(np.asarray(trial_ids, dtype=np.int64) + hqc_stats_cases.FIRST, *args, **kw)


@pytest.mark.parametrize("chunk", [4096, 70])
def test_the_retiring_curve_is_the_curve(chunk):
    """driver.hqc_attack_curve_retiring on the curve case of tests/test_hqc_stats_gpu.py: the four fields of hqc_attack_curve."""
    k = hqc_stats_cases
    sup, rws = k.code()
    args = (sup, k.N, rws, k.OMEGA, k.wrapped_table(), k.RUNS, k.SEED, k.STEP)
    how = dict(chunk=chunk, bp_method="min_sum", max_iter=k.MAX_ITER, bp_decoder=FromFirstAt)
    whole, got = driver.hqc_attack_curve(*args, **how), driver.hqc_attack_curve_retiring(*args, **how)
    for f in ("steps", "checks_needed", "oracle_calls_needed"):
        assert np.array_equal(got[f], whole[f]), f
    assert got["decoder_stats"] == whole["decoder_stats"]
    need = got["checks_needed"]
    assert np.array_equal(need, k.checks_needed())
    assert got["successes"].tolist() == [int((need == r).sum()) for r in k.STEPS] == [1, 13, 105, 58]
    assert got["decoded"].tolist() == [int(((need == -1) | (need >= r)).sum()) for r in k.STEPS] == [200, 199, 186, 81]


def test_the_retiring_curve_in_float64():
    """... and with bp_decoder=sweeps_in("float64"), on H2's rows ten at a time (tests/test_ref64_mc_gpu.py's curve)."""
    c = ref64_mc_cases
    sup, rws = c.h2_code()
    i = mc_ref.instance("H2")

    class At(bp.BpDecoder):
        def mc_hqc_run_soft(self, runs, omega, table, seed, first_trial=0, **kw):
            return super().mc_hqc_run_soft(runs, omega, table, seed, first_trial=FIRST + first_trial, **kw)

        def mc_hqc_run_soft_at(self, trial_ids, *args, **kw):
            return super().mc_hqc_run_soft_at(np.asarray(trial_ids, dtype=np.int64) + FIRST, *args, **kw)

    args = (sup, i["N"], rws, i["omega"], c.t9(), RUNS, SEED, c.CURVE_STEP)
    how = dict(chunk=50, max_iter=MAX_ITER, bp_decoder=driver.sweeps_in("float64", bp_decoder=At))
    whole, got = driver.hqc_attack_curve(*args, **how), driver.hqc_attack_curve_retiring(*args, **how)
    need, _ = c.curve_key()
    assert np.array_equal(got["checks_needed"], need) and np.array_equal(whole["checks_needed"], need)
    for f in ("steps", "oracle_calls_needed"):
        assert np.array_equal(got[f], whole[f]), f
    assert got["decoder_stats"] == whole["decoder_stats"]
    assert got["decoded"].tolist() == [int(((need == -1) | (need >= r)).sum()) for r in c.CURVE_STEPS]


@pytest.mark.parametrize("precision", [None, "float64"])
def test_the_replay_of_a_sweeps_failures(precision):
    """driver.hqc_replay on the failed trials of one H2 sweep: the sweep's own rows for them, and a decode_batch on what it
    exported that decodes the same words in the same number of iterations."""
    i = mc_ref.instance("H2")
    kw = {} if precision is None else dict(precision=precision)
    shared = np.concatenate([np.full(i["N"], i["omega"] / i["N"]), np.full(i["R"], 0.5)])  # the driver's decoder
    dec = bp.BpDecoder(i["H"], max_iter=MAX_ITER, bp_method="product_sum", channel_probs=shared)
    with np.errstate(divide="ignore"):
        sweep = dec.mc_hqc_run_soft(RUNS, i["omega"], T9(), SEED, first_trial=FIRST, want_inputs=True, want_stats=True, want_bits=True, **kw)
    dec.close()
    failed = FIRST + np.flatnonzero(sweep["success"] == 0)
    assert 0 < failed.size < RUNS
    got = driver.hqc_replay(i["Hin"], i["N"], i["omega"], T9(), failed, SEED, max_iter=MAX_ITER, **kw)
    assert np.array_equal(got["trial_ids"], failed)
    same(got["sweep"], rows(sweep, failed - FIRST), "the sweep's rows")
    assert not got["sweep"]["success"].any()
    d = got["decode"]
    assert np.array_equal(d["bits"], got["sweep"]["bits"]) and np.array_equal(d["iters"], got["sweep"]["iters"])
    assert d["llr"].shape == (failed.size, i["N"] + i["R"]) and d["llr"].dtype == (np.float64 if precision == "float64" else np.float32)
    assert np.array_equal(mc_ref.hqc_success(d["bits"], got["sweep"]["y"], i["N"]), got["sweep"]["success"])
