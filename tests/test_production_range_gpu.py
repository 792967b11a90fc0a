"""The binary BP kernels across the production range of graph SHAPES, at full size and on a live decoder.

Which kernels run is decided by the graph: min-sum keeps its record form only while no column has more than 32 edges,
the variable kernels come in 16 / 32 / 64-edge builds picked by the maximum column degree, the check kernels by the row
degree, and `append_rows` moves all of that on a handle that is alive.  tests/test_bp_gpu.py meets the oracle at full
size at ONE point of that space (W = 50 with 4000 / 8000 / 12000 rows: record form, 32-edge builds, 51-edge rows).

  part A  every point of `helpers.PRODUCTION_POINTS` (16-edge variable builds, 21- and 61-edge rows, the message form
          with 33 .. 38-edge columns, +inf priors at the bench's batch) against the oracle, on the library's own schedule;
  part B  a live decoder grown in steps of 50 rows ACROSS each line (16 and 32 with W = 50, 16 with W = 20), decoded
          after every step on every kernel family, equal to a fresh decoder bit for bit and to the oracle;
  part C  the lines no [Hin | I] graph reaches (a column / a row of 65 edges: the row-parallel tables are dropped, the
          any-degree kernels need their scratch array) on a toy, on every path.

tests/test_production_range.py pins, without a GPU, that the graphs are what they are said to be and the trials hard
enough.  No tolerance of its own anywhere: `compare` and `check_reference_form` as they are.  Every test asserts the
form and the path it claims (`record_form`, `last_row_parallel`).

What the first runs on an MI355X showed (informational; the bounds stay `compare`'s): everything agrees, no product code
changed.  min-sum bit for bit at every point and step, NaN posteriors included.  Tanh rule, largest |dL| against the
f32 oracle over the sample, early exit / fixed (share of the tolerance 2e-4 + 2e-4 |L| at the worst position):
  hqc128 W50 R2000  eps 0     3.1e-5 / 3.1e-5  (0.008)      hqc256 W60 R6000   eps 0     3.1e-5 / 2.3e-5  (0.008)
  hqc128 W50 R4000  eps 0     3.8e-5 / 0       (0.003)      hqc256 W60 R12000  eps 0.08  1.9e-5 / 1.5e-5  (0.006)
  hqc128 W20 R4000  eps 0.01  1.1e-5 / 1.5e-5  (0.004)      hqc256 W60 R20000  eps 0.2   1.1e-5 / 1.1e-5  (0.009)
  hqc128 W50 R8000  eps 0.2   1.1e-5 / 1.5e-5  (0.009)      single decode() at the eps = 0 points: <= 3.1e-5 (0.005)
  growth runs: W50 1900 -> 2100 <= 3.8e-5 (0.007), W50 6500 -> 7000 1.1e-5 (0.013), W20 7200 -> 7400 1.1e-5 (0.009).
One thing the tests had to learn: an early-exit call on > 64 codewords may hand its last few stragglers to the
row-parallel kernels in its compact pass, so `last_row_parallel() == 0` holds for fixed-iteration calls only
(`_ran_on_tiles` bounds the early-exit case by the limit and the compacted count).  Wall time of this file: 37 s
(tests/test_bp_gpu.py: 36 s; the whole `-m gpu` suite without this file: 84 s)."""
import functools
import importlib

import numpy as np
import pytest

from helpers import (ORACLE_METHOD, PRODUCTION_GROWTH, PRODUCTION_POINTS, S, check_reference_form, compare, growth_run,
                     hqc_full_size_point, prefix_graph, prefix_point, reference_floor, sample_rows)
from test_append_gpu import _rows_csr, _same

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")

MAX_ITER = 50
EL_LIMIT = {"min_sum": 6, "product_sum": 4}  # the row-parallel kernels' default limit (el_limit)


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    """The library's own choice of kernels and schedule: at size, the schedule is the subject."""
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC"):
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=1)
def _point(label):  # (both update rules decode the same trials: built once)
    p = PRODUCTION_POINTS[label]
    return hqc_full_size_point(p["name"], p["key"], p["R"], p["eps"], p["batch"])


def _take(out, idx):
    return {k: (v[idx] if v is not None else None) for k, v in out.items()}


def _ran_on_tiles(dec, method, early):
    """The batch itself went through the 64-codeword-tile kernels.  (The only codewords the row-parallel kernels may see
    are the stragglers an EARLY-EXIT call re-decodes in its compact pass, once few enough are left for them.)"""
    st = dec.last_stats()
    if early and st["row_parallel"]:
        assert 0 < st["row_parallel"] <= min(EL_LIMIT[method], st["compacted"]), st
    else:
        assert st["row_parallel"] == 0, st


def _max_dl(got, ref):
    """(informational) the largest posterior difference, both sides clamped to +-80 as `compare` does"""
    a = np.clip(np.nan_to_num(got["llr"].astype(np.float64), nan=0.0, posinf=80.0, neginf=-80.0), -80.0, 80.0)
    b = np.clip(np.nan_to_num(ref["llr"].astype(np.float64), nan=0.0, posinf=80.0, neginf=-80.0), -80.0, 80.0)
    return float(np.abs(a - b).max()), float((np.abs(a - b) / (2e-4 + 2e-4 * np.abs(b))).max())


def _against_oracle(oracle, got, H, probs, x, method, early, what, reference_form=True, max_iter=MAX_ITER):
    with np.errstate(divide="ignore"):
        ref = oracle.bp_decode_batch(H, probs, x, 1, max_iter, ORACLE_METHOD[method], dtype="f32", threads=16, early_exit=early)
        if method == "product_sum":
            dl, share = _max_dl(got, ref)
            print(f"{what} early={early}: tanh rule max |dL| = {dl:.3g} ({share:.3f} of the tolerance), oracle converged "
                  f"{ref['converged'].mean():.2f}, iteration counts {sorted(set(ref['iters'].tolist()))}")
        compare(got, ref, method)
        if method == "product_sum" and reference_form:
            check_reference_form(oracle, got, H, probs, x, 1, max_iter, early, min_fraction=reference_floor(ref), threads=16)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# part A
# ---------------------------------------------------------------------------------------------------------------------
def _decode_on_callers_stream(dec, msg, early):
    """The bench's own call (device pointers on the caller's stream, no posteriors) ..."""
    import torch

    batch, n = msg.shape
    d_in = torch.from_numpy(msg).cuda()
    d_out = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    d_conv = torch.empty(batch, dtype=torch.uint8, device="cuda")
    d_iters = torch.empty(batch, dtype=torch.int32, device="cuda")
    dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, batch, d_out.data_ptr(), early_exit=early,
                            stream=torch.cuda.current_stream().cuda_stream, d_out_conv=d_conv.data_ptr(),
                            d_out_iters=d_iters.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_conv.cpu().numpy(), d_iters.cpu().numpy()


@pytest.mark.parametrize("method", ["min_sum", "product_sum"])
@pytest.mark.parametrize("label", list(PRODUCTION_POINTS))
def test_point_against_oracle(oracle, label, method):
    """One full-size point, whole batch, early exit and 50 fixed iterations, with posteriors: a sample from the first, a
    middle and the last tile (group) against the oracle; on the whole batch, converged flags are truthful and the batch
    order does not matter.  The eps = 0 HQC-128 points run the bench's batch of 4096 from device buffers on the caller's
    stream as well (equal to the host-buffer call), the other HQC-128 points 384 + 6 codewords (a ragged last tile)."""
    p = PRODUCTION_POINTS[label]
    H, Hin, probs, msg, ys = _point(label)
    N, batch = Hin.n, p["batch"]
    if batch == 4096:  # groups of 4 or 8 tiles, two lanes each: the first tile of either lane of the first, a middle and the last group
        pick = sample_rows(batch, 5, (0, 2, 4, 32, 34, 36, 60, 62))
    else:
        pick = sample_rows(batch, 15 if batch == 390 else 14)  # 15 + 15 + 6 | 14 + 14 + 8
    assert 36 <= pick.size <= 48 and pick[-1] >= (batch - 1) // 64 * 64 - (128 if batch == 4096 else 0)  # (... reaches the last tile / group)
    with np.errstate(divide="ignore"):  # (eps = 0: p = 0 priors)
        dec = bp.bp_decoder(H, max_iter=MAX_ITER, bp_method=method, channel_probs=probs)
    for early in (True, False):
        got = dec.decode_batch(msg, early_exit=early, want_llr=True)
        _ran_on_tiles(dec, method, early)
        assert dec.time_kernels(2)["record_form"] == (method == "min_sum" and p["max_col_deg"] <= 32)
        if batch == 4096:
            bits_dev, conv_dev, iters_dev = _decode_on_callers_stream(dec, msg, early)
            _ran_on_tiles(dec, method, early)
            assert np.array_equal(got["bits"], bits_dev) and np.array_equal(got["converged"], conv_dev)
            assert np.array_equal(got["iters"], iters_dev)
        _against_oracle(oracle, _take(got, pick), H, probs, msg[pick], method, early, label)
        conv = got["converged"].astype(bool)
        assert np.array_equal(H.syndrome((got["bits"] ^ msg)[conv]), msg[conv][:, N:]), "a codeword flagged converged does not satisfy H e = s"
        if early:
            perm = np.random.RandomState(5).permutation(batch)
            again = dec.decode_batch(msg[perm], early_exit=True)
            assert np.array_equal(again["bits"], got["bits"][perm]) and np.array_equal(again["iters"], got["iters"][perm])
            assert np.array_equal(again["converged"], got["converged"][perm])
    dec.close()


@pytest.mark.parametrize("label", [k for k, p in PRODUCTION_POINTS.items() if p["eps"] == 0.0])
def test_single_decode_with_certain_checks(oracle, label):
    """The attack loop's call at each eps = 0 point: one decode(), tanh rule, max_iter 100 (hqc.py:694-708) -- the
    row-parallel kernels with +inf priors on every check, at size -- equals the oracle's codeword 0."""
    p = PRODUCTION_POINTS[label]
    H, Hin, probs, msg, ys = hqc_full_size_point(p["name"], p["key"], p["R"], p["eps"], 1)
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(H, max_iter=100, bp_method="product_sum", channel_probs=probs)
    bits = dec.decode(msg[0])
    assert dec.last_row_parallel() == 1
    got = {"bits": bits[None, :].astype(np.uint8), "llr": dec.log_prob_ratios[None, :].astype(np.float32),
           "iters": np.array([dec.iter], dtype=np.int32), "converged": np.array([dec.converge], dtype=np.uint8)}
    dec.close()
    _against_oracle(oracle, got, H, probs, msg, "product_sum", True, label + " decode()", max_iter=100)


# ---------------------------------------------------------------------------------------------------------------------
# part B
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["min_sum", "product_sum"])
@pytest.mark.parametrize("run", list(PRODUCTION_GROWTH))
def test_live_decoder_grown_across_a_line(oracle, run, method):
    """A decoder built below a line of the kernel selection and grown across it, 50 rows at a time.  After EVERY step:
    a single codeword, a batch at the row-parallel limit and 130 codewords (tiles, a ragged third one), early exit and
    fixed iterations, with posteriors -- equal to a freshly built decoder bit for bit.  At the start, at the first step
    past the crossing row and at the end: equal to the oracle.  Right after the crossing the batch doubles (130 -> 260),
    so the group capacity grows on a handle whose build / form has just changed."""
    g = PRODUCTION_GROWTH[run]
    Hin, probs, msg = growth_run(run, 260)
    N, lim = Hin.n, EL_LIMIT[method]
    pick = sample_rows(130, 17)
    assert pick.size == 36
    sizes = list(range(g["R0"], g["R1"] + 1, 50))
    first_past = next(r for r in sizes if r >= g["crossing"])
    assert sizes[1] < first_past <= sizes[-2]  # whole steps on either side of the one that holds the crossing row

    def new_decoder(r):
        with np.errstate(divide="ignore"):
            return bp.bp_decoder(prefix_graph(Hin, r), max_iter=MAX_ITER, bp_method=method, channel_probs=probs[: N + r])

    live = new_decoder(sizes[0])
    for prev, r in zip([None] + sizes[:-1], sizes):
        if prev is not None:
            rp, ci = _rows_csr(prefix_graph(Hin, r), prev, r)
            live.append_rows(rp, ci, N + r, probs[N + prev : N + r])
        H, pr, x = prefix_point(Hin, probs, msg, r)
        fresh = new_decoder(r)
        past = r >= g["crossing"]
        record = method == "min_sum" and not (g["line"] == 32 and past)
        batches = (1, lim, 130) + ((260,) if r == first_past else ())
        for nb in batches:  # (in this order: the row-parallel tables are patched in place, the tile tables rebuilt on demand)
            for early in (True, False):
                a = live.decode_batch(x[:nb], early_exit=early, want_llr=True)
                if nb <= lim:
                    assert live.last_row_parallel() == nb
                else:
                    _ran_on_tiles(live, method, early)
                    assert live.time_kernels(2)["record_form"] == record, (r, nb)
                b = fresh.decode_batch(x[:nb], early_exit=early, want_llr=True)
                _same(a, b, (run, method, r, nb, early))
                if nb == 130 and r in (sizes[0], first_past, sizes[-1]):
                    _against_oracle(oracle, _take(a, pick), H, pr, x[pick], method, early, f"{run} at {r} rows", reference_form=False)
        if method == "min_sum" and g["line"] == 32 and past:
            # asking for the record form changes nothing on a graph whose columns no longer fit it
            before = live.decode_batch(x[:130], early_exit=True, want_llr=True)
            live.configure(minsum_rec=1)
            after = live.decode_batch(x[:130], early_exit=True, want_llr=True)
            assert live.time_kernels(2)["record_form"] is False
            _same(before, after, (run, r, "minsum_rec=1"))
        fresh.close()
    assert (live.m, live.n) == (g["R1"], N + g["R1"])
    live.close()


# ---------------------------------------------------------------------------------------------------------------------
# part C
# ---------------------------------------------------------------------------------------------------------------------
def _toy(rng):
    """120 x 400, sparse; column 0 has 15 edges, row 0 has 63 (column 0 not among them); nothing else comes close."""
    H = (rng.rand(120, 400) < 0.03).astype(np.int8)
    H[:, 0] = 0
    H[0, :] = 0
    H[1:16, 0] = 1
    H[0, 1 + rng.choice(399, size=63, replace=False)] = 1
    for i in range(120):
        if not H[i].any():
            H[i, 1 + rng.randint(399)] = 1
    assert H[:, 0].sum() == 15 and H[0].sum() == 63 and H[:, 1:].sum(axis=0).max() < 15 and H[1:].sum(axis=1).max() < 40
    return H


def _exact(got, ref, what):
    """min-sum against the oracle where inf - inf = NaN posteriors occur: everything bit for bit as `compare` asks, the
    NaNs in the same places (`np.array_equal` alone calls NaN unequal to itself)."""
    assert np.array_equal(got["iters"], ref["iters"]) and np.array_equal(got["converged"].astype(np.int32), ref["converged"]), what
    assert np.array_equal(got["bits"], ref["bits"]), what
    assert np.array_equal(got["llr"], ref["llr"], equal_nan=True), what


@pytest.mark.parametrize("method", ["min_sum", "product_sum"])
@pytest.mark.parametrize("path", ["auto", "stream", "edge"])
@pytest.mark.parametrize("line", ["column", "row"])
def test_every_line_on_a_toy(oracle, line, path, method):
    """Degrees no [Hin | I] graph with W <= 60 reaches, but the ABI takes any graph: a live decoder whose designated
    column goes 15 -> 16, 17, 32, 33, 64, 65 edges, or that gains a row of 64 and then of 65 edges.  Past 32 min-sum
    leaves its record form; past 64 the row-parallel tables are dropped and the any-degree kernels need a scratch array
    the message array was sized without.  After each append, batches of 1, 5 and 150 equal a fresh decoder's bit for bit
    and the oracle's.  min-sum: p = 0 priors on a tenth of the columns (inf - inf = NaN posteriors in the same places)."""
    rng = np.random.RandomState(31)
    Hd = _toy(rng)
    probs = rng.uniform(0.02, 0.2, size=400)
    if method == "min_sum":
        probs[rng.choice(400, size=40, replace=False)] = 0.0
    if line == "column":  # (rows appended, degree of column 0 afterwards)
        steps = [(1, 16), (1, 17), (15, 32), (1, 33), (31, 64), (1, 65)]
    else:                 # (degree of the appended row)
        steps = [(1, 64), (1, 65)]
    err = (rng.rand(150, 400) < 0.05).astype(np.uint8)

    def new_decoder(dense):
        with np.errstate(divide="ignore"):
            d = bp.bp_decoder(S.TannerGraph.from_dense(dense), max_iter=20, bp_method=method, channel_probs=probs)
        if path != "auto":
            d.configure(path=path)
        return d

    def check(dense, what):
        G = S.TannerGraph.from_dense(dense)
        synd = G.syndrome(err)
        wide = max(dense.sum(axis=0).max(), dense.sum(axis=1).max()) > 64
        fresh = new_decoder(dense)
        for nb in (1, 5, 150):
            for early in (True, False):
                a = live.decode_batch(synd[:nb], early_exit=early, want_llr=True)
                if path == "edge" and nb <= 64:
                    assert live.last_row_parallel() == (0 if wide else nb), (what, nb)
                elif path == "stream":
                    assert live.last_row_parallel() == 0
                    if method == "min_sum":
                        rec = dense.sum(axis=0).max() <= 32 and dense.sum(axis=1).max() <= 64
                        assert live.time_kernels(2)["record_form"] == bool(rec), (what, nb)
                b = fresh.decode_batch(synd[:nb], early_exit=early, want_llr=True)
                _same(a, b, (what, nb, early))
                with np.errstate(divide="ignore", invalid="ignore"):
                    ref = oracle.bp_decode_batch(G, probs, synd[:nb], 0, 20, ORACLE_METHOD[method], dtype="f32", threads=8,
                                                 early_exit=early)
                if method == "min_sum":
                    _exact(a, ref, (what, nb, early))
                else:
                    compare(a, ref, method)
        fresh.close()

    live = new_decoder(Hd)
    check(Hd, "start")
    for count, target in steps:
        new = np.zeros((count, 400), dtype=np.int8)
        for i in range(count):
            if line == "column":
                new[i, 0] = 1
                new[i, 1 + rng.choice(399, size=5, replace=False)] = 1
            else:
                new[i, 1 + rng.choice(399, size=target, replace=False)] = 1
        g_new = S.TannerGraph.from_dense(new)
        live.append_rows(g_new.row_ptr, g_new.col_idx, 400, np.zeros(0))
        Hd = np.concatenate([Hd, new], axis=0)
        if line == "column":
            assert Hd[:, 0].sum() == target == Hd.sum(axis=0).max() > Hd[:, 1:].sum(axis=0).max()
        else:
            assert Hd[-1].sum() == target == Hd.sum(axis=1).max()
        check(Hd, (line, target))
    live.close()
