"""Min-sum in its record form on columns of 33 to 64 edges (`minsum_rec = 2`): a second variable launch,
k_var<64, ..> in its record mode over the widest degree bucket, beside the narrow kernels' launch over the other buckets.

Every decode here is compared with the f32 oracle bit for bit -- decisions, iteration counts, converged flags and
posteriors, NaNs in the same places (`_exact` of tests/test_production_range_gpu.py) -- and with the same handle under
`minsum_rec = 0`; every case that claims the record form asserts `time_kernels(2)["record_form"] is True`.  The inputs are
tests/rec_wide_cases.py's; tests/test_rec_wide.py shows without a GPU that they decide something.  The path is pinned to
the 64-codeword-tile kernels."""
import importlib

import numpy as np
import pytest

import kernel_matrix_cases as K
import mc_ref
import rec_wide_cases as W
import settle_ref as R
from helpers import PRODUCTION_POINTS, S, hqc_full_size_point, sample_rows
from test_append_gpu import _same
from test_production_range_gpu import _exact, _toy

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")


@pytest.fixture(autouse=True)
def own_knobs(monkeypatch):
    """Every knob at the library's default unless a case sets it."""
    for v in ("SCALDPC_PATH", "SCALDPC_SPLIT", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_COMPACT_AFTER", "SCALDPC_FIRST_FUSED",
              "SCALDPC_FUSE_TEST", "SCALDPC_MINSUM_REC", "SCALDPC_PRECISION", "SCALDPC_SETTLE", "SCALDPC_SETTLE_HORIZON"):
        monkeypatch.delenv(v, raising=False)


def _decoder(G, probs, max_iter, rec=2, **knobs):
    with np.errstate(divide="ignore"):  # (p = 0 priors)
        dec = bp.bp_decoder(G, max_iter=max_iter, bp_method="min_sum", channel_probs=probs)
    dec.configure(path="stream", minsum_rec=rec, **knobs)
    return dec


def _decode(dec, synd, early, prior=None, **kw):
    with np.errstate(divide="ignore"):
        return dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome", channel_probs=prior, **kw)


def _record(dec):
    return dec.time_kernels(2)["record_form"]


# ------------------------------------------------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("tall", [False, True], ids=["72x200", "144x400"])
@pytest.mark.parametrize("R_,C", W.WIDE)
def test_wide_columns_on_graph(oracle, R_, C, tall):
    """Graph (R, C), C in 33 .. 64: early exit x prior source x first_fused x fuse_test as the kernel matrix composes them;
    tile groups of one and of two tiles on one and on two lanes (a launch over two tiles takes the XCD map, a launch over one
    does not); and the call whose first record pass carries the convergence test."""
    seed = W.SEEDS[(R_, C, tall)]
    G, _ = K.graph(R_, C, tall, seed)
    inp = K.inputs(R_, C, "min_sum", tall, seed)
    key = lambda early, prior: K.key(R_, C, "min_sum", early, prior, K.BATCH, tall, seed)
    for knobs in ({}, {"first_fused": 0}, {"fuse_test": 0}):
        dec = _decoder(G, inp["probs"], K.MAX_ITER, **knobs)
        kept = {}
        for prior in ("shared", "full") + (("tail",) if not knobs else ()):
            for early in (True, False):
                what = (R_, C, tall, knobs, prior, early)
                got = _decode(dec, inp["synd"], early, K.prior_array(inp, prior))
                assert dec.last_row_parallel() == 0 and _record(dec) is True, what
                _exact(got, key(early, prior), what)
                kept[(prior, early)] = got
        dec.configure(minsum_rec=0)  # the same handle in the message form
        for (prior, early), got in kept.items():
            other = _decode(dec, inp["synd"], early, K.prior_array(inp, prior))
            assert _record(dec) is False
            _same(got, other, (R_, C, tall, knobs, prior, early, "minsum_rec=0"))
        dec.close()
    for group in (1, 2):
        for split in (1, 2):
            dec = _decoder(G, inp["probs"], K.MAX_ITER, split=split)
            dec.set_tile_group(group)
            for early in (True, False):
                got = _decode(dec, inp["synd"], early)
                assert dec.last_row_parallel() == 0 and _record(dec) is True
                _exact(got, key(early, "shared"), (R_, C, tall, "group", group, "split", split, early))
            dec.close()
    # A group skips its poll at iteration 1 once an earlier group of the call saw nobody finish there; only then does
    # iteration 1's test ride on iteration 2's check pass, the FIRST record pass (k_check_minsum_rec<CAP, true, true>).
    ref = key(True, "shared")
    late = np.flatnonzero(~(ref["converged"].astype(bool) & (ref["iters"] == 1)))
    order = np.concatenate([np.resize(late, 64), np.arange(K.BATCH)])
    dec = _decoder(G, inp["probs"], K.MAX_ITER)
    dec.set_tile_group(1)
    got = _decode(dec, inp["synd"][order], True)
    assert dec.last_row_parallel() == 0 and dec.last_schedule()["polls"] >= 2 and _record(dec) is True
    _exact(got, {k: v[order] for k, v in ref.items()}, (R_, C, tall, "one-tile groups"))
    dec.close()


# ------------------------------------------------------------------------------------------------------------- 2. the lines
@pytest.mark.parametrize("R_,C,rec", [(16, 65, 2), (65, 48, 2), (16, 33, 1)])
def test_past_the_lines_it_is_the_message_form(oracle, R_, C, rec):
    """A column or a row of 65 edges under knob 2, a column of 33 under knob 1: the message form, as before."""
    seed = W.SEEDS[(R_, C, False)]
    G, _ = K.graph(R_, C, False, seed)
    inp = K.inputs(R_, C, "min_sum", False, seed)
    dec = _decoder(G, inp["probs"], K.MAX_ITER, rec=rec)
    for early in (True, False):
        got = _decode(dec, inp["synd"], early)
        assert dec.last_row_parallel() == 0 and _record(dec) is False
        _exact(got, K.key(R_, C, "min_sum", early, "shared", K.BATCH, False, seed), (R_, C, rec, early))
    dec.close()


def test_any_other_value_is_one(oracle):
    """0 = off, 2 = wide; every other value means what it meant: 1."""
    seed = W.SEEDS[(16, 33, False)]
    G, _ = K.graph(16, 33, False, seed)
    Gn, _ = K.graph(16, 32)
    inp, inpn = K.inputs(16, 33, "min_sum", False, seed), K.inputs(16, 32, "min_sum")
    for value, wide, narrow in ((0, False, False), (1, False, True), (2, True, True), (3, False, True), (-1, False, True),
                                ("2.5", False, True)):
        for graph, i, want in ((G, inp, wide), (Gn, inpn, narrow)):
            dec = _decoder(graph, i["probs"], K.MAX_ITER, rec=value)
            _decode(dec, i["synd"], False)
            assert _record(dec) is want, (value, graph.n, want)
            dec.close()


@pytest.mark.parametrize("value,wide", [("2", True), ("1", False), ("0", False)])
def test_value_from_the_environment(oracle, monkeypatch, value, wide):
    """SCALDPC_MINSUM_REC is read once, when the handle is created, through the same parse as configure()."""
    seed = W.SEEDS[(16, 33, False)]
    G, _ = K.graph(16, 33, False, seed)
    inp = K.inputs(16, 33, "min_sum", False, seed)
    monkeypatch.setenv("SCALDPC_MINSUM_REC", value)
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(G, max_iter=K.MAX_ITER, bp_method="min_sum", channel_probs=inp["probs"])
    monkeypatch.delenv("SCALDPC_MINSUM_REC")  # (a handle does not read it again)
    dec.configure(path="stream")
    got = _decode(dec, inp["synd"], False)
    assert _record(dec) is wide
    _exact(got, K.key(16, 33, "min_sum", False, "shared", K.BATCH, False, seed), ("environment", value))
    dec.close()


# ------------------------------------------------------------------------------------------------------ 3. every exact degree
def test_every_exact_degree(oracle):
    """One column of every degree 33 .. 64 (and of every degree below) in one decode, 130 codewords."""
    G, _, probs, synd = W.staircase()
    dec = _decoder(G, probs, W.STAIR_ITER)
    kept = {}
    for early in (True, False):
        got = _decode(dec, synd, early)
        assert dec.last_row_parallel() == 0 or early
        assert _record(dec) is True
        _exact(got, W.staircase_key(early), ("staircase", early))
        kept[early] = got
    dec.configure(minsum_rec=0)
    for early, got in kept.items():
        other = _decode(dec, synd, early)
        assert _record(dec) is False
        _same(got, other, ("staircase", early, "minsum_rec=0"))
    dec.close()


# ----------------------------------------------------------------------------------------------------------------- 4. growth
def test_column_grown_across_both_lines(oracle):
    """The toy of test_every_line_on_a_toy, column 0 grown 15 -> 16, 17, 32, 33, 64, 65 edges on a live decoder under knob
    2: the record form up to 64 edges, the message form at 65; after every step 150 codewords equal a fresh decoder's and
    the oracle's."""
    rng = np.random.RandomState(31)
    Hd = _toy(rng)
    probs = rng.uniform(0.02, 0.2, size=400)
    probs[rng.choice(400, size=40, replace=False)] = 0.0
    err = (rng.rand(150, 400) < 0.05).astype(np.uint8)

    def check(dense, what):
        G = S.TannerGraph.from_dense(dense)
        synd = G.syndrome(err)
        fresh = _decoder(G, probs, 20)
        for early in (True, False):
            a = _decode(live, synd, early)
            if not early:
                assert live.last_row_parallel() == 0
            assert _record(live) is bool(dense.sum(axis=0).max() <= 64), what
            b = _decode(fresh, synd, early)
            _same(a, b, (what, early))
            with np.errstate(divide="ignore", invalid="ignore"):
                ref = oracle.bp_decode_batch(G, probs, synd, 0, 20, "min_sum", dtype="f32", threads=8, early_exit=early)
            _exact(a, ref, (what, early))
        fresh.close()

    live = _decoder(S.TannerGraph.from_dense(Hd), probs, 20)
    check(Hd, "start")
    for count, target in [(1, 16), (1, 17), (15, 32), (1, 33), (31, 64), (1, 65)]:
        new = np.zeros((count, 400), dtype=np.int8)
        for i in range(count):
            new[i, 0] = 1
            new[i, 1 + rng.choice(399, size=5, replace=False)] = 1
        g_new = S.TannerGraph.from_dense(new)
        live.append_rows(g_new.row_ptr, g_new.col_idx, 400, np.zeros(0))
        Hd = np.concatenate([Hd, new], axis=0)
        assert Hd[:, 0].sum() == target == Hd.sum(axis=0).max() > Hd[:, 1:].sum(axis=0).max()
        check(Hd, target)
    live.close()


# ----------------------------------------------------------------------------------------------------------------- 5. settle
OFF = {"frozen_at": [], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}


def test_settled_tiles_with_a_wide_column(oracle):
    """[Hin | I] with one column of 40 edges, 130 codewords, 30 fixed iterations: the first tile freezes, the second never
    does.  settle 0, 1, 2 and a forced horizon give the oracle's outputs, and the frozen-at numbers are settle_ref's."""
    c = W.settle_case()
    ref = W.settle_key()
    want = R.frozen_at(c.same, c.first, W.SETTLE_ITER, batch=W.SETTLE_BATCH)
    tracked = {"frozen_at": want, "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    call = lambda dec: _decode(dec, c.synd, False)
    off = _decoder(c.H, c.probs, W.SETTLE_ITER, settle=0)
    base = call(off)
    assert _record(off) is True and off.last_row_parallel() == 0
    _exact(base, ref, "settle = 0")
    assert off.last_settle() == OFF
    for settle in (1, 2):
        dec = _decoder(c.H, c.probs, W.SETTLE_ITER, settle=settle)
        for n_call in range(2):  # (settle = 2: fewer than 7/8 of the tiles froze in the first call, so no horizon is learned)
            got = call(dec)
            st = dec.last_settle()
            assert _record(dec) is True
            _exact(got, ref, ("settle", settle, n_call))
            _same(got, base, ("settle", settle, n_call, "settle = 0"))
            assert st == tracked, (settle, n_call, st)
        dec.close()
    # the library's own choice on a graph [Hin | I] is 2
    dec = _decoder(c.H, c.probs, W.SETTLE_ITER)
    _exact(call(dec), ref, "default settle")
    assert dec.last_settle() == tracked
    # a horizon forced to the largest frozen-at number + 2 (what a call learns where every tile froze): passes of the
    # frozen tiles are not enqueued, the tile that never froze is decoded again
    K_ = max(want) + 2
    dec.configure(settle_horizon=K_)
    got = call(dec)
    st = dec.last_settle()
    _exact(got, ref, "forced horizon")
    assert st["horizon"] == K_ and st["launches_saved"] > 0 and st["tiles_rerun"] >= 1 and st["frozen_at"] == want, st
    dec.configure(minsum_rec=0)
    _same(call(dec), base, "minsum_rec=0")
    assert _record(dec) is False and dec.last_settle() == OFF
    dec.close()
    off.close()


def test_learned_horizon_with_a_wide_column(oracle):
    """The same graph, ten tiles that all freeze: the first settle = 2 call learns the horizon (the slowest tile's frozen-at
    number + 2), the second runs under it -- passes not enqueued, no tile decoded again -- and both give the oracle's outputs
    and settle = 0's."""
    c = W.horizon_case()
    ref = W.horizon_key()
    want = R.frozen_at(c.same, c.first, W.HORIZON_ITER, batch=W.HORIZON_BATCH)
    off, dec = _decoder(c.H, c.probs, W.HORIZON_ITER, settle=0), _decoder(c.H, c.probs, W.HORIZON_ITER, settle=2)
    base = _decode(off, c.synd, False)
    _exact(base, ref, "settle = 0")
    seen = []
    for n_call in range(2):
        got = _decode(dec, c.synd, False)
        seen.append(dec.last_settle())
        assert _record(dec) is True and dec.last_row_parallel() == 0
        _exact(got, ref, ("settle = 2", n_call))
        _same(got, base, ("settle = 2", n_call, "settle = 0"))
    assert seen[0] == {"frozen_at": want, "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}, seen[0]
    assert seen[1]["horizon"] == max(want) + 2 and seen[1]["launches_saved"] > 0 and seen[1]["tiles_rerun"] == 0, seen[1]
    assert seen[1]["frozen_at"] == want
    dec.close()
    off.close()


# ----------------------------------------------------------------------------------------------------------------- 6. sweeps
@pytest.mark.parametrize("early", [True, False], ids=["early", "fixed"])
def test_sweeps_with_a_wide_column(oracle, early):
    """mc_hqc_run and mc_fer_run on the settle graph, 130 trials: knob 2 == knob 0, and the first 24 trials are what
    decode_batch returns for the exported inputs."""
    c = W.settle_case()
    runs, seed, n24 = 130, 77, 24
    wide, msgf = _decoder(c.H, c.probs, W.SETTLE_ITER), _decoder(c.H, c.probs, W.SETTLE_ITER, rec=0)
    hq = [d.mc_hqc_run(runs, W.SETTLE_OMEGA, W.SETTLE_EPS, seed, early_exit=early, want_inputs=True) for d in (wide, msgf)]
    fe = [d.mc_fer_run(runs, seed, early_exit=early, want_errors=True) for d in (wide, msgf)]
    for a, b in (hq, fe):
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), (k, early)
    d = wide.decode_batch(hq[0]["msg"][:n24], early_exit=early, want_llr=True, input_vector_type="received")
    assert _record(wide) is True
    assert np.array_equal(hq[0]["success"][:n24], mc_ref.hqc_success(d["bits"], hq[0]["y"][:n24], W.SETTLE_N).astype(np.uint8))
    assert np.array_equal(hq[0]["iters"][:n24], d["iters"])
    err = fe[0]["errors"][:n24]
    d = wide.decode_batch(c.H.syndrome(err), early_exit=early, want_llr=True, input_vector_type="syndrome")
    assert np.array_equal(fe[0]["success"][:n24], (d["bits"] == err).all(axis=1).astype(np.uint8))
    assert np.array_equal(fe[0]["iters"][:n24], d["iters"])
    assert len(set(hq[0]["success"].tolist())) == 2 or len(set(hq[0]["iters"].tolist())) > 1  # (the sweep decides something)
    wide.close()
    msgf.close()


# ------------------------------------------------------------------------------------------------------- 7. one point at size
def test_production_point_with_wide_columns(oracle):
    """HQC-128, W 50, 8000 rows: 408 000 edges, 54 columns of 33 .. 36 edges among 25 669; 390 codewords, 30 iterations."""
    p = PRODUCTION_POINTS["hqc128_W50_R8000"]
    H, Hin, probs, msg, _ = hqc_full_size_point(p["name"], p["key"], p["R"], p["eps"], p["batch"])
    cdeg = np.diff(np.asarray(H.col_ptr))
    assert H.nnz == p["E"] and (cdeg > 32).sum() == p["cols_over_32"] == 54 and cdeg.max() == p["max_col_deg"] <= 64
    pick = sample_rows(p["batch"], 12)
    dec = bp.bp_decoder(H, max_iter=30, bp_method="min_sum", channel_probs=probs)
    dec.configure(minsum_rec=2)
    kept = {}
    for early in (True, False):
        got = dec.decode_batch(msg, early_exit=early, want_llr=True)
        assert _record(dec) is True
        ref = oracle.bp_decode_batch(H, probs, msg[pick], 1, 30, "min_sum", dtype="f32", threads=16, early_exit=early)
        _exact({k: v[pick] for k, v in got.items()}, ref, ("hqc128_W50_R8000", early))
        kept[early] = got
    dec.configure(minsum_rec=0)
    for early, got in kept.items():
        other = dec.decode_batch(msg, early_exit=early, want_llr=True)
        assert _record(dec) is False
        _same(got, other, ("hqc128_W50_R8000", early, "minsum_rec=0"))
    dec.close()
