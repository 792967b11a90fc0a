"""Settled min-sum (knob `settle`) on every kernel instantiation and launch shape its code can meet, where
tests/test_settle_gpu.py and tests/test_settle_outputs_gpu.py run one graph (rows of 11, columns of at most 8: cap 16 of both
record-form kernels) on launches of one and three tiles.  Here: rows of 18 and 34 edges and columns of up to 17 (the other
instantiations of k_check_minsum_rec / k_var_rec, whose compare-what-you-overwrite code is per degree); launches of 2, 4 and 8
tiles, which k_var_rec maps to XCDs before it takes its settle word (`xmap`), under 1, 2 and 3 stream lanes, and the re-run
groups that start in the middle of a call; first_fused = 0, fuse_test = 0, minsum_rec = 0; a soft call; a handle whose graph
grows; the Monte-Carlo sweeps, which run under a horizon learned on other trials; asynchronous device calls.

The bar is that of tests/test_settle_gpu.py: every call is held to the float32 oracle -- decisions, posterior bit patterns,
converged flags, iteration counts, all equal -- and to a handle with settle = 0 on the same inputs, and its report
(scaldpc_bp_last_settle) to the frozen-at numbers of tests/settle_ref.py and the rules of scaldpc_bp_sched.h as
tests/settle_matrix_cases.py restates them.  No tolerance anywhere.  tests/test_settle_matrix.py shows that the inputs hold
what the cases rely on.  The path is pinned to the 64-codeword-tile kernels."""
import importlib
import types

import numpy as np
import pytest

import settle_matrix_cases as M

bp = importlib.import_module("sca-ldpc_amd.bp")
driver = importlib.import_module("sca-ldpc_amd.driver")
lib = importlib.import_module("sca-ldpc_amd._lib")

pytestmark = pytest.mark.gpu
OFF = {"frozen_at": [], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}


def decoder(c, *, settle=None, group=0, **knobs):
    dec = bp.bp_decoder(c.H, max_iter=M.MAX_ITER, bp_method="min_sum", channel_probs=c.probs, ms_scaling_factor=1.0)
    dec.configure(path="stream", **knobs)
    if settle is not None:
        dec.configure(settle=settle)
    dec.set_tile_group(group)
    return dec


def same(got, ref, what):
    assert (got["bits"] == ref["bits"]).all(), what
    if got["llr"] is not None:
        assert (got["llr"].view(np.uint32) == ref["llr"].view(np.uint32)).all(), what
    assert (got["converged"].astype(np.int32) == ref["converged"].astype(np.int32)).all(), what
    assert (got["iters"] == ref["iters"]).all(), what


def call(dec, synd, want_llr, **kw):
    return dec.decode_batch(synd, max_iter=M.MAX_ITER, early_exit=False, want_llr=want_llr, **kw)


def report(want, K):
    """What a tracked call with horizon K (0 = none) reports, but for launches_saved (positive with a horizon, else 0)."""
    return {"frozen_at": list(want), "tiles_rerun": M.rerun(want, K), "horizon": K}


def held(st, want, K, what):
    assert {k: st[k] for k in ("frozen_at", "tiles_rerun", "horizon")} == report(want, K), (what, st, want, K)
    assert (st["launches_saved"] > 0) == (K > 0), (what, st)


def three_calls(c, ref, want=None, *, group=0, long_horizon=False, schedule=None, tracked=True, call_kw=None, **knobs):
    """One handle, three calls: it learns; it runs under what it learned (a horizon of the largest frozen-at number + 2 where at
    least 7/8 of the tiles froze, else none); it runs under a forced horizon below the largest frozen-at number, which decodes
    again every tile not frozen by it -- and those report what their re-run found.  long_horizon: a fourth call, forced to the
    largest frozen-at number + 2: exactly the tiles that never freeze are decoded again.  The whole sequence once with and
    once without posteriors; the two sequences of reports are equal."""
    want = c.want if want is None else want
    call_kw = call_kw or {}
    off = decoder(c, settle=0, group=group, **knobs)
    reports = []
    for want_llr in (True, False):
        dec, seen = decoder(c, group=group, **knobs), []
        K = 0
        steps = [("learns", None), ("learned horizon", None), ("short horizon", M.short_horizon(want))]
        if long_horizon:
            steps.append(("long horizon", max(want) + 2))
        for what, forced in steps:
            if forced is not None:
                assert M.usable(forced)
                dec.configure(settle_horizon=forced)
                K = forced
            got = call(dec, c.synd, want_llr, **call_kw)
            st = dec.last_settle()
            print(what, want_llr, st, dec.last_schedule()["fixed_chained"], flush=True)
            same(got, ref, f"oracle, {what}")
            same(got, call(off, c.synd, want_llr, **call_kw), f"settle = 0, {what}")
            assert off.last_settle() == OFF
            if not tracked:
                assert st == OFF, what
                continue
            held(st, want, K, what)
            if what == "learned horizon" and K:
                assert st["horizon"] == max(want) + 2
            if what == "short horizon":
                assert st["tiles_rerun"] == sum(1 for f in want if not 0 < f <= forced) > 0
            if schedule:
                schedule(dec.last_schedule())
            seen.append(st)
            K = M.next_horizon(want, K)
        reports.append(seen)
        dec.close()
    assert reports[0] == reports[1]
    off.close()
    return reports[0]


# ------------------------------------------------------------------------------------------------------------ the kernel ladder
@pytest.mark.parametrize("name", ["row32", "row64", "col32", "ties32", "ties64"])
def test_kernel_ladder(scaldpc, oracle, name):
    """k_check_minsum_rec<32> / <64> (rows of 18 / 34 edges: the 34-edge rows fetch what they overwrite late) and
    k_var_rec<32> (columns of up to 17 edges, beyond the records' inline ids), each with a partial last tile, a tile that never
    freezes and -- row32 -- one that freezes at the next-to-last test.  ties32 / ties64: the same rows with every prior one
    float; there a tile's last change is an arg-min byte alone, which the check pass must not leave out of its compare."""
    c = M.case(name)
    three_calls(c, M.oracle_of(name))


# -------------------------------------------------------------------------------------------------------------- launch shapes
def chained(sched):
    assert sched["fixed_chained"] > 0


@pytest.mark.parametrize("split,group", [(2, 4), (2, 8), (2, 16), (1, 2), (1, 4), (1, 8), (3, 6)])
def test_launch_shapes_one_unfrozen_tile(scaldpc, oracle, split, group):
    """Ten tiles, tile 5 never freezes.  (split, group): (2, 4) two tiles per launch, chained groups -- the bench's shape;
    (2, 8) four per launch, then a group of two; (2, 16) one group of ten, five per lane, no XCD map; (1, 2), (1, 4), (1, 8)
    one lane (the column records heaviest first); (3, 6) three lanes of two, then two, one and one.  The second call runs under
    the learned horizon and decodes tile 5 again: a group of one that starts in the middle of the call."""
    c = M.case("wide_one")
    seen = three_calls(c, M.oracle_of("wide_one"), group=group, split=split, long_horizon=True,
                       schedule=chained if (split, group) == (2, 4) else None)
    assert seen[1]["horizon"] == max(c.want) + 2 and seen[1]["tiles_rerun"] == 1 and seen[3]["tiles_rerun"] == 1


@pytest.mark.parametrize("split,group", [(1, 4), (2, 4)])
def test_launch_shapes_adjacent_unfrozen_tiles(scaldpc, oracle, split, group):
    """Tiles 2, 3 and 6 never freeze: fewer than 7/8 freeze, so nothing is learned; under the forced horizons tiles 2 and 3 are
    decoded again as ONE group that starts at tile 2 (one launch of two tiles with one lane, one tile per lane with two) and
    tile 6 as a group of one."""
    c = M.case("wide_three")
    seen = three_calls(c, M.oracle_of("wide_three"), group=group, split=split, long_horizon=True)
    assert seen[1]["horizon"] == 0 and seen[3]["tiles_rerun"] == 3


# ------------------------------------------------------------------------------------------------------------------ knob forms
@pytest.mark.parametrize("knob", ["first_fused", "fuse_test", "minsum_rec"])
def test_knob_forms(scaldpc, oracle, knob):
    """first_fused = 0: iteration 1 has a message-form check pass and the bootstrap record pass moves to iteration 2;
    fuse_test = 0: the unsharded k_parity_fin closes the call; minsum_rec = 0: no record form, so nothing is tracked -- the
    report is the "did not track" one and the results are the oracle's."""
    c = M.case("base")
    three_calls(c, M.oracle_of("base"), tracked=knob != "minsum_rec", **{knob: 0})


# -------------------------------------------------------------------------------------------------------------- the soft call
def test_soft_call_on_wide_columns(scaldpc, oracle):
    """Per-codeword priors for the 600 check columns of col32, two rows dealt to 130 codewords in turn: the frozen-at numbers
    are those of the restatement on every codeword's own priors."""
    c, s = M.case("col32"), M.soft()
    inputs = types.SimpleNamespace(H=c.H, probs=c.probs, synd=s.synd, want=s.want)
    three_calls(inputs, M.soft_oracle(), call_kw=dict(channel_probs=s.cp))


# ------------------------------------------------------------------------------------------------------------ a growing handle
def _tail_rows(H, first):
    rp = np.asarray(H.row_ptr)[first:].astype(np.int64)
    return (rp - rp[0]).astype(np.int32), np.asarray(H.col_idx)[rp[0] : rp[-1]].astype(np.int32)


@pytest.mark.parametrize("want_llr", [True, False])
def test_growing_handle(scaldpc, oracle, want_llr):
    """100 rows: call (learns), call (horizon in force).  append_rows of the other 50 with their identity columns and
    update_channel_probs, as the attack loop does: call (no horizon: what was learned belongs to another graph), call (the new
    one).  Then a row without a column of its own, into a column of Hin that had degree 1 and into the identity column of row 7,
    whose last edge is then no constant any more -- and NO new priors, so that the horizon is append_rows' own to forget: call
    (no horizon), call.  That graph is no [Hin | I], so the handle is told settle = 2 for it.  Every call is the oracle's on the
    graph as it is then, and a fresh decoder's."""
    first, grown, extra = M.case("base100"), M.case("grown"), M.case("extra")
    dec = decoder(first)
    seen = []

    def two_calls(c, name):
        fresh = decoder(c, settle=0)
        K = 0
        for n_call in range(2):
            got = call(dec, c.synd, want_llr)
            st = dec.last_settle()
            print(name, n_call, st, flush=True)
            same(got, M.oracle_of(name), f"oracle, {name}, call {n_call}")
            same(got, call(fresh, c.synd, want_llr), f"fresh decoder, {name}, call {n_call}")
            held(st, c.want, K, (name, n_call))
            seen.append(st)
            K = M.next_horizon(c.want, K)
        fresh.close()

    two_calls(first, "base100")
    assert seen[1]["horizon"] == max(first.want) + 2
    rp, ci = _tail_rows(grown.H, M.GROW_FIRST)
    dec.append_rows(rp, ci, grown.H.n, grown.probs[first.H.n :])
    dec.update_channel_probs(grown.probs)
    two_calls(grown, "grown")
    assert seen[2]["horizon"] == 0 and seen[3]["horizon"] == max(grown.want) + 2
    dec.configure(settle=2)
    row = M.extra_row(grown.H)
    dec.append_rows(np.array([0, len(row)], dtype=np.int32), row, grown.H.n, np.zeros(0))
    two_calls(extra, "extra")
    assert seen[4]["horizon"] == 0 and seen[5]["horizon"] == M.next_horizon(extra.want, 0)
    dec.close()


# ------------------------------------------------------------------------------------------------------------------ the sweeps
def _sweep_steps():
    return [(0, None), (M.SWEEP_FIRST2, None), (0, M.SWEEP_HORIZON)]


def test_hqc_sweep(scaldpc, oracle):
    """mc_hqc_run(early_exit=False, want_stats=True): level 0 without a posterior plane, per-trial priors, and k_mc_hqc_stats
    reading the decision planes after the re-runs.  Trials 0 ... 139 (learns), 1000 ... 1139 (under the horizon learned on
    the others: one tile is decoded again), 0 ... 139 with the horizon forced to 5 (all three are).  The sweep leaves its
    report in scaldpc_bp_last_settle like any call."""
    base = M.case("base")
    N = base.H.n - base.H.m
    dec, off = decoder(base), decoder(base, settle=0)
    K = 0
    for first, forced in _sweep_steps():
        if forced:
            dec.configure(settle_horizon=forced)
            K = forced
        kw = dict(omega=3, eps=0.02, seed=M.HQC_SEED, first_trial=first, max_iter=M.MAX_ITER, early_exit=False, want_inputs=True,
                  want_stats=True, want_bits=True)
        got = dec.mc_hqc_run(M.SWEEP_RUNS, **kw)
        st = dec.last_settle()
        print(first, forced, st, flush=True)
        plain = off.mc_hqc_run(M.SWEEP_RUNS, **kw)
        assert off.last_settle() == OFF
        for k in got:
            assert np.array_equal(got[k], plain[k]), (first, k)
        c, ref = M.sweep("hqc", first), M.sweep_oracle("hqc", first, True)
        assert np.array_equal(got["msg"], c.msg) and np.array_equal(got["y"], c.y)
        assert np.array_equal(got["bits"], ref["bits"]) and np.array_equal(got["iters"], ref["iters"])
        rows = [driver.hqc_stats(N, ref["bits"][i], c.msg[i, N:], c.y[i]) for i in range(M.SWEEP_RUNS)]
        assert got["success"].tolist() == [int(ok) for ok, _ in rows]
        assert got["stats"].tolist() == [[s[k] for k in bp.HQC_STATS_COLUMNS] for _, s in rows]
        # decode_batch on the exported inputs, with the sweep's priors per codeword
        d = call(off, got["msg"], True, channel_probs=np.full((M.SWEEP_RUNS, base.H.m), 0.02, dtype=np.float32))
        same(d, ref, f"decode_batch on the exported inputs, {first}")
        held(st, c.want, K, (first, forced))
        K = M.next_horizon(c.want, K)
        if forced is None and first:
            assert st["horizon"] > 0 and st["tiles_rerun"] == 1
    assert st["horizon"] == M.SWEEP_HORIZON and st["tiles_rerun"] == 3
    dec.close()
    off.close()


def test_fer_sweep(scaldpc, oracle):
    """mc_fer_run(early_exit=False): shared priors, syndromes of errors drawn on the device.  The same three calls."""
    base = M.case("base")
    dec, off = decoder(base), decoder(base, settle=0)
    K = 0
    for first, forced in _sweep_steps():
        if forced:
            dec.configure(settle_horizon=forced)
            K = forced
        kw = dict(seed=M.FER_SEED, first_trial=first, max_iter=M.MAX_ITER, early_exit=False, want_errors=True)
        got = dec.mc_fer_run(M.SWEEP_RUNS, **kw)
        st = dec.last_settle()
        print(first, forced, st, flush=True)
        plain = off.mc_fer_run(M.SWEEP_RUNS, **kw)
        assert off.last_settle() == OFF
        for k in got:
            assert np.array_equal(got[k], plain[k]), (first, k)
        c, ref = M.sweep("fer", first), M.sweep_oracle("fer", first)
        assert np.array_equal(got["errors"], c.errors)
        assert got["success"].tolist() == (ref["bits"] == c.errors).all(axis=1).astype(int).tolist()
        assert np.array_equal(got["iters"], ref["iters"])
        same(call(off, c.synd, True), ref, f"decode_batch on the exported inputs, {first}")
        held(st, c.want, K, (first, forced))
        K = M.next_horizon(c.want, K)
        if forced is None and first:
            assert st["horizon"] > 0 and st["tiles_rerun"] == 1
    assert st["horizon"] == M.SWEEP_HORIZON and st["tiles_rerun"] == 3
    dec.close()
    off.close()


# ------------------------------------------------------------------------------------------------- asynchronous device calls
@pytest.mark.parametrize("want_llr", [True, False])
def test_asynchronous_device_call(scaldpc, oracle, want_llr):
    """decode_batch_device on a torch stream: synchronous (learns), SCALDPC_F_ASYNC (enqueues only: it skips on the device,
    reads nothing back, reports nothing and neither uses nor forgets the learned horizon), synchronous (runs under the horizon
    the first call learned).  After a stream synchronise the asynchronous outputs are the oracle's."""
    import torch

    c = M.case("grown")  # 69 codewords of the base graph: both tiles freeze
    ref = M.oracle_of("grown")
    batch, n = c.synd.shape[0], c.H.n
    dec = decoder(c)
    stream = torch.cuda.Stream()
    seen = []
    with torch.cuda.stream(stream):
        d_in = torch.from_numpy(c.synd).cuda()
        for asynchronous in (False, True, False):
            out = dict(bits=torch.full((batch, n), 0xAA, dtype=torch.uint8, device="cuda"),
                       llr=torch.full((batch, n), float("nan"), dtype=torch.float32, device="cuda") if want_llr else None,
                       iters=torch.full((batch,), -7, dtype=torch.int32, device="cuda"),
                       converged=torch.full((batch,), 0xAA, dtype=torch.uint8, device="cuda"))
            stream.synchronize()
            dec.decode_batch_device(d_in.data_ptr(), lib.IN_SYNDROME, batch, out["bits"].data_ptr(), max_iter=M.MAX_ITER,
                                    early_exit=False, stream=stream.cuda_stream, d_out_llr=out["llr"].data_ptr() if want_llr else 0,
                                    d_out_iters=out["iters"].data_ptr(), d_out_conv=out["converged"].data_ptr(),
                                    asynchronous=asynchronous)
            seen.append(dec.last_settle())
            stream.synchronize()
            got = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
            same(got, ref, f"oracle, asynchronous = {asynchronous}")
    print(seen, flush=True)
    held(seen[0], c.want, 0, "synchronous, learns")
    assert seen[1] == OFF
    held(seen[2], c.want, max(c.want) + 2, "synchronous, after the asynchronous call")
    dec.close()
