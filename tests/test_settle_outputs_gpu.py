"""Settled codewords, calls that want NO posteriors (want_llr=False): there every record-form variable pass of a tracked level
leaves its columns' decisions, and the closing pass returns for the columns of a frozen tile that have them (k_var_rec,
DESIGN.md 4).  tests/test_settle_gpu.py calls with want_llr=True throughout and never reaches that path.  Every call here is
held to the float32 oracle and to a handle with settle = 0 -- decisions bit for bit, converged flags, iteration counts -- and
the settle report (frozen-at numbers, launches saved, tiles re-run, horizon) to tests/settle_ref.py and to the same call with
want_llr=True, which runs the closing pass in full.  The path is pinned to the 64-codeword-tile kernels."""
import functools
import importlib

import numpy as np
import pytest

import settle_ref as R

bp = importlib.import_module("sca-ldpc_amd.bp")

pytestmark = pytest.mark.gpu
OFF = {"frozen_at": [], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}


def decoder(c, *, settle=None, **knobs):
    dec = bp.bp_decoder(c.H, max_iter=R.MAX_ITER, bp_method="min_sum", channel_probs=c.probs, ms_scaling_factor=c.alpha)
    dec.configure(path="stream", **knobs)
    if settle is not None:
        dec.configure(settle=settle)
    return dec


def same(got, ref, what):
    assert got["llr"] is None, what
    assert (got["bits"] == ref["bits"]).all(), what
    assert (got["converged"].astype(np.int32) == ref["converged"].astype(np.int32)).all(), what
    assert (got["iters"] == ref["iters"]).all(), what


def call(dec, x, max_iter=R.MAX_ITER, want_llr=False, **kw):
    return dec.decode_batch(x, max_iter=max_iter, early_exit=False, want_llr=want_llr, **kw)


def head(ref, batch):
    return {k: v[:batch] for k, v in ref.items()}


@pytest.fixture(scope="module")
def plain(scaldpc):
    """One decoder per case with settle = 0: what every call is also compared with."""
    decs = {}

    def get(name):
        if name not in decs:
            decs[name] = decoder(R.case(name), settle=0)
        return decs[name]

    yield get
    for d in decs.values():
        d.close()


@pytest.mark.parametrize("group", [0, 2])
@pytest.mark.parametrize("batch", [1, 70, R.BATCH])
def test_sizes_first_and_second_call(scaldpc, plain, batch, group):
    """One codeword; a partial second tile; six tiles, with group 2 three chained groups of two tiles on both lanes.  The
    first call runs without a horizon, the second with the learned one; the report is that of a call that wants posteriors."""
    c = R.case("hqc")
    dec, full, off = decoder(c), decoder(c), plain("hqc")
    for d in (dec, full, off):
        d.set_tile_group(group)
    ref = head(R.oracle_at("hqc", R.MAX_ITER), batch)
    want = R.frozen_at(c.same, 3, R.MAX_ITER, batch=batch)
    assert all(want) == (batch <= 70)  # (two of the six tiles hold a codeword that never settles: their closing pass runs in full)
    for n_call in range(2):
        got = call(dec, c.synd[:batch])
        st = dec.last_settle()
        print(batch, group, n_call, st, want, flush=True)
        same(got, ref, f"oracle, call {n_call}")
        same(got, call(off, c.synd[:batch]), f"settle = 0, call {n_call}")
        assert off.last_settle() == OFF
        llr = call(full, c.synd[:batch], want_llr=True)
        assert (llr["bits"] == got["bits"]).all() and st == full.last_settle()
        assert st["frozen_at"] == want and st["tiles_rerun"] == 0
        if n_call == 0 or not all(want):  # (fewer than 7/8 of the tiles froze: nothing to learn)
            assert st["horizon"] == 0 and st["launches_saved"] == 0
        else:
            assert st["horizon"] == max(want) + 2 and st["launches_saved"] > 0
        if group and batch == R.BATCH:
            assert dec.last_schedule()["fixed_chained"] == 2
    dec.close()
    full.close()
    off.set_tile_group(0)


def test_forced_horizon_reruns_tiles(scaldpc, plain):
    """A horizon of 8, below the largest frozen-at number: the closing pass of a tile that is not frozen by it runs in full
    (on a state that is thrown away), and the tile is decoded again."""
    c = R.case("hqc")
    want = R.frozen_at(c.same, 3, R.MAX_ITER)
    dec, full = decoder(c, settle_horizon=8), decoder(c, settle_horizon=8)
    for d in (dec, full):
        d.set_tile_group(2)
    got = call(dec, c.synd)
    st = dec.last_settle()
    print(st, flush=True)
    same(got, R.oracle_at("hqc", R.MAX_ITER), "oracle")
    same(got, call(plain("hqc"), c.synd), "settle = 0")
    call(full, c.synd, want_llr=True)
    assert st == full.last_settle()
    assert st["horizon"] == 8 and st["launches_saved"] > 0
    assert st["tiles_rerun"] == sum(1 for f in want if not 0 < f <= 8) > 0
    assert st["frozen_at"] == want
    dec.close()
    full.close()


def test_max_iter_across_the_settle_point(scaldpc, plain):
    """max_iter 2 (no test possible), 3 (one test, the first), 4, every value from the smallest settle iteration of the inputs
    - 1 to the largest + 1, and 50: tiles frozen exactly at the last test (their decisions are those of variable pass
    max_iter - 1), tiles that hold settled and unsettled codewords (the closing pass in full)."""
    c = R.case("hqc")
    at = R.settled_at(c.same, 3, R.MAX_ITER)
    lo, hi = int(at[at > 0].min()), int(at.max())
    dec, off = decoder(c), plain("hqc")
    exactly_last = mixed = 0
    for mi in sorted({2, 3, 4, R.MAX_ITER} | set(range(lo - 1, hi + 2))):
        ref = R.oracle_at("hqc", mi)
        got = call(dec, c.synd, mi)
        st = dec.last_settle()
        print(mi, st, flush=True)
        same(got, ref, f"oracle, max_iter {mi}")
        same(got, call(off, c.synd, mi), f"settle = 0, max_iter {mi}")
        want = R.frozen_at(c.same, 3, mi) if mi >= 3 else []
        assert st["frozen_at"] == want and st["horizon"] == 0
        exactly_last += sum(1 for f in want if f == mi)
        for t, f in enumerate(want):
            some = at[t * R.TW : (t + 1) * R.TW]
            mixed += f == 0 and ((some > 0) & (some <= mi)).any()
    assert exactly_last > 0 and mixed > 0
    dec.close()


def test_alpha_schedule(scaldpc, plain):
    """ms_scaling_factor 0: alpha moves until iteration 25, so the passes before test 26 run untracked (and leave their
    columns' decisions all the same); max_iter 20 allows no test, 27 two in which nothing freezes, 50 freezes both tiles."""
    c = R.case("schedule")
    dec = decoder(c)
    for mi in (20, 27, R.MAX_ITER):
        ref = R.oracle_at("schedule", mi)
        got = call(dec, c.synd, mi)
        st = dec.last_settle()
        print(mi, st, flush=True)
        same(got, ref, f"oracle, max_iter {mi}")
        same(got, call(plain("schedule"), c.synd, mi), f"settle = 0, max_iter {mi}")
        first = R.first_test(0.0, mi)
        want = R.frozen_at(c.same, first, mi) if first <= mi else []
        assert st["frozen_at"] == want and st["horizon"] == 0
    dec.close()


def test_regular_graph_never_freezes(scaldpc, plain):
    """settle = 2 on the (3,6)-regular graph: tracked, no tile ever freezes, so every closing pass runs in full."""
    c = R.case("regular")
    ref = R.oracle_at("regular", R.MAX_ITER)
    dec = decoder(c, settle=2)
    for _ in range(2):
        got = call(dec, c.synd)
        same(got, ref, "oracle")
        assert dec.last_settle() == {"frozen_at": [0, 0], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    same(got, call(plain("regular"), c.synd), "settle = 0")
    dec.close()


def test_soft_call(scaldpc, oracle, plain):
    """Per-codeword priors for the check columns: two rows of priors, dealt to the codewords in turn."""
    c = R.case("hqc")
    Rr, batch = c.H.m, 130
    rows = (np.full(Rr, 0.02, dtype=np.float32), np.full(Rr, 0.06, dtype=np.float32))
    cp = np.stack([rows[i % 2] for i in range(batch)])
    ref = None
    for k, row in enumerate(rows):  # one oracle call per row of priors; each codeword takes the results of its own
        probs = np.concatenate([c.probs[: c.H.n - Rr], row.astype(np.float64)])
        r = oracle.bp_decode_batch(c.H, probs, c.synd[:batch], 0, R.MAX_ITER, "min_sum", alpha=1.0, dtype="f32", threads=4,
                                   early_exit=False)
        ref = ref or {key: v.copy() for key, v in r.items()}
        for key in ref:
            ref[key][k::2] = r[key][k::2]
    dec, full = decoder(c), decoder(c)
    for n_call in range(2):
        got = call(dec, c.synd[:batch], channel_probs=cp)
        st = dec.last_settle()
        print(st, flush=True)
        same(got, ref, f"oracle, call {n_call}")
        call(full, c.synd[:batch], want_llr=True, channel_probs=cp)
        assert st == full.last_settle() and len(st["frozen_at"]) == 3
    same(got, call(plain("hqc"), c.synd[:batch], channel_probs=cp), "settle = 0")
    dec.close()
    full.close()


@functools.lru_cache(maxsize=None)
def received_case():
    """Received words [0 | syndrome] of the first 70 trials of the HQC-shaped case, and the oracle on them."""
    from oracle import pyoracle

    c = R.case("hqc")
    recv = np.concatenate([np.zeros((70, c.H.n - c.H.m), dtype=np.uint8), c.synd[:70]], axis=1)
    ref = pyoracle.bp_decode_batch(c.H, c.probs, recv, 1, R.MAX_ITER, "min_sum", alpha=c.alpha, dtype="f32",
                                   threads=max(1, min(8, pyoracle.max_threads())), early_exit=False)
    return recv, ref


def test_received_input(scaldpc, plain):
    """Received words instead of syndromes: the decisions are merged with the received bits on the way out."""
    c = R.case("hqc")
    recv, ref = received_case()
    want = R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    dec = decoder(c)
    for n_call in range(2):
        got = call(dec, recv)
        same(got, ref, f"oracle, call {n_call}")
        assert dec.last_settle()["frozen_at"] == want
    assert dec.last_settle()["horizon"] == max(want) + 2
    same(got, call(plain("hqc"), recv), "settle = 0")
    dec.close()


def test_nothing_carries_over_between_inputs(scaldpc):
    """One handle, syndromes X, then Y, then X, then Y, all in the handle's tile 0.  X freezes at 11 and Y at 6, so Y runs with
    the horizon learned on X and X with the one learned on Y, which is too short for it (the tile is decoded again): the
    decisions a frozen tile keeps are those of THIS call's passes."""
    c = R.case("hqc")
    ref = R.oracle_at("hqc", R.MAX_ITER)
    X, Y = slice(0, 64), slice(320, 323)
    dec, seen = decoder(c), []
    for n_call, sel in enumerate((X, Y, X, Y)):
        got = call(dec, c.synd[sel])
        seen.append(dec.last_settle())
        print(n_call, seen[-1], flush=True)
        same(got, {k: v[sel] for k, v in ref.items()}, f"oracle, call {n_call}")
    assert [s["frozen_at"] for s in seen] == [[11], [6], [11], [6]]
    assert [s["horizon"] for s in seen] == [0, 13, 8, 0] and [s["tiles_rerun"] for s in seen] == [0, 0, 1, 0]
    dec.close()


def test_alternating_want_llr(scaldpc):
    """One handle, want_llr False / True / False / True: the calls that want posteriors run the closing pass in full, and
    their posteriors are the oracle's."""
    c = R.case("hqc")
    ref = head(R.oracle_at("hqc", R.MAX_ITER), 70)
    want = R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    dec = decoder(c)
    for n_call in range(4):
        got = call(dec, c.synd[:70], want_llr=bool(n_call & 1))
        st = dec.last_settle()
        assert st["frozen_at"] == want and st["horizon"] == (max(want) + 2 if n_call else 0) and st["tiles_rerun"] == 0
        if n_call & 1:
            assert (got["llr"].view(np.uint32) == ref["llr"].view(np.uint32)).all()
            assert ((got["llr"] <= 0) == (ref["bits"] != 0)).all()
            got = dict(got, llr=None)
        same(got, ref, f"oracle, call {n_call}")
    dec.close()
