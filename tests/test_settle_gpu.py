"""Settled codewords on the device (fixed-iteration min-sum calls on the record-form kernels, knob `settle`): passes return at
once for tiles whose message state has stopped changing, and a learned horizon keeps them from being enqueued at all.
Every call here is compared with the float32 oracle -- decisions, posteriors, converged flags, iteration counts, bit for bit
-- and with the same call at settle = 0; the device's frozen-at numbers (scaldpc_bp_last_settle) are held to
tests/settle_ref.py.  tests/test_settle_ref.py shows that the inputs contain what the cases below rely on.  The path is
pinned to the 64-codeword-tile kernels."""
import importlib

import numpy as np
import pytest

import settle_ref as R

bp = importlib.import_module("sca-ldpc_amd.bp")

pytestmark = pytest.mark.gpu
OFF = {"frozen_at": [], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}


def decoder(scaldpc, c, *, settle=None, alpha=None, **knobs):
    dec = bp.bp_decoder(c.H, max_iter=R.MAX_ITER, bp_method="min_sum", channel_probs=c.probs,
                        ms_scaling_factor=c.alpha if alpha is None else alpha)
    dec.configure(path="stream", **knobs)
    if settle is not None:
        dec.configure(settle=settle)
    return dec


def same(got, ref, what):
    assert (got["bits"] == ref["bits"]).all(), what
    assert (got["llr"].view(np.uint32) == ref["llr"].view(np.uint32)).all(), what
    assert (got["converged"].astype(np.int32) == ref["converged"].astype(np.int32)).all(), what
    assert (got["iters"] == ref["iters"]).all(), what


def call(dec, synd, max_iter=R.MAX_ITER, **kw):
    return dec.decode_batch(synd, max_iter=max_iter, early_exit=False, want_llr=True, **kw)


@pytest.fixture(scope="module")
def plain(scaldpc):
    """One decoder per case with settle = 0: what every call is also compared with."""
    decs = {}

    def get(name):
        if name not in decs:
            decs[name] = decoder(scaldpc, R.case(name), settle=0)
        return decs[name]

    yield get
    for d in decs.values():
        d.close()


@pytest.mark.parametrize("batch,group", [(70, 0), (R.BATCH, 2)])
def test_sizes(scaldpc, plain, batch, group):
    """A partial second tile; chained groups of two tiles on both lanes.  The first call of a handle runs without a horizon,
    and its frozen-at numbers are the reference's."""
    c = R.case("hqc")
    dec, off = decoder(scaldpc, c), plain("hqc")
    for d in (dec, off):
        d.set_tile_group(group)
    ref = {k: v[:batch] for k, v in R.oracle_at("hqc", R.MAX_ITER).items()}
    want = R.frozen_at(c.same, 3, R.MAX_ITER, batch=batch)
    got = call(dec, c.synd[:batch])
    st = dec.last_settle()
    print(batch, st, want, flush=True)
    same(got, ref, "oracle")
    same(got, call(off, c.synd[:batch]), "settle = 0")
    assert off.last_settle() == OFF
    assert st == {"frozen_at": want, "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    if group:
        assert dec.last_schedule()["fixed_chained"] == 2
    # the second call: a horizon where the rules allow one, the same results, the same numbers
    got2 = call(dec, c.synd[:batch])
    st2 = dec.last_settle()
    print(batch, st2, flush=True)
    same(got2, ref, "second call")
    assert st2["frozen_at"] == want
    if all(want):
        assert st2["horizon"] == max(want) + 2 and st2["launches_saved"] > 0 and st2["tiles_rerun"] == 0
    else:
        assert st2["horizon"] == 0  # fewer than 7/8 of the tiles froze: nothing to learn
    dec.close()
    off.set_tile_group(0)


def test_max_iter_across_the_settle_point(scaldpc, plain):
    """max_iter 2, 3, 4, every value from the smallest settle iteration of the inputs - 1 to the largest + 1, and 50: the
    middle values stop with tiles that hold settled and unsettled codewords."""
    c = R.case("hqc")
    at = R.settled_at(c.same, 3, R.MAX_ITER)
    lo, hi = int(at[at > 0].min()), int(at.max())
    dec, off = decoder(scaldpc, c), plain("hqc")
    for mi in sorted({2, 3, 4, R.MAX_ITER} | set(range(lo - 1, hi + 2))):
        ref = R.oracle_at("hqc", mi)
        got = call(dec, c.synd, mi)
        st = dec.last_settle()
        print(mi, st, flush=True)
        same(got, ref, f"oracle, max_iter {mi}")
        same(got, call(off, c.synd, mi), f"settle = 0, max_iter {mi}")
        assert st["frozen_at"] == (R.frozen_at(c.same, 3, mi) if mi >= 3 else []) and st["horizon"] == 0
    dec.close()


def test_regular_graph_never_freezes(scaldpc, plain):
    """The (3,6)-regular graph has no column of degree 1: by default a handle on it does not track at all; with settle = 2
    given, no tile ever freezes, nothing is skipped and no horizon is learned."""
    c = R.case("regular")
    ref = R.oracle_at("regular", R.MAX_ITER)
    auto = decoder(scaldpc, c)
    same(call(auto, c.synd), ref, "oracle, default")
    assert auto.last_settle() == OFF
    auto.close()
    dec = decoder(scaldpc, c, settle=2)
    for _ in range(2):  # (the second call: nothing was learned, no horizon)
        got = call(dec, c.synd)
        same(got, ref, "oracle")
        assert dec.last_settle() == {"frozen_at": [0, 0], "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    same(got, call(plain("regular"), c.synd), "settle = 0")
    dec.close()


def test_forced_horizon_reruns_tiles(scaldpc, plain):
    """A horizon of 8, below the largest frozen-at number: the tiles it is wrong for are decoded again."""
    c = R.case("hqc")
    want = R.frozen_at(c.same, 3, R.MAX_ITER)
    dec = decoder(scaldpc, c, settle_horizon=8)
    dec.set_tile_group(2)
    got = call(dec, c.synd)
    st = dec.last_settle()
    print(st, flush=True)
    same(got, R.oracle_at("hqc", R.MAX_ITER), "oracle")
    same(got, call(plain("hqc"), c.synd), "settle = 0")
    assert st["horizon"] == 8 and st["launches_saved"] > 0
    assert st["tiles_rerun"] == sum(1 for f in want if not 0 < f <= 8) > 0
    assert st["frozen_at"] == want  # (re-run tiles report what their re-run found)
    dec.close()


def test_alpha_schedule(scaldpc, plain):
    """ms_scaling_factor 0: alpha moves until iteration 25, so no test before 26."""
    c = R.case("schedule")
    dec = decoder(scaldpc, c)
    for mi in (20, 27, R.MAX_ITER):
        ref = R.oracle_at("schedule", mi)
        got = call(dec, c.synd, mi)
        st = dec.last_settle()
        print(mi, st, flush=True)
        same(got, ref, f"oracle, max_iter {mi}")
        same(got, call(plain("schedule"), c.synd, mi), f"settle = 0, max_iter {mi}")
        first = R.first_test(0.0, mi)
        assert st["frozen_at"] == (R.frozen_at(c.same, first, mi) if first <= mi else []) and st["horizon"] == 0
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
    # the restatement on the codewords' own priors (held to the oracle here, as tests/test_settle_ref.py does for the rest)
    prior = np.stack([R.prior_llr(np.concatenate([c.probs[: c.H.n - Rr], rows[i % 2].astype(np.float64)])) for i in range(2)])
    out = R.run(c.H, prior[np.arange(batch) % 2], c.synd[:batch], R.MAX_ITER, 1.0)
    assert (out["post"][R.MAX_ITER].view(np.uint32) == ref["llr"].view(np.uint32)).all()
    want = R.frozen_at(out["same"], 3, R.MAX_ITER)
    K = max(want) + 2
    K = K if 8 * sum(1 for f in want if f) >= 7 * len(want) and 2 * K < R.MAX_ITER else 0
    dec = decoder(scaldpc, c)
    for n_call in range(2):
        got = call(dec, c.synd[:batch], channel_probs=cp)
        st = dec.last_settle()
        print(st, want, K, flush=True)
        same(got, ref, f"oracle, call {n_call}")
        assert st["frozen_at"] == want and st["horizon"] == (K if n_call else 0) and st["tiles_rerun"] == 0
    same(got, call(plain("hqc"), c.synd[:batch], channel_probs=cp), "settle = 0")
    dec.close()


def test_handle_reused(scaldpc, oracle):
    """Call (learns), call (horizon in force), new priors (the learning starts over), call, call."""
    c = R.case("hqc")
    synd, want = c.synd[:70], R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    ref = {k: v[:70] for k, v in R.oracle_at("hqc", R.MAX_ITER).items()}
    dec, off = decoder(scaldpc, c), decoder(scaldpc, c, settle=0)
    seen = []
    for _ in range(2):
        got = call(dec, synd)
        same(got, ref, "oracle")
        same(got, call(off, synd), "settle = 0")
        seen.append(dec.last_settle())
    probs2 = np.where(np.arange(c.H.n) < c.H.n - c.H.m, c.probs, 0.03)
    dec.update_channel_probs(probs2)
    off.update_channel_probs(probs2)
    ref2 = oracle.bp_decode_batch(c.H, probs2, synd, 0, R.MAX_ITER, "min_sum", alpha=1.0, dtype="f32", threads=4, early_exit=False)
    for _ in range(2):
        got = call(dec, synd)
        same(got, ref2, "oracle, new priors")
        same(got, call(off, synd), "settle = 0, new priors")
        seen.append(dec.last_settle())
    print(seen, flush=True)
    assert seen[0] == {"frozen_at": want, "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    assert seen[1]["horizon"] == max(want) + 2 and seen[1]["launches_saved"] > 0 and seen[1]["frozen_at"] == want
    assert seen[2]["horizon"] == 0 and seen[2]["launches_saved"] == 0  # learning reset
    if all(seen[2]["frozen_at"]):
        assert seen[3]["horizon"] == max(seen[2]["frozen_at"]) + 2
    dec.close()
    off.close()


def test_device_side_skipping_only(scaldpc, plain):
    """settle = 1: every call tracks and skips on the device, none learns a horizon."""
    c = R.case("hqc")
    synd, want = c.synd[:70], R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    ref = {k: v[:70] for k, v in R.oracle_at("hqc", R.MAX_ITER).items()}
    dec = decoder(scaldpc, c, settle=1)
    for _ in range(3):
        got = call(dec, synd)
        same(got, ref, "oracle")
        assert dec.last_settle() == {"frozen_at": want, "launches_saved": 0, "tiles_rerun": 0, "horizon": 0}
    same(got, call(plain("hqc"), synd), "settle = 0")
    dec.close()


@pytest.mark.parametrize("env,first", [({"SCALDPC_SETTLE": "0"}, None), ({"SCALDPC_SETTLE": "1"}, 0),
                                       ({"SCALDPC_SETTLE_HORIZON": "8"}, 8)])  # fmt: skip
def test_environment_defaults(scaldpc, plain, monkeypatch, env, first):
    """A new handle takes `settle` and `settle_horizon` from the environment, once, at creation."""
    c = R.case("hqc")
    synd, want = c.synd[:70], R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    ref = {k: v[:70] for k, v in R.oracle_at("hqc", R.MAX_ITER).items()}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dec = decoder(scaldpc, c)
    for k in env:
        monkeypatch.delenv(k)
    for _ in range(2):
        got = call(dec, synd)
        same(got, ref, "oracle")
        st = dec.last_settle()
        print(env, st, flush=True)
        if first is None:
            assert st == OFF
        else:
            assert st["frozen_at"] == want and st["horizon"] == first
            assert st["tiles_rerun"] == sum(1 for f in want if first and not 0 < f <= first)
    same(got, call(plain("hqc"), synd), "settle = 0")
    dec.close()


def test_time_kernels_runs_full_passes(scaldpc, plain):
    """After a settled decode scaldpc_bp_time_kernels still launches full passes: its launch counts are those of settle = 0,
    and the next decode is what it was."""
    c = R.case("hqc")
    synd = c.synd[:128]
    ref = {k: v[:128] for k, v in R.oracle_at("hqc", R.MAX_ITER).items()}
    dec, off = decoder(scaldpc, c), plain("hqc")
    out = []
    for d in (dec, off):
        same(call(d, synd), ref, "oracle")
        kt = d.time_kernels(3)
        out.append({k: v for k, v in kt.items() if not k.startswith("ms_")})
        assert kt["ms_check"] > 0 and kt["ms_var"] > 0
    assert any(dec.last_settle()["frozen_at"])
    assert out[0] == out[1]
    same(call(dec, synd), ref, "after time_kernels")
    dec.close()
