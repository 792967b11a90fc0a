"""The sparse settle gate on the device (knob `settle_sparse`): in a tracked fixed-iteration min-sum call a check pass returns
for the rows none of whose columns ran in the variable pass before, and a variable pass for the columns none of whose
messages changed.  Every call here is held, bit for bit, to the float32 oracle (decisions, converged flags, iteration counts,
posteriors where asked) and to a twin handle with settle_sparse = 0 on the same inputs, whose report (scaldpc_bp_last_settle)
it must equal; and after every call the gate's two tables, exported per tile (scaldpc_bp_debug_sparse_flags), are the ones
tests/settle_sparse_ref.py predicts -- every node's last stamp is the last pass in which the rule lets it run, every dirty
mask is equal -- which shows that the gate engaged and that it is the rule.  tests/test_settle_sparse.py shows on the CPU that
the rule is conservative on these inputs and that they hold passes in which some but not all nodes run.  All calls run 50
iterations on the 64-codeword-tile kernels."""
import functools
import importlib

import numpy as np
import pytest

import rec_wide_cases as W
import settle_matrix_cases as MC
import settle_ref as R
import settle_sparse_ref as SP

bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")

pytestmark = pytest.mark.gpu
ITER = R.MAX_ITER


def decoder(H, probs, alpha=1.0, *, sparse=None, group=0, **knobs):
    dec = bp.bp_decoder(H, max_iter=ITER, bp_method="min_sum", channel_probs=probs, ms_scaling_factor=alpha)
    dec.configure(path="stream", **knobs)
    if sparse is not None:
        dec.configure(settle_sparse=sparse)
    dec.set_tile_group(group)
    return dec


def same(got, ref, what):
    assert (got["bits"] == ref["bits"]).all(), what
    if got.get("llr") is not None:
        assert (got["llr"].view(np.uint32) == ref["llr"].view(np.uint32)).all(), what
    assert (got["converged"].astype(np.int32) == ref["converged"].astype(np.int32)).all(), what
    assert (got["iters"] == ref["iters"]).all(), what


def call(dec, synd, want_llr, **kw):
    return dec.decode_batch(synd, max_iter=ITER, early_exit=False, want_llr=want_llr, **kw)


class Model:
    """One trace of the restatement and, per tile, the tables the rule leaves (computed once per case)."""

    def __init__(self, H, prior, synd, alpha=1.0, wide=False):
        self.tr = SP.trace(H, prior, synd, ITER, alpha)
        self.batch, self.first, self.wide = synd.shape[0], R.first_test(alpha, ITER), wide
        self.acts = {}

    def act(self, tile, start=0):
        start = max(start, self.first)
        if (tile, start) not in self.acts:
            self.acts[tile, start] = SP.activity(self.tr, tile, self.batch, self.first, wide=self.wide, start=start)
        return self.acts[tile, start]

    def holds(self, flags, what, start=0):
        tiles = (self.batch + 63) // 64
        assert len(flags) == tiles, (what, len(flags))
        for t, f in enumerate(flags):
            a = self.act(t, start)
            assert np.array_equal(f["col_flag"], a.col_flag), (what, "col_flag", t, np.flatnonzero(f["col_flag"] != a.col_flag)[:8])
            assert np.array_equal(f["row_stamp"], a.row_stamp), (what, "row stamp", t, np.flatnonzero(f["row_stamp"] != a.row_stamp)[:8])
            assert np.array_equal(f["row_dirty"], a.row_dirty), (what, "row dirty", t, np.flatnonzero(f["row_dirty"] != a.row_dirty)[:8])


def held(dec, twin, model, synd, ref, want_llr, what, prev=None, **kw):
    """One call of the handle and of its twin: the oracle's results, the twin's results and report, the model's tables.
    prev = the report of the handle's call before on the same priors, max_iter and alpha (None = it learns): the call gates
    from the start learned there (settle_sparse_ref.next_start), which the device reports and the model is run with."""
    got, plain = call(dec, synd, want_llr, **kw), call(twin, synd, want_llr, **kw)
    st = dec.last_settle()
    print(what, want_llr, st, flush=True)
    same(got, ref, f"oracle, {what}")
    same(got, plain, f"settle_sparse = 0, {what}")
    assert st == twin.last_settle(), what
    assert st["frozen_at"] == [model.act(t).frozen_at for t in range(len(st["frozen_at"]))], what
    start = max(SP.next_start(prev and prev["frozen_at"], model.first), model.first)
    assert dec.debug_sparse_start() == start, (what, dec.debug_sparse_start(), start)
    model.holds(dec.debug_sparse_flags(), what, start)
    assert twin.debug_sparse_flags() == [] and twin.debug_sparse_start() == 0, what
    return st


@functools.lru_cache(maxsize=None)
def hqc_model():
    c = R.case("hqc")
    return Model(c.H, R.prior_llr(c.probs), c.synd)


# ------------------------------------------------------------------------------------------- the 150 x 650 graph, three calls
@pytest.mark.parametrize("want_llr", [True, False])
def test_three_calls(scaldpc, oracle, want_llr):
    """323 codewords: tiles 0, 2 and 4 thin out and stop, tiles 1 and 3 cycle to the end, tile 5 holds 3 codewords.  The handle
    learns; runs under what it learned; runs under a forced horizon of 8, which decodes tiles 1 and 3 (and every tile frozen
    later than 8) again -- after the tables of those tiles were cleared: the re-run meets the same stamps otherwise."""
    c, model = R.case("hqc"), hqc_model()
    ref = R.oracle_at("hqc", ITER)
    dec, twin = decoder(c.H, c.probs, group=2), decoder(c.H, c.probs, sparse=0, group=2)
    st = held(dec, twin, model, c.synd, ref, want_llr, "learns")
    st = held(dec, twin, model, c.synd, ref, want_llr, "learned horizon and start", prev=st)
    assert dec.debug_sparse_start() == min(f for f in st["frozen_at"] if f) - 2 > model.first  # (a later start than the first test)
    for d in (dec, twin):
        d.configure(settle_horizon=8)
    st = held(dec, twin, model, c.synd, ref, want_llr, "short horizon", prev=st)
    assert st["horizon"] == 8 and st["tiles_rerun"] >= 2
    dec.close()
    twin.close()


@pytest.mark.parametrize("split,group", [(2, 4), (1, 2), (3, 6)])
def test_launch_shapes(scaldpc, oracle, split, group):
    """Two tiles per launch on two lanes (the XCD map), one lane (the column records heaviest first), three lanes."""
    c, model = R.case("hqc"), hqc_model()
    ref = R.oracle_at("hqc", ITER)
    dec, twin = decoder(c.H, c.probs, group=group, split=split), decoder(c.H, c.probs, sparse=0, group=group, split=split)
    st = held(dec, twin, model, c.synd, ref, False, f"split {split} group {group}")
    for d in (dec, twin):
        d.configure(settle_horizon=8)
    held(dec, twin, model, c.synd, ref, True, f"split {split} group {group}, short horizon", prev=st)
    dec.close()
    twin.close()


# ------------------------------------------------------------------------------------------------------------ the kernel ladder
@pytest.mark.parametrize("name", ["row32", "row64", "ties32", "ties64"])
def test_kernel_ladder(scaldpc, oracle, name):
    """Rows of 18 and 34 edges -- the 32- and 64-edge builds of the check kernel, whose compare sits elsewhere -- and the tie
    inputs, where a row's only change is often its arg-min index."""
    c = MC.case(name)
    model = Model(c.H, R.prior_llr(c.probs), c.synd)
    dec, twin = decoder(c.H, c.probs), decoder(c.H, c.probs, sparse=0)
    held(dec, twin, model, c.synd, MC.oracle_of(name), True, name)
    dec.close()
    twin.close()


def test_wide_column(scaldpc, oracle):
    """minsum_rec = 2 on a graph with a column of 40 edges: the wide launch is never gated and always stamps."""
    c = W.settle_case()
    ref = oracle.bp_decode_batch(c.H, c.probs, c.synd, 0, ITER, "min_sum", alpha=1.0, dtype="f32", threads=8, early_exit=False)
    model = Model(c.H, R.prior_llr(c.probs), c.synd, wide=True)
    dec, twin = decoder(c.H, c.probs, minsum_rec=2), decoder(c.H, c.probs, sparse=0, minsum_rec=2)
    held(dec, twin, model, c.synd, ref, True, "wide")
    wide = int(np.flatnonzero(np.diff(np.asarray(c.H.col_ptr)) >= SP.WIDE_FROM)[0])
    assert model.act(1).frozen_at == 0 and dec.debug_sparse_flags()[1]["col_flag"][wide] == (ITER - 1) << 1
    dec.close()
    twin.close()


def test_own_sign_changed_rule(scaldpc, oracle):
    """settle_sparse_ref.own_case: the codeword alone in tile 1 has columns that run through their own sign_changed bit and
    nothing else (tests/test_settle_sparse.py counts them); a gate without that term leaves other tables and other results."""
    c = SP.own_case()
    ref = oracle.bp_decode_batch(c.H, c.probs, c.synd, 0, ITER, "min_sum", alpha=1.0, dtype="f32", threads=4, early_exit=False)
    model = Model(c.H, R.prior_llr(c.probs), c.synd)
    dec, twin = decoder(c.H, c.probs, sparse=1, settle=2), decoder(c.H, c.probs, sparse=0, settle=2)
    st = None
    for want_llr in (True, False):
        st = held(dec, twin, model, c.synd, ref, want_llr, "own sign", prev=st)
        assert st["frozen_at"] == [0, 0]  # (nothing froze: the second call gates from the first test again)
    dec.close()
    twin.close()


def test_soft_call(scaldpc, oracle):
    """Per-codeword priors for the check columns of col32, two rows dealt to 130 codewords in turn."""
    c, s = MC.case("col32"), MC.soft()
    Rr, n = c.H.m, c.H.n
    prior = np.stack([R.prior_llr(np.concatenate([c.probs[: n - Rr], r.astype(np.float64)])) for r in s.rows])
    model = Model(c.H, prior[np.arange(MC.SOFT_BATCH) % 2], s.synd)
    dec, twin = decoder(c.H, c.probs), decoder(c.H, c.probs, sparse=0)
    st = None
    for what in ("learns", "second call"):
        st = held(dec, twin, model, s.synd, MC.soft_oracle(), True, f"soft, {what}", prev=st, channel_probs=s.cp)
    dec.close()
    twin.close()


def test_growing_handle(scaldpc, oracle):
    """100 rows, then append_rows of the other 50 with their identity columns: the tables are laid out again for the graph as
    it is."""
    first, grown = MC.case("base100"), MC.case("grown")
    dec, twin = decoder(first.H, first.probs), decoder(first.H, first.probs, sparse=0)
    held(dec, twin, Model(first.H, R.prior_llr(first.probs), first.synd), first.synd, MC.oracle_of("base100"), True, "100 rows")
    rp = np.asarray(grown.H.row_ptr)[MC.GROW_FIRST :].astype(np.int64)
    ci = np.asarray(grown.H.col_idx)[rp[0] : rp[-1]].astype(np.int32)
    for d in (dec, twin):
        d.append_rows((rp - rp[0]).astype(np.int32), ci, grown.H.n, grown.probs[first.H.n :])
        d.update_channel_probs(grown.probs)
    held(dec, twin, Model(grown.H, R.prior_llr(grown.probs), grown.synd), grown.synd, MC.oracle_of("grown"), False, "150 rows")
    dec.close()
    twin.close()


def test_asynchronous_device_call(scaldpc, oracle):
    """An SCALDPC_F_ASYNC call gates on the device alone: no read-back, no report; after a stream synchronise its outputs are
    the oracle's and those of a twin with settle_sparse = 0, and its tables the model's."""
    import torch

    c = MC.case("grown")
    ref = MC.oracle_of("grown")
    model = Model(c.H, R.prior_llr(c.probs), c.synd)
    batch, n = c.synd.shape[0], c.H.n
    stream = torch.cuda.Stream()
    got = {}
    for name, dec in (("gate", decoder(c.H, c.probs)), ("twin", decoder(c.H, c.probs, sparse=0))):
        with torch.cuda.stream(stream):
            d_in = torch.from_numpy(c.synd).cuda()
            out = dict(bits=torch.full((batch, n), 0xAA, dtype=torch.uint8, device="cuda"),
                       llr=torch.full((batch, n), float("nan"), dtype=torch.float32, device="cuda"),
                       iters=torch.full((batch,), -7, dtype=torch.int32, device="cuda"),
                       converged=torch.full((batch,), 0xAA, dtype=torch.uint8, device="cuda"))
            stream.synchronize()
            dec.decode_batch_device(d_in.data_ptr(), lib.IN_SYNDROME, batch, out["bits"].data_ptr(), max_iter=ITER, early_exit=False,
                                    stream=stream.cuda_stream, d_out_llr=out["llr"].data_ptr(), d_out_iters=out["iters"].data_ptr(),
                                    d_out_conv=out["converged"].data_ptr(), asynchronous=True)
            assert dec.last_settle()["frozen_at"] == []
            stream.synchronize()
            got[name] = {k: v.cpu().numpy() for k, v in out.items()}
        same(got[name], ref, f"oracle, asynchronous, {name}")
        if name == "gate":
            assert dec.debug_sparse_start() == model.first
            model.holds(dec.debug_sparse_flags(), "asynchronous")
        else:
            assert dec.debug_sparse_flags() == []
        dec.close()
    same(got["gate"], got["twin"], "settle_sparse = 0, asynchronous")


def test_alpha_schedule(scaldpc, oracle):
    """ms_scaling_factor 0: alpha moves until iteration 25; nothing is tracked, stamped or gated before the first test."""
    c = R.case("schedule")
    model = Model(c.H, R.prior_llr(c.probs), c.synd, alpha=0.0)
    assert model.first == c.first > 20
    dec, twin = decoder(c.H, c.probs, 0.0), decoder(c.H, c.probs, 0.0, sparse=0)
    held(dec, twin, model, c.synd, R.oracle_at("schedule", ITER), True, "schedule")
    f = dec.debug_sparse_flags()[0]
    assert f["row_stamp"][f["row_stamp"] > 0].min() >= c.first and (f["col_flag"][f["col_flag"] > 0] >> 1).min() >= c.first - 1
    dec.close()
    twin.close()
