"""Monte-Carlo trials of DecoderSpecial on drawn secrets on the GPU (scaldpc_mc_qary_run_secret; QarySpecialDecoder.mc_run_secret).
Secrets and outcomes are held to the trial law restated on the oracle's Philox words (tests/qary_secret_ref.py), the symbols to
the CPU oracle AND to the decoder's own plain call on the materialised input -- the entry's defining property -- in every kernel
form the plan can choose and at any split of the trials into calls; the per-trial results follow from the arrays."""
import ctypes as C
import functools
import importlib
import json
import os

import numpy as np
import pytest

import qary_secret_ref as ref
from helpers import S
from oracle import pyoracle

pytestmark = pytest.mark.gpu
qary = importlib.import_module("sca-ldpc_amd.qary")
trials = importlib.import_module("sca-ldpc_amd.trials")
lib = importlib.import_module("sca-ldpc_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("success", "wrong", "channel_wrong", "secret", "levels", "symbols")
DTYPES = dict(success=np.uint8, wrong=np.int32, channel_wrong=np.int32, secret=np.int8, levels=np.uint8, symbols=np.int8)


def same(got, want, rows=slice(None), what=""):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k][rows]), (what, k)


class Case:
    """A graph, a prior and two tables; `run` is mc_run_secret with every output, `restated` the law on the CPU."""

    def __init__(self, H, B, BSUM, prior, tb, ts, seed):
        self.H, self.B, self.BSUM, self.prior, self.seed = H, B, BSUM, prior, seed
        self.R, self.N = H.shape
        self.BV = self.N - self.R
        self.lb, self.wb = tb["levels"].astype(np.float32), tb["weights"]
        self.ls, self.ws = ts["levels"].astype(np.float32), ts["weights"]

    def run(self, dec, batch, first=0, seed=None, **want):
        want = want or dict(want_secret=True, want_levels=True, want_symbols=True)
        return dec.mc_run_secret(batch, self.seed if seed is None else seed, self.prior, self.lb, self.wb, self.ls, self.ws, first_trial=first, **want)

    def restated(self, batch, first=0):
        secret, levels = ref.draw(self.H, self.B, self.BSUM, self.seed, first, batch, self.prior, self.wb, self.ws)
        assert not (self.H.astype(np.int64) @ secret.T.astype(np.int64)).any()  # every drawn word is a code word
        return secret, levels

    def pmf(self, levels):
        return self.lb[levels[:, : self.BV]], self.ls[levels[:, self.BV :]]

    def follows(self, res):
        """success, wrong and channel_wrong as secret, levels and symbols define them, and every dtype."""
        want = ref.results(res["secret"], res["levels"], res["symbols"], self.BV, self.lb, self.ls, self.B, self.BSUM)
        for k in want:
            assert np.array_equal(res[k], want[k]), k
        assert all(res[k].dtype == DTYPES[k] for k in KEYS)
        assert res["wrong"].shape == res["channel_wrong"].shape == (len(res["success"]), 2)


# ------------------------------------------------------------------------------------- 1. the 32 x 80 graph at accuracy 0.95
SEED1, FIRST1, RUNS1 = 99, 1000, 70
RECOVERED1 = 26  # of 70, counted on the CPU (qary_secret_ref + the oracle) before the first GPU run; the band asked for is 10 .. 60


def graph1():
    return S.codes.make_qary_qc_graph(16, 3, 3, S.codes.make_random_state(0), 2)  # 32 x 80, row weight 4, entries +-1


@functools.lru_cache(maxsize=None)
def case1():
    """The case, its restated secrets and levels and the oracle's symbols -- computed once, shared, never modified."""
    g = graph1()
    prior = trials.centered_binomial(2)
    tb = trials.oracle_posterior_table(ref.SHARED_5, prior, 0.95)  # two symbols share a code word
    ts = trials.oracle_posterior_table(ref.expansion(13, 4), trials.centered_binomial(2, 3), 0.95, reverse=True)
    c = Case(g.to_dense(np.int8), 2, 6, prior, tb, ts, SEED1)
    secret, levels = c.restated(RUNS1, FIRST1)
    sym = pyoracle.qary_special_batch(g, 2, 6, *c.pmf(levels), 4, threads=8)
    for a in (secret, levels, sym):
        a.setflags(write=False)
    return c, secret, levels, sym


def test_first_graph_secret_levels_symbols_and_results():
    c, secret, levels, sym = case1()
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    res = c.run(dec, RUNS1, FIRST1)
    assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels)
    assert np.array_equal(res["symbols"], sym) and np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    c.follows(res)
    assert 10 <= int(res["success"].sum()) <= 60 and int(res["success"].sum()) == RECOVERED1  # both outcomes
    assert res["channel_wrong"][:, 0].sum() > res["wrong"][:, 0].sum() > 0  # the sum checks resolve what the rows alone leave
    # the outputs that were not asked for are not there, the others do not change
    same(c.run(dec, RUNS1, FIRST1, want_levels=False), {k: res[k] for k in KEYS[:3]}, what="results only")
    a, b = c.run(dec, 33, FIRST1), c.run(dec, 37, FIRST1 + 33)
    same({k: np.concatenate([a[k], b[k]]) for k in KEYS}, res, what="33 + 37")
    for nb in (1, 64, 65):
        same(c.run(dec, nb, FIRST1), res, slice(0, nb), f"batch {nb}")
    other = c.run(dec, 64, FIRST1, seed=SEED1 + (1 << 32))
    assert not np.array_equal(other["secret"], secret[:64]) and not np.array_equal(other["levels"], levels[:64])
    for kn in (dict(wave=0), dict(dp_any=1), dict(var_small=0, llr_tiled=0)):
        dec.configure(**kn)
        same(c.run(dec, RUNS1, FIRST1), res, what=str(kn))
    dec.close()


# ----------------------------------------------------------------------------------- 2. rows beyond 8 edges, QS = 37, N - R = 22
def long_rows_H():
    """7 x 29 = [H' | +-I]: rows of 9, 9, 8, 9, 3, 0 and 1 coefficient edges over 22 coefficient variables (no multiple of 4: the
    Philox block of variables 20 .. 23 straddles the two tables), identity entries -1 in rows 1 and 4."""
    rng = np.random.RandomState(52)
    coeffs, BV = [9, 9, 8, 9, 3, 0, 1], 22
    R = len(coeffs)
    H = np.zeros((R, BV + R), dtype=np.int8)
    for r, k in enumerate(coeffs):
        H[r, rng.choice(BV, k, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), size=k)
        H[r, BV + r] = -1 if r in (1, 4) else 1
    return H


@functools.lru_cache(maxsize=None)
def case2():
    prior = trials.centered_binomial(2)
    tb = trials.oracle_posterior_table(ref.expansion(5, 3), prior, 0.9)
    # 37 row-sum symbols on five oracle bits: the index modulo 32 (the five outermost values share code words), 32 outcomes
    ts = trials.oracle_posterior_table([ref.expansion(32, 5)[s & 31] for s in range(37)], trials.centered_binomial(2, 9), 0.95, reverse=True)
    assert ts["levels"].shape == (32, 37) and tb["levels"].shape == (8, 5)
    return Case(long_rows_H(), 2, 18, prior, tb, ts, 2024)


def long_rows_decoder(c, iterations=2):
    return qary.decoder_class(f"DecoderN{c.N}R{c.R}SW9B2")(c.H, iterations)


def test_rows_beyond_eight_edges_and_a_block_that_straddles_the_tables():
    c = case2()
    assert c.BV == 22 and (c.H[:, :22] != 0).sum(axis=1).tolist() == [9, 9, 8, 9, 3, 0, 1] and (c.H[[1, 4], [23, 26]] == -1).all()
    dec = long_rows_decoder(c)
    res = c.run(dec, 70)
    secret, levels = c.restated(70)
    assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels)
    assert (res["secret"][:, 22 + 5] == 0).all() and np.abs(res["secret"][:, 22:]).max() > 6  # the row without coefficient edges: t = 0
    assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    few = pyoracle.qary_special_batch(S.TannerGraph.from_dense(c.H), 2, 18, *(p[:3] for p in c.pmf(levels)), 2, threads=4)
    assert np.array_equal(res["symbols"][:3], few)
    c.follows(res)
    dec.close()


# ------------------------------------------------------------------------------------ 3. trial indices crossing 2^32 in a batch
def test_trial_indices_crossing_two_to_the_32():
    c = case2()
    first = (1 << 32) - 30
    dec = long_rows_decoder(c)
    res = c.run(dec, 70, first)
    secret, levels = c.restated(70, first)
    assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels)
    assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    c.follows(res)
    same(c.run(dec, 40, first + 30), res, slice(30, 70), "from 2^32 on")
    assert not np.array_equal(c.run(dec, 40, 0)["secret"], res["secret"][30:])  # the high word of the index counts
    dec.close()


# ------------------------------------------------------------------------------------------------------------ 4. the reduction
def test_a_point_mass_prior_and_equal_rows_are_mc_run():
    c, _, _, _ = case1()
    wb, ws = np.array([0.04, 0.0, 0.9, 0.06]), np.full(16, 0.1 / 15)  # mostly the answers that are the code words of the value 0
    ws[6] = 0.9
    point = np.array([0.0, 0.0, 1.0, 0.0, 0.0])
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    got = dec.mc_run_secret(RUNS1, SEED1, point, c.lb, np.tile(wb, (5, 1)), c.ls, np.tile(ws, (13, 1)), first_trial=FIRST1, want_secret=True,
                            want_levels=True, want_symbols=True)
    plain = dec.mc_run(RUNS1, SEED1, c.lb, wb, c.ls, ws, first_trial=FIRST1, want_levels=True, want_symbols=True)
    assert not got["secret"].any()
    assert np.array_equal(got["levels"], plain["levels"]) and np.array_equal(got["symbols"], plain["symbols"])
    assert np.array_equal(got["wrong"].sum(axis=1), plain["wrong"]) and np.array_equal((got["wrong"].sum(axis=1) == 0).astype(np.uint8), plain["success"])
    assert 0 < plain["success"].sum() < RUNS1 and 1 not in got["levels"][:, :48]
    dec.close()


# ----------------------------------------------------------------------------------- 5. accuracy 1.0 with an injective coding
def test_a_perfect_oracle_recovers_every_key():
    """Rows of weights 0 and 1, one-hot levels: every LLR row is 0 at the secret and +inf elsewhere."""
    c1, _, _, _ = case1()
    prior = trials.centered_binomial(2)
    tb = trials.oracle_posterior_table(ref.expansion(5, 3), prior, 1.0)
    ts = trials.oracle_posterior_table(ref.expansion(13, 4), trials.centered_binomial(2, 3), 1.0, reverse=True)
    assert (tb["weights"] == 0).sum() == 20 and (ts["levels"] == 0).sum() == 13 * 12
    c = Case(c1.H, 2, 6, prior, tb, ts, 5)
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    with np.errstate(divide="ignore"):
        res = c.run(dec, 70)
        secret, levels = c.restated(70)
        assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels)
        assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    assert res["success"].all() and not res["wrong"].any() and not res["channel_wrong"].any()
    assert np.array_equal(res["symbols"], secret) and len(np.unique(secret[:, :48])) == 5
    dec.close()


# -------------------------------------------------------------------------------------------------------- 6. the Kyber shape
def test_kyber_shape():
    with open(os.path.join(ROOT, "tests", "golden", "generators.json")) as fh:
        g = S.TannerGraph.from_coo(json.load(fh)["qary_qc_256_6_3_s0_cb2"])
    prior = trials.centered_binomial(2)
    tb = trials.oracle_posterior_table(ref.expansion(5, 3), prior, 0.95)
    ts = trials.oracle_posterior_table(ref.expansion(25, 5), trials.centered_binomial(2, 6), 0.95, reverse=True)
    c = Case(g.to_dense(np.int8), 2, 12, prior, tb, ts, 31)
    assert (c.N, c.R) == (1280, 512)
    dec = qary.decoder_class("DecoderN1280R512SW6")(c.H, 2)
    res = c.run(dec, 8, 17)
    secret, levels = c.restated(8, 17)
    assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels)
    assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    c.follows(res)
    for kn in (dict(dp=0, tree=1), dict(dp=1, dp_min=1)):  # the tree walk and the min-plus recursion both see it
        dec.configure(**kn)
        same(c.run(dec, 8, 17), res, what=str(kn))
        assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels))), kn
    dec.close()


# --------------------------------------------------------------------------------------------------------- 7. device pointers
def test_device_pointers_against_the_host_call():
    import torch

    def tensors(batch, N):
        fill = dict(success=7, wrong=-1, channel_wrong=-1, secret=9, levels=9, symbols=9)
        shape = dict(success=(batch,), wrong=(batch, 2), channel_wrong=(batch, 2), secret=(batch, N), levels=(batch, N), symbols=(batch, N))
        return {k: torch.full(shape[k], fill[k], dtype=getattr(torch, np.dtype(DTYPES[k]).name), device="cuda") for k in KEYS}

    stream = torch.cuda.current_stream().cuda_stream
    c, _, _, _ = case1()
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    host = c.run(dec, RUNS1, FIRST1)
    t = tensors(RUNS1, 80)
    dec.mc_run_secret_device(RUNS1, SEED1, c.prior, c.lb, c.wb, c.ls, c.ws, *(t[k].data_ptr() for k in KEYS), first_trial=FIRST1, stream=stream)
    same({k: t[k].cpu().numpy() for k in KEYS}, host, what="every output")
    t = tensors(RUNS1, 80)
    dec.mc_run_secret_device(RUNS1, SEED1, c.prior, c.lb, c.wb, c.ls, c.ws, t["success"].data_ptr(), first_trial=FIRST1)  # the required one alone
    assert np.array_equal(t["success"].cpu().numpy(), host["success"])
    assert (t["wrong"].cpu().numpy() == -1).all() and (t["channel_wrong"].cpu().numpy() == -1).all()
    assert all((t[k].cpu().numpy() == 9).all() for k in ("secret", "levels", "symbols"))
    dec.close()


# ---------------------------------------------------------------------------------------------- the largest table a launch keeps
def test_the_largest_tables_that_fit_the_lds_of_a_launch():
    """B = 63, rows of two coefficient edges: 127 and 253 symbols.  32 levels of 253 symbols need 4 (2 * 32 * 253 + 253) = 65 780 B of
    LDS and are refused; 31 levels (63 756 B) run, and are held to the law and to the plain call like every other table."""
    rng = np.random.RandomState(63)
    H = np.zeros((2, 6), dtype=np.int8)
    H[0, [0, 2, 4]] = [1, -1, 1]
    H[1, [1, 3, 5]] = [-1, -1, -1]
    prior = rng.dirichlet(np.ones(127))

    def table(K, Q):
        return dict(levels=rng.dirichlet(np.full(Q, 0.8), size=K), weights=rng.dirichlet(np.ones(K), size=Q))

    tb = table(2, 127)
    dec = qary.decoder_class("DecoderN6R2SW2B63")(H, 1)
    c = Case(H, 63, 126, prior, tb, table(32, 253), 8)
    with pytest.raises(lib.ScaldpcError, match=r"\[6\].*LDS"):
        c.run(dec, 8)
    c = Case(H, 63, 126, prior, tb, table(31, 253), 8)
    res = c.run(dec, 70)
    secret, levels = c.restated(70)
    assert np.array_equal(res["secret"], secret) and np.array_equal(res["levels"], levels) and len(np.unique(levels[:, 4:])) > 20
    assert np.array_equal(res["symbols"], dec.min_sum_batch(*c.pmf(levels)))
    c.follows(res)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_come_before_anything_is_queued():
    L = lib.load()
    c, _, _, _ = case1()
    dec = qary.decoder_class("DecoderN80R32SW3")(c.H, 4)
    base = c.run(dec, 8, FIRST1)
    untouched = np.full(8, 7, dtype=np.uint8)
    wrong = np.full((8, 2), -1, dtype=np.int32)

    def call(h=None, prior=c.prior, lb=c.lb, wb=c.wb, kb=None, ls=c.ls, ws=c.ws, ks=None, first=0, batch=8, flags=0, out=untouched):
        rc = L.scaldpc_mc_qary_run_secret(dec._h if h is None else h, lib.ptr(prior), lib.ptr(lb), lib.ptr(wb), c.lb.shape[0] if kb is None else kb,
                                          lib.ptr(ls), lib.ptr(ws), c.ls.shape[0] if ks is None else ks, first, batch, SEED1, flags, None,
                                          lib.ptr(out), lib.ptr(wrong), None, None, None, None)
        return rc, L.scaldpc_last_error().decode()

    def tab(K, Q):
        return np.tile(np.full(Q, 1.0 / Q, dtype=np.float32), (K, 1)), np.tile(np.full(K, 1.0 / K), (Q, 1))

    for name in ("prior", "lb", "wb", "ls", "ws", "out"):
        assert call(**{name: None})[0] == lib.EINVAL, name
    assert call(h=C.c_void_p())[0] == lib.EINVAL
    for kw in (dict(kb=0), dict(ks=0), dict(first=-1), dict(batch=0), dict(batch=-1), dict(flags=lib.F_ASYNC), dict(flags=lib.F_ASYNC | lib.F_DEVICE_IO)):
        assert call(**kw)[0] == lib.EINVAL, kw
    lb33, wb33 = tab(33, 5)
    ls33, ws33 = tab(33, 13)
    assert call(lb=lb33, wb=wb33, kb=33)[0] == lib.EINVAL and call(ls=ls33, ws=ws33, ks=33)[0] == lib.EINVAL
    for bad in ([-0.1, 0.5, 0.6, 0.0, 0.0], [np.nan, 0.5, 0.5, 0.0, 0.0], [0.2, 0.2, 0.2, 0.2, 0.2 + 2e-6], [0.0] * 5):
        rc, msg = call(prior=np.array(bad))
        assert rc == lib.EINVAL and "prior_b" in msg, bad
    for key, r, name in (("wb", 3, "weights_b[3]"), ("ws", 12, "weights_s[12]")):
        for v in (1.5, -0.1, np.inf, np.nan):
            w = getattr(c, key).copy()
            w[r, 0] = v
            rc, msg = call(**{key: w})
            assert rc == lib.EINVAL and name in msg, (key, v)
        w = getattr(c, key).copy()
        w[r, 0] += 2e-6
        rc, msg = call(**{key: w})
        assert rc == lib.EINVAL and name in msg and "sum" in msg
    short = c.lb.copy()
    short[1] *= 0.9
    rc, msg = call(lb=short)
    assert rc == lib.EPMF and "levels_b" in msg and "level 1" in msg
    nan_s = c.ls.copy()
    nan_s[2] = np.nan
    rc, msg = call(ls=nan_s)
    assert rc == lib.EPMF and "levels_s" in msg and "level 2" in msg
    with pytest.raises(ValueError):
        c.run(dec, 0)
    with pytest.raises(ValueError):
        dec.mc_run_secret(8, SEED1, c.prior[:4], c.lb, c.wb, c.ls, c.ws)
    with pytest.raises(ValueError):
        dec.mc_run_secret(8, SEED1, c.prior, c.lb, c.wb.T, c.ls, c.ws)
    with pytest.raises(lib.ScaldpcError, match=r"\[4\]"):
        dec.mc_run_secret(8, SEED1, c.prior, short, c.wb, c.ls, c.ws)
    # nothing was written, and the handle returns its earlier result
    assert (untouched == 7).all() and (wrong == -1).all()
    assert call(first=FIRST1)[0] == 0 and np.array_equal(untouched, base["success"]) and np.array_equal(wrong, base["wrong"])
    same(c.run(dec, 8, FIRST1), base, what="after the refusals")
    dec.close()
    # a plain handle: without row-sum variables a drawn secret is no code word
    plain = qary.decoder_class("DecoderN2R1V1C2B2")(np.array([[1, 1]], dtype=np.int8), 2)
    rc, msg = call(h=plain._h)
    assert rc == lib.EINVAL and "special" in msg
    plain.close()
