"""Every check and variable kernel held to the TRUE message, one pass at a time (tests/message_probes.py).

On a star forest the posterior of a row's probe variable (prior p = 0.5) is the check-to-variable message on its edge,
recomputed from the same inputs by every iteration; the key is a float64 closed form of the library's own float32
priors, so neither the oracle nor another kernel stands between a kernel and the truth.  On the combs every posterior is
a signed sum of priors: the variable pass.  tests/test_message_probes.py checks the key itself and measures the float32
oracle against it.

The tanh rule's bound, per (row-degree band, magnitude profile) cell, in u = 2^-24 * max(1, |L|):
    bound = max(16 u, 4 x the float32 oracle's worst in that cell), never more than 64 u (3.8e-6 * max(1, |L|))
The oracle's worst is measured in this run, on these probes.  Why 4: per edge the device chains three ~1-ulp hardware
operations (v_exp_f32, v_rcp_f32, v_log_f32) and the rounding of a * log2(e), which grows with |a| as u does, where the
oracle chains glibc calls of <= 1 ulp and a correctly rounded division: about twice the error per operation, and as much
again for margin.  Min-sum probes are bit-exact against the closed form.  The measured worst per (kernel family, band,
profile) is printed when the module is done (lines starting with PROBE; run with -s) and kept in
profiles/message_probes/message_error_mi355x.txt.

Which test reaches which kernel is listed in profiles/message_probes/README.md.
"""
import functools
import importlib

import numpy as np
import pytest

import message_probes as mp
from message_probes import comb_case, forest_case, soft_variants

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

FLOOR_U, FACTOR, CEIL_U = 16.0, 4.0, 64.0
TILE_FORESTS = ["cap16", "cap32", "cap64", "cap200"]
COL_BANDS = (16, 32, 64, 1 << 30)


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER", "SCALDPC_SPLIT"):
        monkeypatch.delenv(v, raising=False)


def _oracle():
    from oracle import pyoracle

    pyoracle.lib()
    return pyoracle


# ------------------------------------------------------------------------------------------------ keys, computed once
@functools.lru_cache(maxsize=None)
def shared_key(name):
    """(forest with its stuck row, syndromes, truth [70, probes], per-probe bound in u [probes]) for the shared priors."""
    f, synd = forest_case(name, True)
    truth = f.truth(synd)
    with np.errstate(all="ignore"):
        ref = _oracle().bp_decode_batch(f.graph, f.probs, synd, 0, 1, "tanh_complement", dtype="f32", threads=8, early_exit=False)
    cells = mp.worst_per_cell(f, mp.errors_in_u(ref["llr"][:, f.probe[f.rows]], truth))
    bound = np.array([min(CEIL_U, max(FLOOR_U, FACTOR * cells[(int(f.band[r]), str(f.kind[r]))])) for r in f.rows])
    return f, synd, truth, bound


@functools.lru_cache(maxsize=None)
def soft_key(name):
    """The same for the per-codeword priors: (probs32 [70, n], kinds [P, m], which, truth, bound in u [70, probes])."""
    f, synd = forest_case(name, True)
    p32, kinds, which = soft_variants(name)
    truth = f.truth(synd, p32, which)
    bound = np.zeros(truth.shape)
    for v in range(len(p32)):
        with np.errstate(all="ignore"):
            ref = _oracle().bp_decode_batch(f.graph, p32[v].astype(np.float64), synd[which == v], 0, 1, "tanh_complement",
                                            dtype="f32", threads=8, early_exit=False)
        cells = mp.worst_per_cell(f, mp.errors_in_u(ref["llr"][:, f.probe[f.rows]], truth[which == v]), kinds[v:v + 1])
        bound[which == v] = [min(CEIL_U, max(FLOOR_U, FACTOR * cells[(int(f.band[r]), str(kinds[v, r]))])) for r in f.rows]
    return p32[which], kinds, which, truth, bound


@functools.lru_cache(maxsize=None)
def minsum_key(name, alpha, soft):
    f, synd = forest_case(name, True)
    if not soft:
        return f.truth_minsum(synd, alpha)
    p32, _, which = soft_variants(name)
    return f.truth_minsum(synd, alpha, p32, which)


def decoder(graph, probs, method, max_iter, alpha=1.0, **knobs):
    with np.errstate(divide="ignore"):
        if probs is None:  # (a soft call brings every prior itself: whatever the decoder holds must not show)
            dec = bp.bp_decoder(graph, max_iter=max_iter, bp_method=method, error_rate=0.1, ms_scaling_factor=alpha)
        else:
            dec = bp.bp_decoder(graph, max_iter=max_iter, bp_method=method, channel_probs=probs, ms_scaling_factor=alpha)
    if knobs:
        dec.configure(**knobs)
    return dec


TABLE, COMB_TABLE, HALF = {}, {}, []  # worst per (kernel family, band, profile); per comb cell; families beyond half a bound


@pytest.fixture(scope="module", autouse=True)
def error_table():
    """Prints what the module measured (run with -s): the table kept in profiles/message_probes/message_error_mi355x.txt."""
    yield
    kinds = list(mp.PROFILES) + ["one_certain"]
    print("\nPROBE tanh rule, worst |got - truth| per (kernel family, row-degree band, profile), in u = 2^-24 * max(1, |L|)")
    print(f"PROBE {'family':32s} {'band':5s}" + "".join(f"{k:>12s}" for k in kinds))
    for fam in sorted({k[0] for k in TABLE}):
        for band in mp.BANDS:
            if any(k[0] == fam and k[1] == band for k in TABLE):
                print(f"PROBE {fam:32s} {mp.band_name(band):5s}" + "".join(
                    f"{TABLE[(fam, band, k)]:12.2f}" if (fam, band, k) in TABLE else " " * 12 for k in kinds))
    print(f"PROBE worst of all: {max(TABLE.values(), default=0.0):.2f} u; families with a probe beyond half its bound: {HALF or 'none'}")
    print("PROBE combs, worst |got - sum| in u' = 2^-24 * (sum of |terms|): hub / leaf per column-degree band (<=16, <=32, <=64, >64)")
    for key in sorted(COMB_TABLE):
        print(f"PROBE {key:60s} " + "  ".join(f"{'leaf' if c & 1 else 'hub'}[{c >> 1}] {w:5.2f}" for c, w in sorted(COMB_TABLE[key].items())))


def report(family, f, err, bound, kinds=None, which=None):
    for (band, kind), w in mp.worst_per_cell(f, err, kinds, which).items():
        if kind in mp.PROFILES or kind == "one_certain":
            TABLE[(family, band, kind)] = max(TABLE.get((family, band, kind), 0.0), w)
    if (err > np.broadcast_to(bound, err.shape) / 2).any() and family not in HALF:
        HALF.append(family)


def check_tanh(family, name, got, nb=None, soft=False):
    """The probes of `got` (a decode_batch result on forest `name`, the first nb codewords) against the truth."""
    f, synd, truth, bound = shared_key(name)
    kinds = which = None
    if soft:
        _, kinds, which, truth, bound = soft_key(name)
    nb = synd.shape[0] if nb is None else nb
    truth, which = truth[:nb], None if which is None else which[:nb]
    bound = bound[:nb] if soft else bound
    llr = got["llr"][:, f.probe[f.rows]]
    assert llr.shape == truth.shape
    err = mp.errors_in_u(llr, truth)
    report(family, f, err, bound, kinds, which)
    assert (err <= bound).all(), f"{family}: worst {np.nanmax(err / bound):.2f} of the bound"
    decided = np.abs(truth) > bound * mp.unit(truth)
    assert np.array_equal(np.sign(llr)[decided], np.sign(truth)[decided]), f"{family}: sign"
    inf = np.isinf(truth)
    assert inf.any() and np.array_equal(llr[inf].astype(np.float64), truth[inf]), f"{family}: certain rows"
    zero = truth == 0  # a source at p = 0.5 silences its row: exactly zero (the sign of a zero is not asserted)
    assert zero.any() and (llr[zero] == 0).all(), f"{family}: rows with an uninformative source"
    # nothing else is touched: the only NaN is the stuck variable's inf - inf, and every source keeps its prior + (+-0)
    col = f.graph.col_idx[f.graph.row_ptr[f.stuck]]
    nan = np.isnan(got["llr"])
    assert nan[:, col].all() and nan.sum() == nb, f"{family}: NaN posteriors"


def check_minsum(family, name, got, alpha, nb=None, soft=False):
    f, synd = forest_case(name, True)
    key = minsum_key(name, alpha, soft)
    nb = synd.shape[0] if nb is None else nb
    llr = got["llr"][:, f.probe[f.rows]]
    assert llr.dtype == np.float32 and np.array_equal(llr, key[:nb]), f"{family}: min-sum probe != +-fl(alpha * min|x|)"


def check(family, name, got, method, alpha=1.0, nb=None, soft=False):
    if method == "min_sum":
        check_minsum(family, name, got, alpha, nb, soft)
    else:
        check_tanh(family, name, got, nb, soft)


def assert_form(dec, f, method, rec=1):
    """The form and the path that ran are the ones asked for."""
    assert dec.last_stats()["row_parallel"] == 0
    want = method == "min_sum" and bool(rec) and int(f.deg.max()) <= 64
    assert dec.time_kernels(2)["record_form"] is want


# ------------------------------------------------------------------------------------------------ tile kernels
@pytest.mark.parametrize("name", TILE_FORESTS)
def test_tanh_tile_kernels(name):
    """k_check_tanh<CAP> (cap200: check_tanh_row_generic behind k_init_msg): the FIRST pass (max_iter 1, first_fused 0),
    k_var_first with the first-message table (max_iter 1, first_fused 1), the message-reading pass (max_iter 2, 3, 5);
    posteriors bit-identical across max_iter within a configuration and between the two."""
    f, synd, _, _ = shared_key(name)
    outs = {}
    for ff in (1, 0):
        dec = decoder(f.graph, f.probs, "product_sum", 5, path="stream", first_fused=ff)
        for it in (1, 2, 3, 5):
            outs[ff, it] = dec.decode_batch(synd, max_iter=it, early_exit=False, want_llr=True)
        assert_form(dec, f, "product_sum")
        dec.close()
        check_tanh(f"tile {name} " + ("k_var_first" if ff and name != "cap200" else "first pass"), name, outs[ff, 1])
        check_tanh(f"tile {name} message pass", name, outs[ff, 3])
        for it in (2, 3, 5):
            assert np.array_equal(outs[ff, it]["llr"], outs[ff, 1]["llr"], equal_nan=True), (name, ff, it)
    assert np.array_equal(outs[1, 1]["llr"], outs[0, 1]["llr"], equal_nan=True)


@pytest.mark.parametrize("fuse_test", [1, 0])
@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
@pytest.mark.parametrize("name", TILE_FORESTS)
def test_early_exit_kept_running_by_the_stuck_row(name, method, fuse_test):
    """early_exit = True: the stuck row keeps every codeword going to max_iter = 4, so the passes that carry the convergence
    test of the iteration before (the PAR builds of k_check_tanh / k_check_minsum_rec / k_check_minsum_x; fuse_test 0: the
    stand-alone test) produce the final messages; flags and counts say so."""
    f, synd, _, _ = shared_key(name)
    assert f.m > 128  # (at least FT_WORDS = 36 words of unsatisfied-row flags per tile: the test does ride)
    for rec in ((1, 0) if method == "min_sum" else (1,)):  # min-sum: record form and message form
        dec = decoder(f.graph, f.probs, method, 4, path="stream", fuse_test=fuse_test, minsum_rec=rec)
        got = dec.decode_batch(synd, early_exit=True, want_llr=True)
        assert_form(dec, f, method, rec)
        assert dec.last_stats()["compacted"] == 0
        dec.close()
        assert (got["iters"] == 4).all() and not got["converged"].any()
        check(f"tile {name} early " + ("riding test" if fuse_test else "own test"), name, got, method)


@pytest.mark.parametrize("alpha", [1.0, 0.75])
@pytest.mark.parametrize("name", TILE_FORESTS)
def test_minsum_tile_kernels(name, alpha):
    """Min-sum, record form (k_check_minsum_x FIRST, then k_check_minsum_rec boot at iteration 2 and steady from 3 on,
    k_var_rec) and message form (k_check_minsum_x; cap200: the loop form k_check_minsum), with and without the first
    check pass: every max_iter 1, 2, 3, 5 is the closed form bit for bit."""
    f, synd = forest_case(name, True)
    for rec in (1, 0):
        for ff in (1, 0):
            dec = decoder(f.graph, f.probs, "min_sum", 5, alpha, path="stream", minsum_rec=rec, first_fused=ff)
            for it in (1, 2, 3, 5):
                got = dec.decode_batch(synd, max_iter=it, early_exit=False, want_llr=True)
                check_minsum(f"min-sum tile {name} rec={rec} first_fused={ff} it={it}", name, got, alpha)
            assert_form(dec, f, "min_sum", rec)
            dec.close()


@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
def test_two_lanes_of_a_two_tile_group(method):
    """set_tile_group(2) with split = 2: each stream lane takes one tile of the group (the second one ragged)."""
    f, synd, _, _ = shared_key("cap32")
    dec = decoder(f.graph, f.probs, method, 3, path="stream", split=2)
    dec.set_tile_group(2)
    got = dec.decode_batch(synd, early_exit=False, want_llr=True)
    assert_form(dec, f, method)
    dec.close()
    check("tile cap32 two lanes", "cap32", got, method)


# ------------------------------------------------------------------------------------------------ row-parallel, LDS
@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
def test_row_parallel_kernels(method):
    """k_el_check<M, first, P> / k_el_var on the forest of rows up to 64 edges: 5 and 64 codewords, first pass alone and
    three iterations, early exit held open by the stuck row; and the single decode() of the ldpc surface."""
    f, synd, _, _ = shared_key("cap64")
    for nb in (5, 64):
        dec = decoder(f.graph, f.probs, method, 3, path="edge")
        one = dec.decode_batch(synd[:nb], max_iter=1, early_exit=False, want_llr=True)
        assert dec.last_stats()["row_parallel"] == nb
        three = dec.decode_batch(synd[:nb], early_exit=False, want_llr=True)
        early = dec.decode_batch(synd[:nb], max_iter=4, early_exit=True, want_llr=True)
        assert dec.last_stats()["row_parallel"] == nb
        dec.close()
        assert (early["iters"] == 4).all() and not early["converged"].any()
        check(f"row-parallel nb={nb} first pass", "cap64", one, method, nb=nb)
        check(f"row-parallel nb={nb} message pass", "cap64", three, method, nb=nb)
        check(f"row-parallel nb={nb} early", "cap64", early, method, nb=nb)
        assert np.array_equal(one["llr"], three["llr"], equal_nan=True) and np.array_equal(one["llr"], early["llr"], equal_nan=True)
    dec = decoder(f.graph, f.probs, method, 4)
    dec.decode(synd[0])
    assert dec.last_row_parallel() == 1 and dec.iter == 4 and dec.converge == 0
    got = {"llr": dec.log_prob_ratios[None].astype(np.float32)}
    dec.close()
    check("row-parallel decode()", "cap64", got, method, nb=1)


@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
def test_lds_resident_decoder(method):
    """k_bp_small on the thinned forest (rows up to 100 edges) that fits its 60 KB: `path = lds` is accepted, i.e. taken."""
    f, synd, _, _ = shared_key("lds")
    dec = decoder(f.graph, f.probs, method, 3, path="lds")
    one = dec.decode_batch(synd, max_iter=1, early_exit=False, want_llr=True)
    three = dec.decode_batch(synd, early_exit=False, want_llr=True)
    early = dec.decode_batch(synd, max_iter=4, early_exit=True, want_llr=True)
    assert dec.last_stats()["row_parallel"] == 0
    dec.close()
    assert (early["iters"] == 4).all() and not early["converged"].any()
    for what, got in (("first pass", one), ("message pass", three), ("early", early)):
        check(f"LDS {what}", "lds", got, method)
    assert np.array_equal(one["llr"], three["llr"], equal_nan=True) and np.array_equal(one["llr"], early["llr"], equal_nan=True)


# ------------------------------------------------------------------------------------------------ per-codeword priors
@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
@pytest.mark.parametrize("name,path", [(n, "stream") for n in TILE_FORESTS] + [("cap64", "edge"), ("lds", "lds")])
def test_per_codeword_priors(name, path, method):
    """decode_batch(..., channel_probs = [batch, n]): every prior comes with the codeword (k = n; the decoder's own are
    0.1 everywhere and must not show), probe columns at 0.5, codeword b carrying draw b % P in which every row has moved on
    to the next profile.  Reaches the SoftPrior builds: the FIRST pass of k_check_tanh / k_check_minsum_x /
    k_check_minsum, k_init_msg (cap200), k_var / k_var_rec, k_el_check / k_el_var, k_bp_small."""
    f, synd = forest_case(name, True)
    p32 = soft_key(name)[0]
    for nb in ((5, 64) if path == "edge" else (70,)):
        dec = decoder(f.graph, None, method, 3, path=path)
        one = dec.decode_batch(synd[:nb], max_iter=1, early_exit=False, want_llr=True, channel_probs=p32[:nb])
        three = dec.decode_batch(synd[:nb], early_exit=False, want_llr=True, channel_probs=p32[:nb])
        early = dec.decode_batch(synd[:nb], max_iter=4, early_exit=True, want_llr=True, channel_probs=p32[:nb])
        assert dec.last_stats()["row_parallel"] == (nb if path == "edge" else 0)
        if path == "stream":
            assert dec.time_kernels(2)["record_form"] is (method == "min_sum" and name != "cap200")
        dec.close()
        assert (early["iters"] == 4).all() and not early["converged"].any()
        for what, got in (("first pass", one), ("message pass", three), ("early", early)):
            check(f"soft {path} {name} nb={nb} {what}", name, got, method, nb=nb, soft=True)
        assert np.array_equal(one["llr"], three["llr"], equal_nan=True) and np.array_equal(one["llr"], early["llr"], equal_nan=True)


# ------------------------------------------------------------------------------------------------ combs: the variable pass
@functools.lru_cache(maxsize=None)
def comb_key(name):
    """(comb, syndromes, closed-form posteriors, u', per-column bound in u', per-column hub degree)."""
    cb, synd = comb_case(name)
    post, un = mp.true_comb_posteriors(cb, synd)
    ref = _oracle().bp_decode_batch(cb.graph, cb.probs, synd, 0, 2, "tanh_complement", dtype="f32", threads=8, early_exit=False)
    e = np.abs(ref["llr"] - post) / un
    cdeg = np.zeros(cb.n, dtype=np.int64)
    cell = np.zeros(cb.n, dtype=np.int64)  # 2 * band index + (1: leaf)
    for h, lv in zip(cb.hub, cb.leaves):
        cdeg[h] = cdeg[lv] = len(lv)
        b = next(i for i, c in enumerate(COL_BANDS) if len(lv) <= c)
        cell[h], cell[lv] = 2 * b, 2 * b + 1
    bound = np.zeros(cb.n)
    for c in np.unique(cell):
        bound[cell == c] = min(CEIL_U, max(FLOOR_U, FACTOR * float(e[:, cell == c].max())))
    return cb, synd, post, un, bound, cdeg, cell


@pytest.mark.parametrize("method", ["product_sum", "min_sum"])
@pytest.mark.parametrize("name", ["col16", "col32", "col64", "col100"])
def test_comb_posteriors_are_the_signed_sums(name, method):
    """k_var<16 | 32 | 64> and the generic column (col100), k_var_first, k_var_rec<16 | 32> (min-sum, record form), k_el_var
    (columns up to 64): hub and leaf posteriors against the closed-form signed sums after 2 and after 5 iterations.
    Tanh rule: within the bound, in u' = 2^-24 * (sum of |terms|); min-sum (alpha = 1: the messages are exact): within
    c * u', c the hub's degree -- c additions, each rounded once."""
    cb, synd, post, un, bound, cdeg, cell = comb_key(name)
    configs = [dict(path="stream", first_fused=1), dict(path="stream", first_fused=0)]
    if method == "min_sum":
        configs.append(dict(path="stream", minsum_rec=0))
    if cdeg.max() <= 64:
        configs.append(dict(path="edge"))
    for knobs in configs:
        nb = 5 if knobs["path"] == "edge" else synd.shape[0]
        dec = decoder(cb.graph, cb.probs, method, 5, **knobs)
        outs = [dec.decode_batch(synd[:nb], max_iter=it, early_exit=False, want_llr=True) for it in (2, 5)]
        assert dec.last_stats()["row_parallel"] == (nb if knobs["path"] == "edge" else 0)
        if knobs["path"] == "stream":
            assert dec.time_kernels(2)["record_form"] is bool(method == "min_sum" and knobs.get("minsum_rec", 1) and cdeg.max() <= 32)
        dec.close()
        for it, got in zip((2, 5), outs):
            e = np.abs(got["llr"].astype(np.float64) - post[:nb]) / un[:nb]
            lim = bound if method == "product_sum" else np.maximum(cdeg, 1).astype(np.float64)
            row = COMB_TABLE.setdefault(f"{method} {name} " + " ".join(f"{k}={v}" for k, v in knobs.items()), {})
            for c in np.unique(cell):
                row[int(c)] = max(row.get(int(c), 0.0), float(e[:, cell == c].max()))
            assert (e <= lim[None, :]).all(), (name, knobs, it, float((e / lim[None, :]).max()))
            clear = np.abs(post[:nb]) > lim[None, :] * un[:nb]
            assert np.array_equal(got["bits"][clear], (post[:nb] <= 0).astype(np.uint8)[clear])
