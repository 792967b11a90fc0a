"""The trimmed passes of the min-sum record form move fewer bytes and must compute what they computed before:

  * a row whose LAST edge goes into a column of degree 1 takes that edge's value from the shared priors (one scalar load)
    instead of loading the edge's 256-B message row -- rows with the constant edge elsewhere, with none, or decoded with
    per-codeword priors load everything as before;
  * the last variable pass of a decode stores neither messages nor sign masks.

Every case runs the tile kernels (path="stream") on graphs of the size of hqc_instance(701, 9, 200, 6, ...) with 130
codewords (two tiles and a ragged third, dealt to two stream lanes), asserts that the record form ran, and compares hard
decisions, posteriors, iteration counts and converged flags bit for bit with the f32 oracle and with the same build in the
message form (minsum_rec = 0; posteriors as bit patterns there too: array_equal cannot see the sign of a zero)."""
import importlib

import numpy as np
import pytest

from helpers import S, hqc_instance, staircase_graph
from soft_cases import oracle_per_codeword

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

KEYS = ("bits", "llr", "iters", "converged")
BATCH = 130
N, W, R, OMEGA, EPS = 701, 9, 200, 6, 0.03


def make_decoder(graph, probs, max_iter, rec, alpha=1.0, group=3):
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(graph, max_iter=max_iter, bp_method="min_sum", channel_probs=probs, ms_scaling_factor=alpha)
    dec.configure(path="stream", minsum_rec=rec, split=2)
    dec.set_tile_group(group)
    return dec


def same(got, want, what):
    for k in KEYS:
        w = np.asarray(want[k])
        assert np.array_equal(np.asarray(got[k]).astype(w.dtype), w, equal_nan=(k == "llr")), (what, k)


def same_bits(got, other, what):
    same(got, other, what)
    a = np.ascontiguousarray(got["llr"], dtype=np.float32).view(np.uint32)
    b = np.ascontiguousarray(other["llr"], dtype=np.float32).view(np.uint32)
    assert np.array_equal(a, b), (what, "posterior bit patterns")


def oracle_key(oracle, graph, probs, synd, max_iter, early, alpha=1.0):
    with np.errstate(divide="ignore", invalid="ignore"):
        return oracle.bp_decode_batch(graph, probs, synd, 0, max_iter, "min_sum", alpha=alpha, dtype="f32", threads=8,
                                      early_exit=early)


def hold(oracle, graph, probs, synd, settings, alpha=1.0, group=3):
    """Record form == oracle == message form for every (max_iter, early exit) of `settings`."""
    for max_iter, early in settings:
        what = (max_iter, early)
        ref = oracle_key(oracle, graph, probs, synd, max_iter, early, alpha)
        out = []
        for rec in (1, 0):
            dec = make_decoder(graph, probs, max_iter, rec, alpha, group)
            out.append(dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome"))
            assert dec.time_kernels(2)["record_form"] is bool(rec)  # the form that ran is the one asked for
            dec.close()
        same(out[0], ref, ("oracle",) + what)
        same_bits(out[0], out[1], ("message form",) + what)


def const_last_rows(Hd):
    """Rows of a dense H whose last edge goes into a column of degree 1 (what the table builder marks)."""
    cdeg = Hd.sum(axis=0)
    last = np.array([np.flatnonzero(row)[-1] if row.any() else -1 for row in Hd])
    return np.array([c >= 0 and cdeg[c] == 1 for c in last])


@pytest.fixture(scope="module")
def inst():
    """[Hin | I_R] dense, its priors, and 130 error patterns drawn from them (a few codewords with no error at all)."""
    H, Hin, probs, _, _ = hqc_instance(N, W, R, OMEGA, EPS, BATCH, seed=5101)
    rng = np.random.RandomState(5102)
    err = (rng.rand(BATCH, H.n) < probs[None, :]).astype(np.uint8)
    err[::9] = 0
    return H.to_dense(np.int8), Hin.to_dense(np.int8), probs, err


def syndromes(graph, err):
    return graph.syndrome(err)


ALL_SETTINGS = [(it, early) for it in (1, 2, 3, 8) for early in (False, True)]


def test_constant_edge_last(oracle, inst):
    """[Hin | I]: every row ends in its identity column -- the new path in every row."""
    Hd, _, probs, err = inst
    assert const_last_rows(Hd).all()
    G = S.TannerGraph.from_dense(Hd)
    hold(oracle, G, probs, syndromes(G, err), ALL_SETTINGS)
    hold(oracle, G, probs, syndromes(G, err), [(3, False), (8, True)], alpha=0.75)


def test_constant_edge_first(oracle, inst):
    """[I | Hin]: every row STARTS with its constant edge and ends in an ordinary one -- all loads, as before."""
    Hd, _, probs, err = inst
    perm = np.concatenate([np.arange(N, N + R), np.arange(N)])
    Hp = np.ascontiguousarray(Hd[:, perm])
    marked = const_last_rows(Hp)
    assert (Hp[:, :R].sum(axis=0) == 1).all() and marked.sum() < R // 4  # (a few rows of Hin end in a column of degree 1 by chance)
    G = S.TannerGraph.from_dense(Hp)
    hold(oracle, G, probs[perm], syndromes(G, err[:, perm]), ALL_SETTINGS)


def test_no_constant_edge(oracle, inst):
    """[Hin | B] with B a double diagonal: every row's last edges go into columns of degree 2."""
    _, Hin, probs, err = inst
    B = np.eye(R, dtype=np.int8) + np.roll(np.eye(R, dtype=np.int8), 1, axis=0)
    Hd = np.concatenate([Hin, B], axis=1)
    assert not const_last_rows(Hd).any()
    G = S.TannerGraph.from_dense(Hd)
    hold(oracle, G, probs, syndromes(G, err), ALL_SETTINGS)


def test_lone_and_doubled_constant_edges(oracle, inst):
    """[Hin | I] plus a row whose ONLY edge goes into a column of degree 1, and a row whose LAST TWO edges do (the last is
    taken from the priors, the one before it is loaded)."""
    Hd, _, probs, err = inst
    m, n = Hd.shape
    H2 = np.zeros((m + 1, n + 2), dtype=np.int8)
    H2[:m, :n] = Hd
    H2[5, n] = 1  # row 5: ..., its identity column, and one more column of degree 1
    H2[m, n + 1] = 1  # the new row: one edge
    marked = const_last_rows(H2)
    assert marked.all() and H2[m].sum() == 1 and (H2[:, [N + 5, n]].sum(axis=0) == 1).all()
    p2 = np.concatenate([probs, [0.2, 0.4]])
    rng = np.random.RandomState(5103)
    e2 = np.concatenate([err, (rng.rand(BATCH, 2) < 0.3).astype(np.uint8)], axis=1)
    G = S.TannerGraph.from_dense(H2)
    hold(oracle, G, p2, syndromes(G, e2), ALL_SETTINGS)


VALUE_SETTINGS = [(2, False), (3, False), (8, False), (8, True)]


@pytest.mark.parametrize("case", ["half", "certain", "equal"])
def test_constant_edge_values(oracle, inst, case):
    """The value the constant edge carries: p = 0.5 (x = +0, which counts as negative), p = 0 and p = 1 (+-inf: never the
    minimum, clamped to FLT_MAX), and the same p on every column (the constant edge ties for m1 with earlier edges of its
    row -- the messages of Hin's own columns of degree 1 -- and the FIRST edge that attains m1 must be the arg-min)."""
    Hd, _, probs, err = inst
    G = S.TannerGraph.from_dense(Hd)
    p = probs.copy()
    rng = np.random.RandomState(5104)
    if case == "half":
        p[N:] = 0.5
    elif case == "certain":
        p[N:] = rng.choice([0.0, 1.0, EPS], size=R, p=[0.4, 0.3, 0.3])
    else:
        p[:] = 0.05
        lone = np.flatnonzero(Hd[:, :N].sum(axis=0) == 1)
        assert len(lone) > 0  # columns of Hin with one edge: their message is the prior too, earlier in the row
    hold(oracle, G, p, syndromes(G, err), VALUE_SETTINGS)


def test_new_priors_on_a_live_decoder(oracle, inst):
    """The constant edge is read from the handle's priors at launch: new priors between two decodes need no rebuild."""
    Hd, _, probs, err = inst
    G = S.TannerGraph.from_dense(Hd)
    synd = syndromes(G, err)
    rng = np.random.RandomState(5105)
    p2 = probs.copy()
    p2[N:] = rng.choice([0.0, 0.5, 0.2, 0.9], size=R)
    for max_iter, early in [(3, False), (8, True)]:
        dec = make_decoder(G, probs, max_iter, 1)
        for pr in (probs, p2, probs):
            with np.errstate(divide="ignore"):
                dec.update_channel_probs(pr)
            got = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome")
            same(got, oracle_key(oracle, G, pr, synd, max_iter, early), ("live priors", max_iter, early))
        assert dec.time_kernels(2)["record_form"] is True
        dec.close()


def test_soft_call(oracle, inst):
    """Per-codeword priors on the identity columns: their edges are no constants of the call -- every row loads all its
    edges -- and a plain call on the same handle afterwards takes the constant again."""
    Hd, _, probs, err = inst
    G = S.TannerGraph.from_dense(Hd)
    synd = syndromes(G, err)
    rng = np.random.RandomState(5106)
    tail = rng.choice(np.array([0.0, 0.02, 0.1, 0.3, 0.5], dtype=np.float32), size=(BATCH, R))
    for max_iter, early in [(3, False), (8, True)]:
        ref = oracle_per_codeword(oracle, G, probs, tail, synd, 0, max_iter, "min_sum", early_exit=early)
        out = []
        for rec in (1, 0):
            dec = make_decoder(G, probs, max_iter, rec)
            out.append(dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome", channel_probs=tail))
            assert dec.time_kernels(2)["record_form"] is bool(rec)
            plain = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome")
            same(plain, oracle_key(oracle, G, probs, synd, max_iter, early), ("plain after soft", max_iter, early, rec))
            dec.close()
        same(out[0], ref, ("soft, oracle", max_iter, early))
        same_bits(out[0], out[1], ("soft, message form", max_iter, early))


def csr_of(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rp, np.concatenate(rows).astype(np.int32)


def test_growing_graph(oracle, inst):
    """append_rows brings new identity columns and gives an OLD column of degree 1 a second edge (its row loses the
    constant); a further append adds a row of another weight (the rows' common degree is gone).  After each step the
    live decoder equals a fresh one and the oracle."""
    _, Hin, probs, err = inst
    R0, R1 = 150, 199
    hin_rows = [np.flatnonzero(Hin[r]) for r in range(R)]
    rows = [np.concatenate([hin_rows[r], [N + r]]) for r in range(R0)]
    p = np.concatenate([probs[:N], probs[N:N + R0]])
    # step 1: rows R0 .. R1-1, each with its identity column; row R0 trades its last edge of Hin for one into the identity
    # column of row 3 (the rows keep their common degree)
    new1 = [np.concatenate([hin_rows[r], [N + r]]) for r in range(R0, R1)]
    new1[0] = np.concatenate([hin_rows[R0][:-1], [N + 3, N + R0]])
    # step 2: one row of another weight (four edges of Hin's row and an identity column)
    new2 = [np.concatenate([hin_rows[R1][:4], [N + R1]])]
    rng = np.random.RandomState(5107)
    e_all = np.concatenate([err[:, :N], (rng.rand(BATCH, R1 + 1) < EPS).astype(np.uint8)], axis=1)
    for max_iter, early in [(3, False), (8, True)]:
        rp, ci = csr_of(rows)
        dec = make_decoder(S.TannerGraph.from_csr(R0, N + R0, rp, ci), p, max_iter, 1)
        cur, cur_p = list(rows), p
        for step, new in enumerate([[], new1, new2]):
            if new:
                nrp, nci = csr_of(new)
                n_new = N + len(cur) + len(new)
                tail = np.full(len(new), EPS)
                dec.append_rows(nrp, nci, n_new, tail)
                cur, cur_p = cur + new, np.concatenate([cur_p, tail])
            rp, ci = csr_of(cur)
            G = S.TannerGraph.from_csr(len(cur), N + len(cur), rp, ci)
            Hd = G.to_dense(np.int8)
            marked = const_last_rows(Hd)
            assert marked.sum() == (len(cur) if step == 0 else len(cur) - 1) and (step == 0 or not marked[3])
            assert (len({len(r) for r in cur}) == 1) == (step < 2)  # one row degree until the second append
            synd = G.syndrome(e_all[:, : G.n])
            got = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome")
            assert dec.time_kernels(2)["record_form"] is True
            same(got, oracle_key(oracle, G, cur_p, synd, max_iter, early), ("grown, oracle", step, max_iter, early))
            fresh = make_decoder(G, cur_p, max_iter, 1)
            same_bits(got, fresh.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome"),
                      ("grown, fresh decoder", step, max_iter, early))
            fresh.close()
        dec.close()


@pytest.mark.parametrize("group", [3, 2])
def test_last_pass_leaves_a_usable_handle(oracle, inst, group):
    """The last variable pass stores nothing: ONE handle decodes with max_iter 3, then 2, then 5 (time_kernels in between:
    it runs on the messages and masks the pass before the last left); each result equals the oracle.  group = 2: the
    third tile is a second group that reuses the first group's arrays right after its store-free pass."""
    Hd, _, probs, err = inst
    G = S.TannerGraph.from_dense(Hd)
    synd = syndromes(G, err)
    for early in (False, True):
        dec = make_decoder(G, probs, 3, 1, group=group)
        for max_iter in (3, 2, 5):
            got = dec.decode_batch(synd, max_iter=max_iter, early_exit=early, want_llr=True, input_vector_type="syndrome")
            same(got, oracle_key(oracle, G, probs, synd, max_iter, early), ("one handle", max_iter, early, group))
            assert dec.time_kernels(3)["record_form"] is True
        dec.close()


def test_early_exit_with_stragglers_at_max_iter(oracle, inst):
    """Early exit on trials noisy enough that some codewords of a tile converge and others reach max_iter: the store-free
    pass runs with the done bits mixed."""
    Hd, _, probs, _ = inst
    G = S.TannerGraph.from_dense(Hd)
    rng = np.random.RandomState(5108)
    noisy = probs.copy()
    noisy[:N] = 5 * OMEGA / N
    noisy[N:] = 0.12
    err = (rng.rand(BATCH, G.n) < noisy[None, :]).astype(np.uint8)
    err[::4] = (rng.rand(len(err[::4]), G.n) < probs[None, :]).astype(np.uint8)  # (easy ones among them)
    synd = syndromes(G, err)
    max_iter = 6
    ref = oracle_key(oracle, G, probs, synd, max_iter, True)
    conv = np.asarray(ref["converged"]).astype(bool)
    for t in range(3):  # every tile holds both kinds
        c = conv[64 * t : 64 * (t + 1)]
        assert c.any() and not c.all(), t
    assert (np.asarray(ref["iters"])[~conv] == max_iter).all()
    hold(oracle, G, probs, synd, [(max_iter, True)])
    hold(oracle, G, probs, synd, [(max_iter, True)], group=2)


def test_every_degree(oracle):
    """helpers.staircase_graph: rows of every degree 1 .. 64 (no common row degree), columns of every degree 0 .. 32 --
    the column of degree 1 makes the row that holds it last a marked row of whatever degree it has."""
    rng = np.random.RandomState(5109)
    G, Hd = staircase_graph(rng)
    probs = rng.uniform(0.01, 0.2, size=G.n)
    err = (rng.rand(BATCH, G.n) < probs[None, :] * 0.5).astype(np.uint8)
    err[::7] = 0
    hold(oracle, G, probs, G.syndrome(err), [(1, False), (2, False), (3, False), (8, False), (8, True)])
