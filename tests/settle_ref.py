"""A NumPy float32 restatement of the min-sum RECORD form (k_check_minsum_rec / k_var_rec) that also says when a codeword's
message state has stopped changing.

After check pass t the state that determines everything later is (rec, arg, sgn): per row the two scaled magnitudes with the
row's parity in their sign bit and the index of the arg-min edge, per edge the sign "the variable-to-check message is <= 0".
A codeword is SETTLED at t (t >= 3) when check pass t produced the records and arg-min indices of check pass t - 1, bit for
bit, for every row, and variable pass t - 1 produced the signs of variable pass t - 2 for every edge.  A tile of 64
codewords is FROZEN at t when all its codewords are settled at t.  tests/test_settle_ref.py holds the arithmetic to the
float32 oracle; tests/test_settle_gpu.py holds the device's frozen-at numbers (scaldpc_bp_last_settle) to the ones here.
"""
import functools
import importlib
import types

import numpy as np

S = importlib.import_module("sca-ldpc_amd")
trials = importlib.import_module("sca-ldpc_amd.trials")

FLT_MAX = np.float32(np.finfo(np.float32).max)
NO_ARG = 255
TW = 64


def alpha_for(alpha, it):
    """ms_scaling_factor 0 = the schedule 1 - 2^-it, formed in float64 and rounded once."""
    return np.float32(1.0 - 2.0 ** (-it)) if alpha == 0.0 else np.float32(alpha)


def first_test(alpha, max_iter):
    """Tests need one alpha in check passes t - 1 and t and in everything later: the first t >= 3 with that."""
    a_end = alpha_for(alpha, max_iter)
    frm = next(i for i in range(1, max_iter + 1) if alpha_for(alpha, i) == a_end)
    return max(3, frm + 1)


def prior_llr(probs):
    p = np.asarray(probs, dtype=np.float64).astype(np.float32)
    q = (np.float32(1) - p) / p  # float32, as the oracle forms it
    return np.log(q.astype(np.float64)).astype(np.float32)


def _padded(ptr, idx, count):
    deg = np.diff(ptr)
    width = int(deg.max()) if count else 0
    tab = np.full((count, max(width, 1)), -1, dtype=np.int64)
    for i in range(count):
        tab[i, : deg[i]] = idx[ptr[i] : ptr[i + 1]]
    return tab, tab >= 0


def run(g, prior, synd, max_iter, alpha=1.0):
    """All `max_iter` iterations on every row of `synd` (uint8 [batch, m]); prior = LLRs float32 [n], or [batch, n] per codeword.
    Returns dict:
    post      float32 [max_iter + 1, batch, n]: the posterior after iteration it (index 0 unused)
    same      bool [max_iter + 1, batch]: same[t] = the two compares of test t found no difference (t >= 3)
    same_but_arg  the same with the arg-min indices left out of the compare: what a test that forgot them would see"""
    prior = np.asarray(prior, dtype=np.float32)
    synd = np.asarray(synd, dtype=np.uint8)
    B, m, n, E = synd.shape[0], g.m, g.n, g.nnz
    row_ptr, col_idx = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    rows, rvalid = _padded(row_ptr, np.arange(E), m)  # edge ids of every row (CSR position = edge id)
    cols, cvalid = _padded(np.asarray(g.col_ptr), np.asarray(g.csc_edge), n)  # ... of every column, in the column's order
    kk = np.arange(rows.shape[1])[None, None, :]
    x = np.broadcast_to(prior[..., col_idx], (B, E)).copy()  # variable-to-check messages; before iteration 1: the priors
    post = np.zeros((max_iter + 1, B, n), dtype=np.float32)
    same = np.zeros((max_iter + 1, B), dtype=bool)
    same_but_arg = np.zeros((max_iter + 1, B), dtype=bool)
    rec_prev = None
    sgn_prev, sgn_same = x <= 0, np.zeros(B, dtype=bool)
    for it in range(1, max_iter + 1):
        a = alpha_for(alpha, it)
        # ---- check pass: records --------------------------------------------------------------------------------
        X = np.where(rvalid[None], x[:, np.where(rvalid, rows, 0)], np.float32(np.inf))  # [B, m, dr]
        neg = X <= 0
        ax = np.minimum(np.abs(X), FLT_MAX)
        srt = np.sort(ax, axis=2)
        m1 = srt[:, :, 0]
        m2 = srt[:, :, 1] if srt.shape[2] > 1 else np.full_like(m1, FLT_MAX)
        odd = (synd.astype(bool)) ^ ((neg.sum(axis=2) & 1).astype(bool))
        eq = np.abs(X) == m1[:, :, None]
        arg = np.where(eq.any(axis=2), eq.argmax(axis=2), NO_ARG)
        r1, r2 = m1 * a, m2 * a
        r1, r2 = np.where(odd, -r1, r1), np.where(odd, -r2, r2)
        rec = (r1.view(np.uint32), r2.view(np.uint32), arg)
        if rec_prev is not None:
            rec_same = np.ones(B, dtype=bool)
            for u, v in zip(rec[:2], rec_prev[:2]):
                rec_same &= (u == v).all(axis=1)
            same_but_arg[it] = rec_same & sgn_same
            rec_same &= (rec[2] == rec_prev[2]).all(axis=1)
            same[it] = rec_same & sgn_same
        rec_prev = rec
        # ---- the messages the variable pass rebuilds: (arg-min ? rec2 : rec1) with the edge's own sign flipped in --------
        mag = np.where(kk == arg[:, :, None], r2[:, :, None], r1[:, :, None]).astype(np.float32)
        c2v_rows = (mag.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(np.float32)
        c2v = np.zeros((B, E), dtype=np.float32)
        c2v[:, rows[rvalid]] = c2v_rows[:, rvalid]
        # ---- variable pass: prefix sums from the prior, suffix sums from 0, in the column's order -------------------
        C = c2v[:, np.where(cvalid, cols, 0)]  # [B, n, dc]
        dc = cols.shape[1]
        temp = np.broadcast_to(prior, (B, n)).copy()
        pp = []
        for k in range(dc):
            pp.append(temp)
            temp = np.where(cvalid[None, :, k], temp + C[:, :, k], temp)
        post[it] = temp
        suf = np.zeros((B, n), dtype=np.float32)
        for k in range(dc - 1, -1, -1):
            v = cvalid[:, k]
            x[:, cols[v, k]] = (pp[k] + suf)[:, v]
            suf = np.where(v[None], suf + C[:, :, k], suf)
        sgn = x <= 0
        sgn_same = (sgn == sgn_prev).all(axis=1)
        sgn_prev = sgn
    return {"post": post, "same": same, "same_but_arg": same_but_arg}


def settled_at(same, first, last):
    """Per codeword the first test t in [first, last] that found no difference, 0 = none."""
    out = np.zeros(same.shape[1], dtype=np.int64)
    for t in range(min(last, same.shape[0] - 1), first - 1, -1):
        out[same[t]] = t
    return out


def frozen_at(same, first, last, batch=None):
    """Per tile of 64 codewords (the last one partial) the first test in [first, last] at which ALL its codewords show no
    difference, 0 = none."""
    batch = same.shape[1] if batch is None else batch
    out = []
    for t0 in range(0, batch, TW):
        tile = same[:, t0 : min(t0 + TW, batch)].all(axis=1)
        hit = [t for t in range(first, min(last, same.shape[0] - 1) + 1) if tile[t]]
        out.append(hit[0] if hit else 0)
    return out


# ---- the graphs and inputs of the settle tests ----------------------------------------------------------------------
def hqc_case(batch, seed=11, N=500, W=10, R=150, omega=3, eps=0.02):
    """An HQC-shaped [Hin | I]: R rows of W circulant-shifted ones over N columns, plus the identity block; trials by the
    bench's law (trials.hqc_trials).  Returns (H, probs, syndromes uint8 [batch, R])."""
    rng = np.random.RandomState(seed)
    sup = S.codes.make_random_ldpc_first_row(N, W, rng)
    Hin = S.codes.hqc_check_graph(sup, N, rng.permutation(N)[:R])
    H = Hin.with_identity()
    msg, _ = trials.hqc_trials(Hin, omega, eps, batch, base_seed=seed)
    return H, trials.hqc_priors(N, R, omega, eps), np.ascontiguousarray(msg[:, N:])


def regular_case(batch, seed=5, n=300, p=0.04):
    """A (3,6)-regular graph, no column of degree 1; syndromes of Bernoulli(p) errors."""
    rng = np.random.RandomState(seed)
    H = S.codes.make_regular_ldpc_graph(n, n // 2, 3, 6, rng)
    err = (rng.rand(batch, n) < p).astype(np.uint8)
    return H, np.full(n, p), H.syndrome(err).astype(np.uint8)


MAX_ITER = 50
BATCH = 64 * 5 + 3


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared inputs, each with one run of the restatement to MAX_ITER (computed once, never changed):
    "hqc"       the HQC-shaped graph, BATCH trials, alpha 1
    "schedule"  the same graph, the first 70 trials, the alpha schedule 1 - 2^-it (ms_scaling_factor 0)
    "regular"   the (3,6)-regular graph, 70 codewords, alpha 1"""
    if name == "regular":
        H, probs, synd = regular_case(70)
        alpha = 1.0
    else:
        H, probs, synd = hqc_case(BATCH)
        alpha = 1.0 if name == "hqc" else 0.0
        synd = synd if name == "hqc" else synd[:70]
    out = run(H, prior_llr(probs), synd, MAX_ITER, alpha)
    return types.SimpleNamespace(H=H, probs=probs, synd=synd, alpha=alpha, first=first_test(alpha, MAX_ITER), **out)


@functools.lru_cache(maxsize=None)
def oracle_at(name, max_iter):
    """The float32 oracle on a case's inputs, fixed iterations (computed once per max_iter, never changed)."""
    from oracle import pyoracle

    c = case(name)
    return pyoracle.bp_decode_batch(c.H, c.probs, c.synd, 0, max_iter, "min_sum", alpha=c.alpha, dtype="f32",
                                    threads=max(1, min(8, pyoracle.max_threads())), early_exit=False)
