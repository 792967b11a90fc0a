"""The inputs of tests/test_settle_matrix_gpu.py: settled min-sum on every kernel instantiation and launch shape
the settle code can meet, each with ONE run of the NumPy restatement (tests/settle_ref.py) that says when every codeword's
message state stops changing.  tests/test_settle_matrix.py holds the restatement to the float32 oracle on every case and
asserts that the cases contain what the GPU tests rely on.  Nothing here needs a GPU, and nothing runs at import.

Every graph is an HQC-shaped [Hin | I] from settle_ref.hqc_case (seed 11), alpha 1, max_iter 50:

  base     N 500, W 10, R 150           rows of 11 edges (cap 16), columns of 0 ... 8 (cap 16); 140 trials
  row32    N 900, W 17, R 150           rows of 18 (cap 32), columns 0 ... 8; 140 trials; one tile freezes at test 49
  row64    N 4000, W 33, R 130          rows of 34 (cap 64), columns 0 ... 7; 70 trials
  col32    N 900, W 17, R 600, omega 10, eps 0.06   rows of 18, columns 1 ... 17 (variable-pass cap 32); 140 trials

  ties32   row32's shape, eps = omega / N   every prior is ONE float, so messages are small multiples of it and rows are full
  ties64   row64's shape, eps = omega / N   of ties: the last thing that changes in a tile is then often an arg-min index
                                            alone, between two edges of equal magnitude (`want_but_arg`: the frozen-at numbers
                                            of a test that left the arg-min indices out differ from `want`)

A codeword whose syndrome is uniform random bits (RandomState(1)) does not settle within 50 iterations on these graphs: that
is how a case gets a tile that never freezes where the trials supply none (col32: codeword 70), and how the launch-shape
cases choose WHICH tiles stay unfrozen.  Those (`wide_one`, `wide_three`) are 579 codewords = 10 tiles on the base graph, put
together from one run of the restatement over a pool of 700 trials and 4 random syndromes: the codewords that settle, in the
pool's order, with a random syndrome at the head of tile 5 (`wide_one`: 9 of 10 tiles freeze, so a horizon is learned and
one tile is decoded again under it), or of tiles 2, 3 and 6 (`wide_three`: two adjacent unfrozen tiles and an isolated one).

The rest: `base100` / `grown` / `extra` are the steps of a handle that grows (69 codewords: both tiles freeze, so a horizon
is learned at every step); `soft()` deals two rows of priors to 130 codewords of col32; `sweep("hqc" | "fer", first)` are the
trials the device draws in mc_hqc_run / mc_fer_run (seeds chosen so that trials 0 ... 139 freeze all three tiles)."""
import functools
import types

import numpy as np

import settle_ref as R

S, MAX_ITER, TW = R.S, R.MAX_ITER, R.TW
SHAPES = {
    "base": dict(batch=140),
    "row32": dict(batch=140, N=900, W=17, R=150),
    "row64": dict(batch=70, N=4000, W=33, R=130),
    "col32": dict(batch=140, N=900, W=17, R=600, omega=10, eps=0.06),
    "ties32": dict(batch=140, N=900, W=17, R=150, omega=3, eps=3 / 900),
    "ties64": dict(batch=70, N=4000, W=33, R=130, omega=3, eps=3 / 4000),
}
REPLACED = {"col32": (70,)}  # codewords that get a random syndrome
WIDE = 64 * 9 + 3
WIDE_UNFROZEN = {"wide_one": (5,), "wide_three": (2, 3, 6)}
GROW_BATCH, GROW_FIRST = 69, 100  # (codewords 69 and 72 of the trials never settle on the first 100 rows)
SWEEP_RUNS, SWEEP_FIRST2, SWEEP_HORIZON = 140, 1000, 5
HQC_SEED, FER_SEED = 3, 4  # (tests/test_settle_matrix.py: trials 0 ... 139 of either sweep freeze all three tiles)


def random_syndromes(count, m):
    return (np.random.RandomState(1).rand(count, m) < 0.5).astype(np.uint8)


def _case(H, probs, synd, replaced=(), prior=None):
    out = R.run(H, R.prior_llr(probs) if prior is None else prior, synd, MAX_ITER, 1.0)
    same = out["same"]
    same.setflags(write=False)
    return types.SimpleNamespace(H=H, probs=probs, synd=synd, alpha=1.0, same=same, post=out["post"][MAX_ITER].copy(),
                                 replaced=tuple(replaced), want=R.frozen_at(same, 3, MAX_ITER), same_but_arg=out["same_but_arg"],
                                 want_but_arg=R.frozen_at(out["same_but_arg"], 3, MAX_ITER))


def _subset(pool, ids, replaced=()):
    """The codewords `ids` of a case, in that order: codewords are independent, so the pool's one run says it all."""
    ids = np.asarray(ids)
    same, but = pool.same[:, ids], pool.same_but_arg[:, ids]
    return types.SimpleNamespace(H=pool.H, probs=pool.probs, synd=pool.synd[ids], alpha=1.0, same=same, post=pool.post[ids],
                                 replaced=tuple(replaced), want=R.frozen_at(same, 3, MAX_ITER), same_but_arg=but,
                                 want_but_arg=R.frozen_at(but, 3, MAX_ITER))


@functools.lru_cache(maxsize=None)
def _graph(name):
    return R.hqc_case(**SHAPES[name])


@functools.lru_cache(maxsize=None)
def _wide_pool():
    """700 trials of the base graph and 4 random syndromes, one run of the restatement."""
    H, probs, synd = R.hqc_case(700)
    synd = np.concatenate([synd, random_syndromes(4, H.m)])
    return _case(H, probs, synd, replaced=range(700, 704))


@functools.lru_cache(maxsize=None)
def _ties32_pool():
    return _case(*R.hqc_case(**dict(SHAPES["ties32"], batch=400)))


def _cut(H, rows):
    """[Hin[:rows] | I_rows] of an [Hin | I] graph."""
    N = H.n - H.m
    rp = np.asarray(H.row_ptr)[: rows + 1]
    ci = np.asarray(H.col_idx)[: rp[-1]]
    assert (ci[rp[1:] - 1] == N + np.arange(rows)).all()
    return S.TannerGraph.from_csr(rows, N + rows, rp.astype(np.int64), ci.astype(np.int32))


def extra_row(H):
    """A 151st row for the grown base graph, without a column of its own: the first column of Hin that has degree 1, and the
    identity column of row 7 -- which then has degree 2, so row 7's last edge is no longer a constant."""
    N = H.n - H.m
    first = int(np.flatnonzero(np.asarray(H.col_degrees())[:N] == 1)[0])
    return np.array([first, N + 7], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """SimpleNamespace(H, probs, synd, alpha, same, post (at MAX_ITER), replaced, want = frozen-at per tile): computed once,
    never changed."""
    if name == "ties32":
        # tile 0: the codeword that settles last among those whose last change is an arg-min index alone, and 63 that settle
        # before that change; tile 1: one that never settles among 63 more; tile 2: 12 more
        pool = _ties32_pool()
        at, but = R.settled_at(pool.same, 3, MAX_ITER), R.settled_at(pool.same_but_arg, 3, MAX_ITER)
        star = max(np.flatnonzero(at != but), key=lambda b: (at[b], -b))
        early = [int(b) for b in np.flatnonzero((at > 0) & (at < but[star]))]
        never = int(np.flatnonzero(at == 0)[0])
        return _subset(pool, [int(star)] + early[:63] + [never] + early[63:138], (64,))
    if name in SHAPES:
        H, probs, synd = _graph(name)
        synd = synd.copy()
        rep = REPLACED.get(name, ())
        synd[list(rep)] = random_syndromes(len(rep), H.m)
        return _case(H, probs, synd, rep)
    if name in WIDE_UNFROZEN:
        pool = _wide_pool()
        at = R.settled_at(pool.same, 3, MAX_ITER)
        settled = [int(b) for b in np.flatnonzero(at[:700] > 0)]
        heads = [t * TW for t in WIDE_UNFROZEN[name]]
        ids = settled[:WIDE]
        for k, b in enumerate(heads):
            ids[b] = 700 + k
        return _subset(pool, ids, heads)
    H, probs, synd = _graph("base")
    N = H.n - H.m
    synd = synd[:GROW_BATCH]
    if name == "base100":
        return _case(_cut(H, GROW_FIRST), np.concatenate([probs[:N], probs[N : N + GROW_FIRST]]), synd[:, :GROW_FIRST].copy())
    if name == "grown":
        return _case(H, probs, synd.copy())
    if name == "extra":
        row = extra_row(H)
        G = S.TannerGraph.from_csr(H.m + 1, H.n, np.concatenate([H.row_ptr, [H.nnz + len(row)]]).astype(np.int64),
                                   np.concatenate([H.col_idx, row]).astype(np.int32))
        bit = (np.arange(GROW_BATCH) % 3 == 0).astype(np.uint8)[:, None]  # the new check's syndrome bit
        return _case(G, probs, np.concatenate([synd, bit], axis=1))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """The float32 oracle on a case's inputs, MAX_ITER fixed iterations."""
    from oracle import pyoracle

    c = case(name)
    return pyoracle.bp_decode_batch(c.H, c.probs, c.synd, 0, MAX_ITER, "min_sum", alpha=1.0, dtype="f32",
                                    threads=max(1, min(8, pyoracle.max_threads())), early_exit=False)


# ---- the rules of scaldpc_bp_sched.h, as the reports of a call follow from the frozen-at numbers ----------------------------
def usable(K):
    return K >= 3 and K + 1 < MAX_ITER


def rerun(want, K):
    """Tiles a call with horizon K decodes again."""
    return sum(1 for f in want if not 0 < f <= K) if K else 0


def next_horizon(want, K):
    """The horizon the call AFTER one with frozen-at numbers `want` under horizon K runs with (settle_next_horizon)."""
    tiles, frozen, top = len(want), sum(1 for f in want if f), max(want)
    if top <= 0 or 8 * rerun(want, K) > tiles or 8 * frozen < 7 * tiles or 2 * (top + 2) >= MAX_ITER:
        return 0
    return top + 2


def short_horizon(want):
    """A forced horizon below the largest frozen-at number."""
    return max(want) - 1


# ---- the soft call ---------------------------------------------------------------------------------------------------------
SOFT_BATCH, SOFT_ROWS = 130, (0.06, 0.03)


@functools.lru_cache(maxsize=None)
def soft():
    """col32, 130 codewords, two rows of check priors dealt in turn: SimpleNamespace(cp float32 [130, R], synd, same, post, want)
    from the restatement on every codeword's own priors."""
    c = case("col32")
    Rr, n = c.H.m, c.H.n
    rows = [np.full(Rr, p, dtype=np.float32) for p in SOFT_ROWS]
    cp = np.stack([rows[i % 2] for i in range(SOFT_BATCH)])
    prior = np.stack([R.prior_llr(np.concatenate([c.probs[: n - Rr], r.astype(np.float64)])) for r in rows])
    out = _case(c.H, c.probs, c.synd[:SOFT_BATCH], c.replaced, prior=prior[np.arange(SOFT_BATCH) % 2])
    out.cp, out.rows = cp, rows
    return out


@functools.lru_cache(maxsize=None)
def soft_oracle():
    """One oracle call per row of priors; each codeword takes the results of its own."""
    from oracle import pyoracle

    c, s = case("col32"), soft()
    ref = None
    for k, row in enumerate(s.rows):
        probs = np.concatenate([c.probs[: c.H.n - c.H.m], row.astype(np.float64)])
        r = pyoracle.bp_decode_batch(c.H, probs, s.synd, 0, MAX_ITER, "min_sum", alpha=1.0, dtype="f32", threads=4, early_exit=False)
        ref = ref or {key: v.copy() for key, v in r.items()}
        for key in ref:
            ref[key][k::2] = r[key][k::2]
    return ref


# ---- the sweeps ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep(kind, first):
    """Trials first ... first + 139 of mc_hqc_run (kind "hqc": omega 3, eps 0.02, HQC_SEED) or mc_fer_run ("fer": FER_SEED) on
    the base graph, by the law the device draws them by (tests/mc_ref.py), with the restatement on their syndromes.  The
    namespace of `case`, and y / msg or errors."""
    import mc_ref

    H, probs, _ = _graph("base")
    N = H.n - H.m
    if kind == "hqc":
        y, msg = mc_ref.hqc(HQC_SEED, first, SWEEP_RUNS, _cut_hin(H), 3, 0.02)
        out = _case(H, probs, np.ascontiguousarray(msg[:, N:]))
        out.y, out.msg = y, msg
    else:
        err, synd = mc_ref.fer(FER_SEED, first, SWEEP_RUNS, H, probs)
        out = _case(H, probs, np.ascontiguousarray(synd.astype(np.uint8)))
        out.errors = err
    return out


def _cut_hin(H):
    """Hin of [Hin | I]: every row without its last edge."""
    N, m = H.n - H.m, H.m
    rp, ci = np.asarray(H.row_ptr), np.asarray(H.col_idx)
    keep = np.ones(len(ci), dtype=bool)
    keep[rp[1:] - 1] = False
    return S.TannerGraph.from_csr(m, N, (rp - np.arange(m + 1)).astype(np.int64), ci[keep].astype(np.int32))


@functools.lru_cache(maxsize=None)
def sweep_oracle(kind, first, received=False):
    """The float32 oracle on a sweep's syndromes -- or (received, "hqc") on its received words msg = [0 | checks], whose decoded
    word is what the sweep's counters are counted on."""
    from oracle import pyoracle

    c = sweep(kind, first)
    return pyoracle.bp_decode_batch(c.H, c.probs, c.msg if received else c.synd, 1 if received else 0, MAX_ITER, "min_sum", alpha=1.0, dtype="f32",
                                    threads=max(1, min(8, pyoracle.max_threads())), early_exit=False)
