"""TEST INFRASTRUCTURE: seeded random CALL SEQUENCES on one live `BpDecoder`, shared by tests/test_handle_sequences.py (CPU:
the model's bookkeeping, that the sequences decide something, the coverage conditions) and
tests/test_handle_sequences_gpu.py (every decode of every sequence against the oracle and against a fresh decoder).

A handle caches many things, each valid for a key that a later call may change (scaldpc_bp.hip, struct scaldpc_bp: the
first-message table, the settle horizon, the prior-derived float64 ratios and Monte-Carlo thresholds, the lazily rebuilt
tables of a grown handle, message against record storage, the workspace and its counters, `async_used`).  Each has a test of
its own invalidation; the sequences here hold the interplay.

  Model       the handle's VISIBLE state in NumPy: the CSR graph (rows of [Hin | I], grown by appends), the shared priors
              as float64, the knobs.  It also restates which kernel family a call takes (`small_lds`, `el_limit`,
              `rec_form`, `first_fusable`, `plan_settle` of scaldpc_bp.hip), from the graph and the knobs alone: the coverage
              conditions are conditions on the inputs, never measurements.
  sequence    `sequence(family, seed)`: a list of plain tuples, from `np.random.RandomState(seed)` only.  SEQUENCES is the
              committed set.
  replay      `replay(ops, make_decoder, ...)`: runs a sequence on the model and on a decoder from the factory, hands every
              decode and sweep to the caller's checks, and names family, seed, step and the op prefix when one fails;
              `replay(prefix, ...)` reproduces it.

Graph families (the smallest at which each kernel family is still picked):
  A  an HQC-shaped [Hin | I] JUST too large for the LDS-resident decoder (W = 11, N about 1150, R about 610: 7 320 edges need
     62.7 KB against small_lds' 60 KiB; the 250 ... 500 rows first thought of all fit, with any W <= 11): the tile kernels,
     the row-parallel kernels, compaction, the default settle = 2
  B  the same with one to three heavy columns (31 or 32, 48, and 30 ... 47 edges): minsum_rec 0, 1 and 2 pick different
     forms, appended rows carry a column across 32/33 and 64/65
  C  tests/golden/generators.json's regular_identity_300_150_3_6: fits the LDS; "stream" / "edge" pin the other families
"""
import functools
import json
import os

import numpy as np

from helpers import S, hqc_instance

TW = 64
LDS_LIMIT = 60 * 1024  # small_lds
EL_DEFAULT = {"min_sum": 6, "product_sum": 4}  # el_limit
REC_COLS = {0: 0, 1: 32, 2: 64}  # rec_form: the widest column of the record form under minsum_rec
FAMILIES = ("A", "B", "C")
BATCHES = (1, 5, 9, 63, 64, 65, 130)
MAX_ITERS = (1, 2, 3, 8, 20, 30)
TANH_ITERS = (1, 2, 3, 8)  # tests/test_bp_property_gpu.py caps the tanh rule at 10 (8 with p = 0 priors), for the reason it gives
ALPHAS = (1.0, 0.75, 0.0)  # 0 = the schedule 1 - 2^-it
SWEEP_RUNS = 130
DEFAULT_KNOBS = dict(path="auto", split=2, first_fused=1, fuse_test=1, minsum_rec=1, settle=-1, settle_horizon=0,
                     compact_after=-1, el_max=-1, tile_group=0)
SENTINEL = dict(bits=0xAB, llr=-3.5, iters=-4, converged=0xCD)  # what a refused call must leave in its outputs


# ---- what scaldpc_bp.hip decides from the graph and the knobs ----------------------------------------------------------------
def small_lds_bytes(E, n, m):
    return 2 * E * 4 + 2 * n + m + 64


def alpha_at(alpha, it):
    return np.float32(1.0 - 2.0 ** (-it)) if alpha == 0.0 else np.float32(alpha)


class Model:
    """The visible state of one live handle."""

    def __init__(self, family, graph_seed):
        self.family, self.graph_seed = family, graph_seed
        self.N, rows, self.probs, self.heavy, self.omega, self.eps, self.W = _base(family, graph_seed)
        self.rows = [np.asarray(r, dtype=np.int32) for r in rows]  # ascending columns per check, identity column last
        self.n = self.N + len(self.rows)
        self.knobs = dict(DEFAULT_KNOBS)
        self.explicit = {}  # the knobs somebody set, in order: what a fresh decoder is configured with
        self._graph = None

    m = property(lambda self: len(self.rows))
    E = property(lambda self: int(sum(len(r) for r in self.rows)))

    def graph(self):
        if self._graph is None:
            rp = np.concatenate([[0], np.cumsum([len(r) for r in self.rows])]).astype(np.int64)
            self._graph = S.TannerGraph.from_csr(self.m, self.n, rp, np.concatenate(self.rows))
        return self._graph

    def hin(self):
        rp = np.concatenate([[0], np.cumsum([len(r) - 1 for r in self.rows])]).astype(np.int64)
        return S.TannerGraph.from_csr(self.m, self.N, rp, np.concatenate([r[:-1] for r in self.rows]))

    def col_degrees(self):
        return np.bincount(np.concatenate(self.rows), minlength=self.n)

    def max_row(self):
        return max(len(r) for r in self.rows)

    # -- the operations ------------------------------------------------------------------------------------------------
    def configure(self, items):
        for k, v in items:
            assert k in DEFAULT_KNOBS, k
            self.knobs[k] = v
            self.explicit[k] = v

    def new_probs(self, seed):
        """Shared priors: the secret's columns at a new weight, the checks at 0, 0.01 ... 0.1; p = 0 on a few secret columns."""
        rng = np.random.RandomState(seed)
        p = np.concatenate([np.full(self.N, rng.randint(2, 6) / self.N),
                            rng.choice([0.0, 0.01, 0.03, 0.05, 0.1], size=self.m, p=[0.1, 0.2, 0.3, 0.3, 0.1])])
        p[rng.choice(self.N, size=3, replace=False)] = 0.0
        return p

    def new_rows(self, count, heavy_col, seed):
        """`count` HQC-style rows: W columns of the secret (plus `heavy_col` when >= 0), each with its identity column; and the
        priors of those.  Returns (row_ptr, col_idx, new_n, tail, rows)."""
        rng = np.random.RandomState(seed)
        rows = []
        for i in range(count):
            pool = np.setdiff1d(np.arange(self.N), [heavy_col]) if heavy_col >= 0 else np.arange(self.N)
            cols = set(rng.choice(pool, size=self.W, replace=False).tolist())
            if heavy_col >= 0:
                cols.add(int(heavy_col))
            rows.append(np.array(sorted(cols) + [self.n + i], dtype=np.int32))
        tail = rng.choice([0.0, 0.02, 0.05], size=count, p=[0.15, 0.45, 0.4])
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return rp, np.concatenate(rows), self.n + count, tail, rows

    def append(self, rows, tail):
        self.rows += rows
        self.n += len(rows)
        self.probs = np.concatenate([self.probs, tail])
        self._graph = None

    # -- which kernels a call takes ------------------------------------------------------------------------------------
    def takes_lds(self):
        return self.E > 0 and small_lds_bytes(self.E, self.n, self.m) <= LDS_LIMIT and self.knobs["path"] in ("auto", "lds")

    def el_limit(self, method):
        if self.E == 0 or self.max_row() > 64 or self.col_degrees().max() > 64:
            return 0
        lim = EL_DEFAULT[method] if self.knobs["el_max"] < 0 else self.knobs["el_max"]
        lim = {"stream": 0, "edge": TW}.get(self.knobs["path"], lim)
        return max(0, min(lim, TW))

    def rec_form(self, method):
        return (method == "min_sum" and self.knobs["minsum_rec"] != 0 and self.max_row() <= 64
                and self.col_degrees().max() <= REC_COLS[self.knobs["minsum_rec"]])

    def path_of(self, batch, method, precision):
        if precision == "float64":
            return "f64"
        if self.takes_lds():
            return "lds"
        return "edge" if batch <= TW and batch <= self.el_limit(method) else "tile"

    def settle_mode(self):
        return 2 if self.knobs["settle"] < 0 else self.knobs["settle"]  # (every graph here is [Hin | I])

    def decode_info(self, op):
        _, batch, max_iter, early, kind, want_llr, prior, method, alpha, precision, io, mix, seed = op
        path = self.path_of(batch, method, precision)
        tile = path == "tile"
        rec = tile and self.rec_form(method)
        narrow = self.max_row() <= 64 and self.col_degrees().max() <= 64
        ff = tile and bool(self.knobs["first_fused"]) and prior == "shared" and narrow
        tracked = rec and not early and io != "async" and self.settle_mode() >= 1 and max_iter >= 3
        learn = (tracked and self.settle_mode() == 2 and self.knobs["settle_horizon"] == 0 and mix == "easy"
                 and max_iter >= 20 and alpha != 0.0)
        return dict(kind="decode", path=path, T=(batch + TW - 1) // TW, rec=rec, ff=ff, tracked=tracked, learn=learn,
                    key=(max_iter, alpha, prior != "shared"), alpha1=float(alpha_at(alpha, 1)), batch=batch, max_iter=max_iter,
                    early=early, method=method, precision=precision, io=io, mix=mix, prior=prior, alpha=alpha,
                    settle2=tracked and self.settle_mode() == 2 and self.knobs["settle_horizon"] == 0,
                    forced=self.knobs["settle_horizon"] if tracked and self.settle_mode() == 2 else 0,
                    minsum_rec=self.knobs["minsum_rec"], family=self.family,
                    compacts=tile and early and mix == "mixed" and batch > TW and self.knobs["compact_after"] != 0 and max_iter >= 20)


def _base(family, seed):
    """(N, rows, priors, heavy columns, omega, eps, W) of a family's graph number `seed`."""
    trials = __import__("importlib").import_module("sca-ldpc_amd.trials")
    if family == "C":
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generators.json")) as fh:
            g = S.TannerGraph.from_coo(json.load(fh)[f"regular_identity_300_150_3_6_s{seed % 2}"])
        N, omega, eps = 300, 3, 0.03
        rows = [g.col_idx[g.row_ptr[r] : g.row_ptr[r + 1]] for r in range(g.m)]
        assert all(r[-1] == N + i for i, r in enumerate(rows))
        return N, rows, trials.hqc_priors(N, g.m, omega, eps), [], omega, eps, 6
    N, W, R, omega, eps = 1100 + 17 * (seed % 5), 11, 610 + 7 * (seed % 3), 3, 0.02
    H, _, probs, _, _ = hqc_instance(N, W, R, omega, eps, 1, seed=900 + seed, flip=False)
    rows = [H.col_idx[H.row_ptr[r] : H.row_ptr[r + 1]].copy() for r in range(R)]
    heavy = []
    if family == "B":
        rng = np.random.RandomState(7000 + seed)
        cdeg = np.bincount(H.col_idx, minlength=H.n)
        targets = [31 + seed % 2, 48, 30 + int(rng.randint(18))][: 1 + seed % 3]
        heavy = [int(c) for c in rng.choice(np.flatnonzero(cdeg[:N] <= 10), size=len(targets), replace=False)]
        for c, want in zip(heavy, targets):
            free = [r for r in range(R) if c not in rows[r]]
            for r in rng.choice(free, size=want - int(cdeg[c]), replace=False):
                rows[r] = np.concatenate([np.sort(np.append(rows[r][:-1], c)), rows[r][-1:]]).astype(np.int32)
    return N, rows, probs, heavy, omega, eps, W


# ---- inputs ------------------------------------------------------------------------------------------------------------------
MIXES = {"easy": (0, 1, 1, 1), "mixed": (0, 1, 2, 1, 1, 2, 3, 1), "hard": None}


def error_words(model, batch, mix, seed):
    """uint8 [batch, n] error words e = [y | flips]; their syndrome H e = Hin y ^ flips is what a decode is given (or e itself,
    as a received word).  Classes: 0 = the zero word (converges at iteration 1), 1 = a light secret and the odd flipped
    check, 2 = a heavier one (a straggler), 3 = a random word (never converges).  "hard": the first tile easy, the rest random."""
    rng = np.random.RandomState(seed)
    N, n = model.N, model.n
    e = np.zeros((batch, n), dtype=np.uint8)
    for b in range(batch):
        cls = (3 if b >= TW else MIXES["easy"][b % 4]) if mix == "hard" else MIXES[mix][b % len(MIXES[mix])]
        if cls in (1, 2):
            e[b, rng.choice(N, size=rng.randint(1, 4) if cls == 1 else rng.randint(5, 10), replace=False)] = 1
            e[b, N:] = rng.rand(n - N) < (0.004 if cls == 1 else 0.03)
        elif cls == 3:
            e[b] = rng.rand(n) < 0.3
    return e


def codeword_priors(model, batch, prior, seed):
    """None, or float32 [batch, k] per-codeword probabilities of the last k columns: k = R (the checks) or k = n; p = 0 among them."""
    if prior == "shared":
        return None
    rng = np.random.RandomState(seed + 1)
    cp = rng.choice([0.0, 0.02, 0.05, 0.2], size=(batch, model.m), p=[0.1, 0.4, 0.4, 0.1])
    if prior == "full":
        cp = np.concatenate([rng.choice([0.0, 2.0, 4.0], size=(batch, model.N), p=[0.01, 0.49, 0.5]) / model.N, cp], axis=1)
    return np.ascontiguousarray(cp, dtype=np.float32)


def full_priors(model_probs, cp):
    """float64 [batch, n]: the shared priors with every codeword's own columns put in."""
    out = np.repeat(np.asarray(model_probs, dtype=np.float64)[None, :], cp.shape[0], axis=0)
    out[:, out.shape[1] - cp.shape[1] :] = cp.astype(np.float64)
    return out


ORACLE_METHOD = {"min_sum": "min_sum", "product_sum": "tanh_complement"}


def oracle_decode(graph, probs, cp, x, kind, max_iter, method, alpha, precision, early, threads=4, perturb=None):
    """The answer key of one decode: the f32 oracle in the kernels' operation order, or (float64) its method 0; with
    per-codeword priors, one call per codeword on that codeword's full prior vector."""
    from oracle import pyoracle

    name, dtype = ("product_sum", "f64") if precision == "float64" else (ORACLE_METHOD[method], "f32")
    with np.errstate(divide="ignore", invalid="ignore"):
        if cp is None:
            return pyoracle.bp_decode_batch(graph, probs, x, kind, max_iter, name, alpha=alpha, dtype=dtype, threads=threads,
                                            early_exit=early)
        full = full_priors(probs, cp)
        outs = [pyoracle.bp_decode_batch(graph, full[b], x[b : b + 1], kind, max_iter, name, alpha=alpha, dtype=dtype, threads=1,
                                         early_exit=early) for b in range(x.shape[0])]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def D(batch=130, max_iter=20, early=False, kind="syndrome", want_llr=True, prior="shared", method="min_sum", alpha=1.0,
      precision="float32", io="host", mix="easy", seed=0):
    return ("decode", batch, max_iter, early, kind, want_llr, prior, method, alpha, precision, io, mix, seed)


def _need(model, **kn):
    """A configure op for the knobs that are not yet as a motif needs them."""
    items = tuple((k, v) for k, v in kn.items() if model.knobs[k] != v)
    return [("configure", items)] if items else []


def _tile_knobs(model, rec=None):
    """Knobs under which a 65+ codeword min-sum call runs the tile kernels (and, rec: in the record form)."""
    kn = {}
    if model.takes_lds() or model.knobs["path"] == "edge":
        kn["path"] = "stream"
    if rec and not model.rec_form("min_sum"):
        kn["minsum_rec"] = 2 if model.col_degrees().max() > 32 else 1
    return kn


def _learn(model, rng, **kw):
    """A settle = 2 learning call: record form, fixed iterations, three tiles of easy trials, no horizon forced."""
    return D(batch=130, max_iter=30, early=False, mix="easy", seed=int(rng.randint(1 << 30)), **kw)


def _motifs():
    """name -> (families, function(model, rng) -> ops).  A motif first sets the knobs it depends on."""
    r30 = lambda rng: int(rng.randint(1 << 30))
    settle2 = dict(settle=2, settle_horizon=0)

    def rec_tanh_rec(m, rng):
        s = r30(rng)
        return _need(m, **_tile_knobs(m, rec=True)) + [D(seed=s, mix="mixed"), D(method="product_sum", max_iter=8, seed=s, mix="mixed"),
                                                        D(seed=s, mix="mixed", batch=65)]

    def ff_update(m, rng):
        d = D(method=rng.choice(["min_sum", "product_sum"]).item(), max_iter=8, early=bool(rng.randint(2)), seed=r30(rng), mix="mixed")
        return _need(m, first_fused=1, **_tile_knobs(m)) + [d, ("update_probs", r30(rng)), d]

    def ff_alpha(m, rng):
        a = rng.permutation(ALPHAS)
        s = r30(rng)
        return _need(m, first_fused=1, **_tile_knobs(m)) + [D(alpha=float(a[0]), seed=s, mix="mixed", early=True),
                                                             D(alpha=float(a[1]), seed=s, mix="mixed", early=True)]

    def ff_method(m, rng):
        s = r30(rng)
        return _need(m, first_fused=1, **_tile_knobs(m)) + [D(seed=s, max_iter=8, mix="mixed"), D(method="product_sum", max_iter=8, seed=s, mix="mixed"),
                                                             D(seed=s, max_iter=8, mix="mixed", kind="received")]

    def learn_then(what):
        def f(m, rng):
            first = _learn(m, rng)
            s = first[-1]
            nxt = {"same": [D(batch=130, max_iter=30, seed=s)],
                   "iter": [D(batch=130, max_iter=20, seed=s)],
                   "alpha": [D(batch=130, max_iter=30, alpha=0.75, seed=s)],
                   "soft": [D(batch=130, max_iter=30, prior="tail", seed=s)],
                   "append": [("append", int(rng.randint(1, 9)), -1, r30(rng)), D(batch=130, max_iter=30, seed=s)],
                   "update": [("update_probs", r30(rng)), D(batch=130, max_iter=30, seed=s)],
                   "group": [("configure", (("tile_group", 1 + int(rng.randint(3))),)), D(batch=130, max_iter=30, seed=s)]}[what]
            return _need(m, **settle2, **_tile_knobs(m, rec=True)) + [first] + nxt
        return f

    def rec_flip(m, rng):
        s = r30(rng)
        order = [int(v) for v in rng.permutation(3)]
        ops = _need(m, **_tile_knobs(m))
        for v in order:
            ops += [("configure", (("minsum_rec", v),)), D(seed=s, mix="mixed", max_iter=8)]
        return ops + [("probe",)]

    def append2(batch):
        def f(m, rng):
            kn = _tile_knobs(m) if batch > TW else dict({"path": "edge"} if m.takes_lds() or m.knobs["path"] == "stream" else {},
                                                        **({"el_max": -1} if m.knobs["el_max"] in (0,) else {}))
            return _need(m, **kn) + [("append", int(rng.randint(1, 6)), -1, r30(rng)), ("append", int(rng.randint(1, 40)), -1, r30(rng)),
                                     D(batch=batch, max_iter=8, early=True, seed=r30(rng), mix="mixed",
                                       method=rng.choice(["min_sum", "product_sum"]).item())]
        return f

    def cross(line):
        def f(m, rng):
            below = [c for c in m.heavy if m.col_degrees()[c] <= line]
            if not below:
                return None
            col = max(below, key=lambda c: m.col_degrees()[c])  # the one nearest to the line
            s = r30(rng)
            count = line + 1 - int(m.col_degrees()[col])
            if count > 24:
                return None
            return (_need(m, minsum_rec=2, **settle2, **_tile_knobs(m)) + [_learn(m, rng)]
                    + [("append", k, col, r30(rng)) for k in (count // 2, count - count // 2) if k]  # (the second one crosses)
                    + [D(batch=130, max_iter=30, seed=s, mix="mixed")])
        return f

    def tiles_131(m, rng):
        s = r30(rng)
        early = bool(rng.randint(2))
        return _need(m, **({"path": "stream"} if m.knobs["path"] != "stream" else {})) + [
            D(batch=int(rng.choice([9, 63, 64])), early=early, seed=s, mix="mixed"), D(batch=130, early=early, seed=s, mix="mixed"),
            D(batch=int(rng.choice([5, 9, 64])), early=early, seed=s, mix="mixed")]

    def iter_grow(m, rng):
        s = r30(rng)
        b = int(rng.choice([5, 65]))
        return _need(m, **({"path": "stream"} if m.takes_lds() else {})) + [D(batch=b, max_iter=2, early=True, seed=s, mix="mixed"),
                                                                           D(batch=b, max_iter=8, early=True, seed=s, mix="mixed"),
                                                                           D(batch=b, max_iter=30, early=True, seed=s, mix="mixed")]

    def f64_between(m, rng):
        s = r30(rng)
        nb = int(rng.choice([9, 65]))
        return [D(batch=nb, seed=s, mix="mixed", max_iter=8), D(batch=int(rng.choice([5, 130])), method="product_sum", precision="float64",
                                                                 max_iter=8, early=True, seed=s, mix="mixed"),
                D(batch=nb + 56, seed=s, mix="mixed", max_iter=8)]

    def f64_update(m, rng):
        d = D(batch=65, method="product_sum", precision="float64", max_iter=8, early=True, seed=r30(rng), mix="mixed",
              prior=rng.choice(["shared", "shared", "tail"]).item())
        return [d, ("update_probs", r30(rng)), d]

    def sweep_update(m, rng):
        s = ("sweep", "fer", r30(rng), 8, bool(rng.randint(2)), 1.0)
        return [s, ("update_probs", r30(rng)), s]

    def sweep_append(m, rng):
        s = ("sweep", "hqc", r30(rng), 20, True, float(rng.choice(ALPHAS)))
        return [s, ("append", int(rng.randint(1, 30)), -1, r30(rng)), s]

    def compaction(bigger):
        def f(m, rng):
            s = r30(rng)
            first, second = (65, 130) if bigger else (130, int(rng.choice([5, 9, 63])))
            ca = int(rng.choice([-1, 2, 4]))
            return _need(m, compact_after=ca, **_tile_knobs(m)) + [D(batch=first, max_iter=30, early=True, seed=s, mix="mixed",
                                                                     want_llr=bool(rng.randint(2))),
                                                                   D(batch=second, max_iter=30, early=True, seed=s, mix="mixed")]
        return f

    def asynchronous(m, rng):
        s = r30(rng)
        return [D(batch=int(rng.choice([65, 130])), max_iter=8, io="async", seed=s, mix="mixed",
                  method=rng.choice(["min_sum", "product_sum"]).item()),
                D(batch=9, max_iter=8, seed=s, mix="mixed"), ("append", int(rng.randint(1, 20)), -1, r30(rng)),
                D(batch=65, max_iter=8, early=True, seed=s, mix="mixed")]

    def refused(m, rng):
        return [("refused", rng.choice(["high", "nan"]).item(), int(rng.choice([5, 65]))), D(batch=65, max_iter=8, seed=r30(rng), mix="mixed")]

    def refused_sweep(m, rng):
        return [("refused", rng.choice(["high", "nan"]).item(), 65), ("sweep", "fer", r30(rng), 8, True, 1.0),
                D(batch=9, max_iter=8, seed=r30(rng), mix="mixed")]

    def append_lds(m, rng):
        ops = _need(m, path="auto") + [("append", int(rng.randint(1, 6)), -1, r30(rng)), ("append", int(rng.randint(1, 40)), -1, r30(rng))]
        return ops + [D(batch=int(rng.choice([5, 65])), max_iter=8, early=True, seed=r30(rng), mix="mixed",
                        method=rng.choice(["min_sum", "product_sum"]).item())]

    def probe_equal(m, rng):
        d = D(batch=int(rng.choice([65, 130])), max_iter=20, early=bool(rng.randint(2)), seed=r30(rng), mix="mixed",
              alpha=float(rng.choice(ALPHAS)))
        return _need(m, **_tile_knobs(m)) + [d, ("probe",), d]

    def short_horizon(m, rng):
        s = r30(rng)
        return (_need(m, settle=2, **_tile_knobs(m, rec=True)) + [("configure", (("settle_horizon", int(rng.choice([3, 4]))),)),
                                                                 D(batch=130, max_iter=20, seed=s, mix="hard", want_llr=bool(rng.randint(2))),
                                                                 ("configure", (("settle_horizon", 0),))])

    everywhere = FAMILIES
    out = {"rec_tanh_rec": (everywhere, rec_tanh_rec), "ff_update": (everywhere, ff_update), "ff_alpha": (everywhere, ff_alpha),
           "ff_method": (everywhere, ff_method), "rec_flip": ("B", rec_flip), "append2_tile": (everywhere, append2(130)),
           "append2_edge": (everywhere, append2(3)), "cross33": ("B", cross(32)), "cross65": ("B", cross(64)),
           "tiles_131": (everywhere, tiles_131), "iter_grow": (everywhere, iter_grow), "f64_between": (everywhere, f64_between),
           "f64_update": (everywhere, f64_update), "sweep_update": (everywhere, sweep_update), "sweep_append": (everywhere, sweep_append),
           "compact_smaller": ("AB", compaction(False)), "compact_larger": ("AB", compaction(True)),
           "async": (everywhere, asynchronous), "refused": (everywhere, refused), "refused_sweep": (everywhere, refused_sweep),
           "append_lds": ("C", append_lds), "probe_equal": (everywhere, probe_equal),
           "short_horizon": ("AB", short_horizon)}
    for what in ("same", "iter", "alpha", "soft", "append", "update", "group"):
        out["learn_" + what] = ("AB", learn_then(what))
    return out


MOTIFS = _motifs()
SEQUENCE_SEEDS = {"A": range(14), "B": range(14), "C": range(12)}  # 40 sequences
MIN_OPS, MAX_OPS = 10, 16  # operations after the opening one


def _filler(model, rng):
    """One random op: a knob or two, a decode of any variant, a probe."""
    r = rng.randint(10)
    if r < 3:
        choices = [("split", int(rng.randint(1, 4))), ("first_fused", int(rng.randint(2))), ("fuse_test", int(rng.randint(2))),
                   ("compact_after", int(rng.choice([0, 2, 4]))), ("el_max", int(rng.choice([-1, 0, 4, 9]))),
                   ("tile_group", int(rng.randint(4))), ("settle", int(rng.choice([-1, 0, 1, 2]))),
                   ("path", rng.choice(["auto", "stream", "edge"]).item()), ("minsum_rec", int(rng.randint(3)))]
        pick = rng.choice(len(choices), size=1 + rng.randint(2), replace=False)
        return ("configure", tuple(choices[i] for i in pick))
    if r == 3:
        return ("probe",)
    method = rng.choice(["min_sum", "product_sum"]).item()
    precision = "float64" if method == "product_sum" and rng.randint(3) == 0 else "float32"
    early = bool(rng.randint(2))
    io = rng.choice(["host", "host", "device", "async"]).item()
    if io == "async" and (early or precision == "float64"):
        io = "device"
    prior = rng.choice(["shared", "shared", "tail", "full"]).item() if io != "async" else "shared"
    return D(batch=int(rng.choice(BATCHES)), max_iter=int(rng.choice(MAX_ITERS if method == "min_sum" else TANH_ITERS)), early=early,
             kind=rng.choice(["syndrome", "received"]).item(), want_llr=bool(rng.randint(4)), prior=prior, method=method,
             alpha=float(rng.choice(ALPHAS)) if method == "min_sum" else 1.0, precision=precision, io=io,
             mix=rng.choice(["easy", "mixed", "mixed", "hard"]).item(), seed=int(rng.randint(1 << 30)))


def _deck(family):
    """The family's motifs in the order its sequences take them: the fewer families a motif has, the more often it is dealt,
    so that each comes up at least three times over the set."""
    deck = []
    for rep in range(3):
        for name, (fam, _) in MOTIFS.items():
            if family in fam and fam != "B" and rep < {1: 3, 2: 2, 3: 2 if family == "C" else 1}[len(fam)]:
                deck.append(name)
    return deck


@functools.lru_cache(maxsize=None)
def _plan(family):
    """seed -> op list, for the family's seeds in order: each sequence takes motifs from where the one before stopped, as many
    as fit, with random ops between them.  All randomness of sequence (family, seed) comes from its own RandomState."""
    deck, at, out, pending = _deck(family), 0, {}, []
    for seed in SEQUENCE_SEEDS[family]:
        rng = np.random.RandomState(100_000 * (1 + FAMILIES.index(family)) + seed)
        ops = [("open", family, seed)]
        model = Model(family, seed)

        def take(new):
            for op in new:
                ops.append(op)
                if op[0] == "configure":
                    model.configure(op[1])
                elif op[0] == "append":
                    _, _, _, tail, rows = model.new_rows(*op[1:])
                    model.append(rows, tail)
                elif op[0] == "update_probs":
                    model.probs = model.new_probs(op[1])

        if family == "B":  # its own three motifs in turn, first (cross65 needs the second heavy column: 1 + seed % 3 >= 2 of them)
            pending.insert(0, ("cross33", "cross65", "rec_flip")[seed % 3])
        for _ in range(len(deck)):  # (bounded: a motif that does not suit this graph goes back for the next sequence)
            name = pending.pop(0) if pending else deck[at % len(deck)]
            new = MOTIFS[name][1](model, rng)
            if new is None or len(ops) - 1 + len(new) > MAX_OPS:
                pending.append(name)
                if new is not None:
                    break
                at += 0 if name != deck[at % len(deck)] else 1
                continue
            take(new)
            at += 0 if name != deck[at % len(deck)] else 1
            if rng.randint(3) == 0 and len(ops) - 1 < MAX_OPS - 6:
                take([_filler(model, rng)])
        while len(ops) - 1 < MIN_OPS:
            take([_filler(model, rng)])
        out[seed] = tuple(ops)
    return out


def sequence(family, seed):
    """The op list of (family, seed)."""
    return list(_plan(family)[seed])


SEQUENCES = [(f, s) for f in FAMILIES for s in SEQUENCE_SEEDS[f]]


# ---- replay ------------------------------------------------------------------------------------------------------------------
class SequenceFailure(AssertionError):
    pass


def replay(ops, make_decoder=None, on_decode=None, on_sweep=None, on_state=None, label=None):
    """Runs `ops` on a Model and, with a factory `make_decoder(graph, probs, knobs) -> decoder`, on one live decoder.

      on_decode(step, model, args, got, dec)  after every decode: args = dict(x, kind, cp, max_iter, early, want_llr, method, alpha,
                                              precision, io), got = the decoder's result
      on_sweep(step, model, args, got, dec)   after every sweep
      on_state(step, model, dec)              after every append and prior update
    Returns the per-step records (dicts: the op, what the model says about it, and the decoder's result where there is one).
    Any failure is re-raised as SequenceFailure naming the sequence, the step and the op prefix that reproduces it."""
    assert ops and ops[0][0] == "open", "a sequence starts with ('open', family, graph_seed)"
    label = label or f"family {ops[0][1]} seed {ops[0][2]}"
    model = Model(ops[0][1], ops[0][2])
    dec = make_decoder(model.graph(), model.probs.copy(), {}) if make_decoder else None
    records = [dict(op=ops[0], kind="open")]
    last_tile = False  # the step before was a decode on the tile kernels: time_kernels has something to time
    try:
        for step, op in enumerate(ops[1:], start=1):
            try:
                rec = _step(step, op, model, dec, on_decode, on_sweep, on_state, last_tile)
            except Exception as e:  # noqa: BLE001  (library errors too: the prefix is what reproduces them)
                raise SequenceFailure(f"{label}: step {step} {op!r} failed: {type(e).__name__}: {e}\n"
                                      f"replay(ops) with ops = {list(ops[: step + 1])!r}") from e
            last_tile = rec["kind"] == "decode" and rec["path"] == "tile" and rec["io"] != "async"
            records.append(rec)
    finally:
        if dec is not None:
            dec.close()
    return records


def _step(step, op, model, dec, on_decode, on_sweep, on_state, last_tile):
    what = op[0]
    if what == "decode":
        info = model.decode_info(op)
        _, batch, max_iter, early, kind, want_llr, prior, method, alpha, precision, io, mix, seed = op
        e = error_words(model, batch, mix, seed)
        x = np.ascontiguousarray(model.graph().syndrome(e) if kind == "syndrome" else e, dtype=np.uint8)
        args = dict(x=x, kind=kind, cp=codeword_priors(model, batch, prior, seed), max_iter=max_iter, early=early,
                    want_llr=want_llr, method=method, alpha=alpha, precision=precision, io=io)
        rec = dict(op=op, args=args, **info)
        if dec is not None:
            got = dec.decode(**args)
            assert got["bits"].shape == (batch, model.n) and got["iters"].shape == (batch,) and got["converged"].shape == (batch,)
            assert (got["llr"] is None) == (not want_llr) and (got["llr"] is None or got["llr"].shape == (batch, model.n))
            rec["got"] = got
            if on_decode:
                on_decode(step, model, args, got, dec)
        return rec
    if what == "configure":
        model.configure(op[1])
        if dec is not None:
            dec.configure(dict(op[1]))
        return dict(op=op, kind="configure")
    if what == "update_probs":
        model.probs = model.new_probs(op[1])
        if dec is not None:
            dec.update_channel_probs(model.probs.copy())
            if on_state:
                on_state(step, model, dec)
        return dict(op=op, kind="update_probs")
    if what == "append":
        before = model.col_degrees()
        rp, ci, new_n, tail, rows = model.new_rows(*op[1:])
        model.append(rows, tail)
        after = model.col_degrees()[: len(before)]
        if dec is not None:
            dec.append_rows(rp, ci, new_n, tail)
            if on_state:
                on_state(step, model, dec)
        grown = np.flatnonzero(after != before)
        return dict(op=op, kind="append", minsum_rec=model.knobs["minsum_rec"],
                    crossings=[(int(before[c]), int(after[c])) for c in grown])
    if what == "sweep":
        _, kind, seed, max_iter, early, alpha = op
        args = dict(kind=kind, runs=SWEEP_RUNS, seed=seed, first=2**32 - 30, max_iter=max_iter, early=early, alpha=alpha,
                    omega=model.omega, eps=model.eps)
        rec = dict(op=op, kind="sweep", sweep=kind)
        if dec is not None:
            got = dec.sweep(**args)
            rec["got"] = got
            if on_sweep:
                on_sweep(step, model, args, got, dec)
        return rec
    if what == "probe":
        if dec is not None:
            dec.probe(last_tile)
        return dict(op=op, kind="probe", timed=last_tile)
    if what == "refused":
        _, bad, batch = op
        e = error_words(model, batch, "mixed", 5)
        cp = codeword_priors(model, batch, "tail", 5)
        cp[batch - 1, model.m // 2] = 1.5 if bad == "high" else np.nan
        if dec is not None:
            left = dec.refused(x=np.ascontiguousarray(model.graph().syndrome(e)), kind="syndrome", cp=cp, max_iter=8)
            assert left["raised"] is ValueError, f"the call was not refused with ValueError: {left['raised']}"
            for k, v in SENTINEL.items():
                assert (left[k] == v).all(), f"the refused call wrote to its {k} output"
        return dict(op=op, kind="refused")
    raise ValueError(f"unknown op {op!r}")
