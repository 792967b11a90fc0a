"""Single-pass answer key for the check and variable kernels: graphs on which ONE message is the posterior.

`star_forest`: disjoint stars, one check per row, every column on exactly one edge.  One "probe" variable per row has
prior p = 0.5, LLR exactly 0, so its posterior after any number of iterations IS the check-to-variable message on its
edge (0 + c2v, no rounding), and every iteration recomputes that message from the same inputs (the other columns
have one edge each: they always send their prior).  The true message is a float64 one-liner (`true_message`):
with phi(a) = -log tanh(a/2) = log1p(2 / expm1(a)) the magnitude is phi(sum_k phi(|x_k|)), the sign the parity of the
negative inputs xor the syndrome bit.  The inputs x_k are the library's own float32 priors, logf((1.0f - p) / p) of
p = (float)prob (`prior32`), so the key owes nothing to any decoder, oracle included.

`comb`: a hub variable of degree c with prior a0, every edge to a two-edge check whose other end is a leaf with prior
x_j: a depth-2 tree, every posterior a signed sum of priors from the second iteration on (`true_comb_posteriors`).

Errors are counted in u(L) = 2^-24 * max(1, |L|) (stars) and u' = 2^-24 * (sum of the |terms| of the signed sum) (combs).

No GPU and no oracle in here.  All |x| <= 85: 2 / (e^85 + 1) = 2.4e-37 is a normal float32, so no intermediate goes
denormal; the band 87.3 < |x| < 88.7, where a float32 message turns infinite a hair earlier or later, is a documented
saturation difference (tests/helpers.compare) and deliberately not probed.
"""
import ctypes
import importlib

import numpy as np

S = importlib.import_module("sca-ldpc_amd")

EPS = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
BANDS = (16, 32, 64, 1 << 30)  # row degree <= 16, <= 32, <= 64, wider: the `with_cap` ladder of the check kernels


def band_of(deg):
    return next(b for b in BANDS if deg <= b)


def band_name(b):
    return f"<={b}" if b < (1 << 30) else ">64"


_LIBM = None


def prior32(probs):
    """logf((1.0f - p) / p) with the host's libm, float32 throughout: `prior_llrs`, `k_soft_convert` and the oracle's
    initial message, bit for bit (the same recipe as tests/test_hqc_soft_mc.host_llr)."""
    global _LIBM
    if _LIBM is None:
        _LIBM = ctypes.CDLL("libm.so.6")
        _LIBM.logf.restype, _LIBM.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    p = np.asarray(probs, dtype=np.float32)
    with np.errstate(divide="ignore"):
        x = (np.float32(1.0) - p) / p
    uniq, inv = np.unique(x.ravel(), return_inverse=True)
    vals = np.array([_LIBM.logf(float(v)) for v in uniq], dtype=np.float32)
    return vals[inv].reshape(x.shape)


def phi(a):
    """-log tanh(a / 2) for a >= 0 in float64, stable at both ends: phi(0) = inf, phi(inf) = 0, phi(phi(a)) = a."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        return np.log1p(2.0 / np.expm1(a))


def true_message(x, synd_bit=0):
    """The tanh rule's check-to-variable message from the OTHER inputs `x` of the row (float64 of the float32 LLRs;
    +-inf allowed) under syndrome bit `synd_bit`: the exact value, to float64 rounding."""
    x = np.asarray(x, dtype=np.float64)
    mag = float(phi(phi(np.abs(x)).sum()))
    neg = int((x < 0).sum()) + int(synd_bit)
    return -mag if neg & 1 else mag


def true_minsum_message(x, synd_bit=0, alpha=1.0):
    """Min-sum's message, float32 bit for bit as the oracle's code forms it (oracle/bp_oracle_impl.h, method 1): the
    running minimum starts at FLT_MAX (so a row of certainties sends FLT_MAX, not inf), the magnitude is multiplied by
    (+-1 * alpha) in float32 (one rounding: fl(alpha * min)), and an input <= 0 counts as negative."""
    x = np.asarray(x, dtype=np.float32)
    mn = np.float32(min(FLT_MAX, float(np.abs(x).min()))) if x.size else np.float32(FLT_MAX)
    neg = int((x <= 0).sum()) + int(synd_bit)
    return np.float32(mn * (np.float32(-1.0 if neg & 1 else 1.0) * np.float32(alpha)))


def unit(L):
    """u(L) = 2^-24 * max(1, |L|); inf for an infinite L (such probes are compared for equality instead)."""
    return EPS * np.maximum(1.0, np.abs(np.asarray(L, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ magnitude profiles
# Each takes (rng, k = number of sources, d = row degree) and returns k magnitudes in (0, 85].  Every profile keeps the
# message informative at every degree (|truth| > 1e-3 on at least 90 % of the probes of every (band, profile) cell,
# tests/test_message_probes.py): "all tiny" and "log-uniform over 1e-3 .. 80" were tried and dropped, because on wide rows
# their message underflows to 0 and the error is trivially 0 -- here the small magnitudes come one, two or three at a
# time among large ones instead.
def _hqc(rng, k, d):  # the workload's own: omega / N = 66 / 17669 -> 5.58, eps = 0.05 -> 2.94
    return np.where(rng.rand(k) < 0.9, 5.58, 2.94)


def _mid(rng, k, d):  # 1 .. 12 (the cell where the float32 oracle is at its worst); rows wider than 64 raise the lower
    return rng.uniform(max(1.0, np.log(d / 24.0)), 12.0, k)  # end so that the sum of phi stays below ~5


def _large(rng, k, d):
    return rng.uniform(15.0, 40.0, k)


def _huge(rng, k, d):
    return rng.uniform(60.0, 85.0, k)


def _one_small(rng, k, d):  # the message is (almost) the small input itself: 2e-3 .. 1, log-uniform
    a = rng.uniform(20.0, 80.0, k)
    a[rng.randint(k)] = np.exp(rng.uniform(np.log(2e-3), 0.0))
    return a


def _few_small(rng, k, d):  # two or three inputs of 0.2 .. 1.5 among large ones
    a = rng.uniform(20.0, 80.0, k)
    few = min(k, int(rng.randint(2, 4)))
    a[rng.choice(k, few, replace=False)] = rng.uniform(0.2, 1.5, few)
    return a


PROFILES = {"hqc": _hqc, "mid": _mid, "large": _large, "huge": _huge, "one_small": _one_small, "few_small": _few_small}
CORNERS = ("one_certain", "all_certain", "zero_source")


class Forest:
    """A star forest and one draw of its priors.
    graph    TannerGraph (m rows, n columns, every column on one edge)
    probs    float64 [n] prior error probabilities (as handed to the decoder)
    deg      int [m] row degrees;  kind [m] profile or corner name of each row ("stuck" for the stuck row)
    probe    int [m] probe column of each row (-1: the stuck row has none)
    sources  list of int arrays: the other columns of each row, in row order
    stuck    row index of the stuck component or None"""

    def __init__(self, graph, deg, kind, probe, sources, stuck):
        self.graph, self.deg, self.kind, self.probe, self.sources, self.stuck = graph, deg, kind, probe, sources, stuck
        self.m, self.n = graph.m, graph.n
        self.rows = np.flatnonzero(probe >= 0)  # rows that carry a probe
        self.band = np.array([band_of(d) for d in deg])
        self.probs = None

    def draw(self, rng, rotate=0, names=None):
        """Priors for every column: row r takes the profile `rotate` places after its own in `names` (the per-codeword
        tests give every codeword another rotation).  Returns (probs float64 [n], kind of every row after the rotation);
        the forest itself is left as it is."""
        names = list(PROFILES) if names is None else list(names)
        p = np.full(self.n, 0.5)
        kinds = []
        for r in range(self.m):
            src, d, kind = self.sources[r], int(self.deg[r]), self.base_kind[r]
            k = len(src)
            if kind == "stuck":
                p[self.graph.col_idx[self.graph.row_ptr[r]]] = 0.0
            elif kind == "all_certain":  # p = 0 and p = 1: +inf and -inf
                p[src] = (rng.rand(k) < 0.3).astype(np.float64)
            else:
                prof = names[(names.index(kind) + rotate) % len(names)] if kind in names else "mid"
                a = PROFILES[prof](rng, k, d)
                # about 30 % negative, only where |x| < 16: p near 1 cannot carry a larger magnitude through float32
                a = np.where((rng.rand(k) < 0.3) & (a < 16.0), -a, a)
                p[src] = 1.0 / (1.0 + np.exp(a))
                if kind == "one_certain":
                    p[src[rng.randint(k)]] = float(rng.rand() < 0.3)
                if kind == "zero_source":
                    p[src[rng.randint(k)]] = 0.5
                if kind in names:
                    kind = prof
            kinds.append(kind)
        return p, np.array(kinds)

    # ---- the key ------------------------------------------------------------------------------------------------
    def truth(self, synd, probs32=None, which=None):
        """float64 [batch, rows with a probe]: the true tanh-rule message of every probe under `synd` (uint8 [batch, m]).
        probs32: float32 [n] priors as the device takes them (default: float32 of self.probs), or [V, n] with
        which [batch]: codeword b carries the priors probs32[which[b]]."""
        return self._key(synd, probs32, which, None)

    def truth_minsum(self, synd, alpha, probs32=None, which=None):
        """float32 [batch, rows with a probe]: min-sum's message, bit for bit (`true_minsum_message`)."""
        return self._key(synd, probs32, which, alpha)

    def _key(self, synd, probs32, which, alpha):
        synd = np.asarray(synd)
        x32 = np.atleast_2d(prior32(self.probs if probs32 is None else probs32))
        which = np.zeros(synd.shape[0], dtype=np.int64) if which is None else np.asarray(which)
        out = np.zeros((synd.shape[0], len(self.rows)), dtype=np.float64 if alpha is None else np.float32)
        for i, r in enumerate(self.rows):
            src = self.sources[r]
            base = np.array([true_message(x[src]) if alpha is None else true_minsum_message(x[src], 0, alpha) for x in x32])
            out[:, i] = np.where(synd[:, r] & 1, -base[which], base[which])
        return out


def star_forest(rng, degrees, profiles=None, rows_per=1, corner_degrees=(2, 3), stuck=False, draw=True):
    """A forest of disjoint stars: for every degree in `degrees` and every profile `rows_per` rows, plus the named corner
    rows (CORNERS) at every degree of `corner_degrees` (degree-2 rows, whose message equals the other input, are ordinary
    rows of degree 2), plus on request the stuck component: a degree-1 row on a p = 0 variable whose syndrome bit the caller
    sets to 1 -- never satisfied, so every codeword of an early-exit run goes on to max_iter; its own variable's posterior
    is inf - inf = NaN (tanh rule) and nothing else is touched.
    Rows come in shuffled order and columns are labelled by a random permutation, so a row's columns are scattered, the
    probe sits at a random position of its (ascending) row and the CSC order is no copy of the CSR order.
    Returns a Forest (with priors drawn unless draw = False)."""
    names = list(PROFILES) if profiles is None else list(profiles)
    spec = [(int(d), nm) for d in degrees for nm in names for _ in range(rows_per)]
    spec += [(int(d), c) for d in corner_degrees for c in CORNERS]
    order = rng.permutation(len(spec))
    spec = [spec[i] for i in order]
    if stuck:
        spec.insert(int(rng.randint(len(spec) + 1)), (1, "stuck"))
    deg = np.array([d for d, _ in spec])
    n = int(deg.sum())
    label = rng.permutation(n)
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col_idx = np.empty(n, dtype=np.int32)
    probe = np.full(len(spec), -1, dtype=np.int64)
    sources = []
    stuck_row = None
    for r, (d, kind) in enumerate(spec):
        cols = np.sort(label[row_ptr[r]:row_ptr[r + 1]])
        col_idx[row_ptr[r]:row_ptr[r + 1]] = cols
        if kind == "stuck":
            stuck_row = r
            sources.append(np.zeros(0, dtype=np.int64))
            continue
        assert d >= 2
        pos = int(rng.randint(d))
        probe[r] = cols[pos]
        sources.append(np.delete(cols, pos).astype(np.int64))
    g = S.TannerGraph.from_csr(len(spec), n, row_ptr, col_idx)
    f = Forest(g, deg, np.array([k for _, k in spec]), probe, sources, stuck_row)
    f.base_kind = [k for _, k in spec]
    f.names = names
    if draw:
        f.probs, f.kind = f.draw(rng, names=names)
    return f


def random_syndromes(rng, forest, batch):
    s = (rng.rand(batch, forest.m) < 0.5).astype(np.uint8)
    if forest.stuck is not None:
        s[:, forest.stuck] = 1
    return s


def errors_in_u(got, truth):
    """|got - truth| / u(truth), elementwise; where the truth is infinite: 0 if got is the same infinity, else inf."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - truth) / unit(truth)
    inf = np.isinf(truth)
    e[inf] = np.where(got[inf] == truth[inf], 0.0, np.inf)
    return e


def worst_per_cell(forest, err, kinds=None, which=None):
    """{(band, kind): worst of err [batch, probe rows]} over the forest's probe rows (a NaN counts as inf).
    kinds [V, m] with which [batch]: codeword b's rows have the kinds kinds[which[b]] (default: the forest's own)."""
    err = np.where(np.isnan(err), np.inf, err)
    kinds = np.atleast_2d(forest.kind if kinds is None else kinds)
    which = np.zeros(err.shape[0], dtype=np.int64) if which is None else np.asarray(which)
    out = {}
    for v in range(kinds.shape[0]):
        if not (which == v).any():
            continue
        worst = err[which == v].max(axis=0)
        for i, r in enumerate(forest.rows):
            key = (int(forest.band[r]), str(kinds[v, r]))
            out[key] = max(out.get(key, 0.0), float(worst[i]))
    return out


# ------------------------------------------------------------------------------------------------ combs
class Comb:
    """Disjoint combs.  hub [K] hub column of each comb; leaves: list of int arrays (leaf columns, in the order of the
    hub's edges, i.e. ascending row); rows: list of int arrays (the two-edge check of each leaf); probs float64 [n]."""

    def __init__(self, graph, hub, leaves, rows, probs):
        self.graph, self.hub, self.leaves, self.rows, self.probs = graph, hub, leaves, rows, probs
        self.m, self.n = graph.m, graph.n


def comb(rng, col_degrees, lo=1.0, hi=12.0):
    """One comb per entry of `col_degrees`: a hub of that degree c (prior a0), each edge to a check of two edges whose
    other end is a leaf (prior x_j).  Magnitudes uniform in [lo, min(hi, 24 / sqrt(c))] (lo >= 1: every term of the signed
    sums is at least one unit u; the upper end shrinks with c so that the hub's outgoing sums, a random walk over the
    syndrome signs, stay clear of the float32 saturation at 87: `max_comb_message` is what a test asserts), about 30 %
    negative.  Rows and column labels are shuffled."""
    hubs, leaf_of = [], []
    n = int(sum(col_degrees)) + len(col_degrees)
    m = int(sum(col_degrees))
    label = rng.permutation(n)
    row_label = rng.permutation(m)
    nxt, row = 0, 0
    pairs = [None] * m
    leaves, rows = [], []
    for c in col_degrees:
        h = int(label[nxt])
        nxt += 1
        rr = np.sort(row_label[row:row + c])  # the hub's edges in ascending row: the order of its column sweep
        row += c
        lv = label[nxt:nxt + c].astype(np.int64)
        nxt += c
        for r, v in zip(rr, lv):
            pairs[int(r)] = sorted((h, int(v)))
        hubs.append(h)
        leaves.append(lv)
        rows.append(rr.astype(np.int64))
    col_idx = np.array([c for p in pairs for c in p], dtype=np.int32)
    g = S.TannerGraph.from_csr(m, n, np.arange(m + 1, dtype=np.int64) * 2, col_idx)
    top = np.empty(n)
    for h, lv, c in zip(hubs, leaves, col_degrees):
        top[h] = top[lv] = max(1.5, min(hi, 24.0 / np.sqrt(c)))
    a = rng.uniform(lo, top)
    a = np.where(rng.rand(n) < 0.3, -a, a)
    return Comb(g, np.array(hubs), leaves, rows, 1.0 / (1.0 + np.exp(a)))


def true_comb_posteriors(cb, synd, alpha=1.0):
    """(post float64 [batch, n], unit float64 [batch, n]): every posterior of the combs from the second iteration on
    -- hub: a0 + sum_j s_j x_j; leaf j: x_j + s_j (a0 + sum_{k != j} s_k x_k), s_j = (-1)^syndrome bit of leaf j's check --
    and its unit u' = 2^-24 * (sum of the |terms|).  alpha: min-sum's scaling (a message through a two-edge check is
    alpha times the other input; the leaf's message is alpha * (a0 + alpha * sum ...)); 1.0 for the tanh rule."""
    x = prior32(cb.probs).astype(np.float64)
    synd = np.asarray(synd)
    post = np.zeros((synd.shape[0], cb.n))
    un = np.zeros((synd.shape[0], cb.n))
    for h, lv, rr in zip(cb.hub, cb.leaves, cb.rows):
        s = 1.0 - 2.0 * (synd[:, rr] & 1)  # [batch, c]
        terms = alpha * s * x[lv][None, :]
        tot = x[h] + terms.sum(axis=1)
        mag = abs(x[h]) + np.abs(terms).sum(axis=1)
        post[:, h], un[:, h] = tot, EPS * mag
        for j, v in enumerate(lv):
            post[:, v] = x[v] + alpha * s[:, j] * (tot - terms[:, j])
            un[:, v] = EPS * (abs(x[v]) + alpha * (mag - np.abs(terms[:, j])))
    return post, un


def max_comb_message(cb, synd):
    """Largest |hub-to-check message| of the combs under `synd`: what passes through the two-edge checks (tanh rule)."""
    post, _ = true_comb_posteriors(cb, synd)
    x = prior32(cb.probs).astype(np.float64)
    return max(float(np.abs(post[:, lv] - x[lv][None, :]).max()) for lv in cb.leaves)


# ------------------------------------------------------------------------------------------------ the cases both files use
# name -> (seed, degrees, rows per (degree, profile)).  The maximum row degree picks the k_check_*<CAP> build (16, 32, 64)
# or, at 200, the any-degree fallbacks; every exact-degree instantiation 2 .. 64 is met.  "lds" is thinned to fit the
# LDS-resident decoder's 60 KB (8 E + 2 n + m + 64 bytes).
FOREST_CASES = {
    "cap16": (1601, list(range(2, 17)), 4),
    "cap32": (1602, list(range(2, 33)), 2),
    "cap64": (1603, list(range(2, 65)), 1),
    "cap200": (1604, [2, 7, 33, 64, 65, 66, 80, 100, 128, 150, 200], 2),
    "lds": (1605, [2, 3, 5, 8, 13, 16, 17, 24, 32, 33, 48, 64, 65, 100], 1),
}
_FORESTS = {}


def forest_case(name, stuck=False):
    """(forest `name`, syndromes uint8 [70, m]: two tiles of codewords, the last ragged).  Built once per process and shared
    by the tests that need it: read-only."""
    key = (name, stuck)
    if key not in _FORESTS:
        seed, degrees, rows_per = FOREST_CASES[name]
        rng = np.random.RandomState(seed)
        f = star_forest(rng, degrees, rows_per=rows_per, corner_degrees=(2, 3, max(degrees)), stuck=stuck)
        _FORESTS[key] = (f, random_syndromes(rng, f, 70))
    return _FORESTS[key]


COMB_CASES = {  # name -> (seed, hub degrees): the maximum picks k_var<16 | 32 | 64> / k_var_rec<16 | 32> / the generic column
    "col16": (1701, [1, 2, 3, 5, 8, 11, 15, 16] * 6),
    "col32": (1702, [1, 2, 7, 16, 17, 20, 25, 31, 32] * 4),
    "col64": (1703, [2, 16, 32, 33, 40, 50, 63, 64] * 3),
    "col100": (1704, [2, 16, 33, 64, 65, 80, 100] * 3),
}
_COMBS = {}


def comb_case(name):
    if name not in _COMBS:
        seed, degs = COMB_CASES[name]
        rng = np.random.RandomState(seed)
        cb = comb(rng, degs)
        _COMBS[name] = (cb, (rng.rand(70, cb.m) < 0.5).astype(np.uint8))
    return _COMBS[name]


_SOFT = {}


def soft_variants(name):
    """Per-codeword priors on the forest `name` (with its stuck row): one draw per profile rotation, codeword b carrying
    draw b % P, so that every row meets every profile within one batch.
    Returns (probs32 float32 [P, n], kinds [P, m], which int [70])."""
    if name not in _SOFT:
        f, _ = forest_case(name, stuck=True)
        rng = np.random.RandomState(FOREST_CASES[name][0] + 500)
        draws = [f.draw(rng, rotate=v, names=f.names) for v in range(len(f.names))]
        _SOFT[name] = (np.stack([d[0] for d in draws]).astype(np.float32), np.stack([d[1] for d in draws]),
                       np.arange(70) % len(f.names))
    return _SOFT[name]
