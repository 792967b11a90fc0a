"""NumPy float32 restatement of both q-ary decoders' WHOLE loop that keeps what the decoders throw away: the per-symbol
totals of the last variable update (helper of tests/test_qary_soft*.py; not collected).

  init                      decoder.rs:567-573 / decoder_special.rs:480-493     v2c = channel * h
  per iteration  checks     decoder.rs:585-631 / decoder_special.rs:506-563     generic_check_enumerated / special_check_enumerated
                                                                                (tests/test_min_marginal_identity.py: the reference form)
                 variables  decoder.rs:634-658 / decoder_special.rs:566-609     channel + incoming messages in column order, minus
                                                                                self, normalised by the first minimum
  last pass                 the totals `sum[q]`, their first-minimum arg-min (the symbol), the margin and the unmet checks

Every addition and subtraction is a float32 operation in the reference's order, so the totals are the bit patterns the
decoders hold before they take the arg-min.  LLRs come from oracle.pyoracle.qary_into_llr (the host's logf).

  cost    float32 [rows]    row of variable v, symbol q (value q - B_v) at var_off[v] + q
  margin  fl(m2 - m1): m1 the total at the decided symbol, m2 the smallest total over the OTHER symbols by the reference's
          scan rule (strict <, NaN never selected, +inf if there is no candidate)
  unmet   number of checks whose integer sum of h_e * x_e over the row's edges is nonzero (decoder.rs:336-337)
"""
import numpy as np

from test_min_marginal_identity import generic_check_enumerated, special_check_enumerated

F = np.float32
_CHECK_MEMO = {}  # generic_check_enumerated is a pure function of (a, B): measured channel outputs repeat a handful of rows


def _generic_check(a, B):
    key = (a.shape, int(B), a.tobytes())
    if key not in _CHECK_MEMO:
        if len(_CHECK_MEMO) > 200000:
            _CHECK_MEMO.clear()
        _CHECK_MEMO[key] = generic_check_enumerated(a, B)
    return _CHECK_MEMO[key]


def first_min(row):
    """decoder.rs:694-704: index of the first strict minimum, NaN never selected, default 0."""
    mv, ma = F(np.inf), 0
    for q, x in enumerate(row):
        if x < mv:
            mv, ma = x, q
    return ma


def margin_of(row, ma=None):
    """fl(m2 - m1) of one row of totals (module docstring)."""
    row = np.asarray(row, dtype=F)
    if ma is None:
        ma = first_min(row)
    m2 = F(np.inf)
    for q, x in enumerate(row):
        if q != ma and x < m2:
            m2 = x
    with np.errstate(invalid="ignore"):
        return F(m2 - row[ma])


def unmet_checks(H, symbols):
    """Checks of H (dense, entries in {-1, 0, 1}) whose signed sum over the integers is nonzero; symbols int [..., N]."""
    s = np.asarray(symbols, dtype=np.int64) @ np.asarray(H, dtype=np.int64).T
    return (s != 0).sum(axis=-1).astype(np.int32)


def _decode_one(H, llr_rows, alph, iterations, special_B=None, special_BSUM=None):
    """llr_rows: list of N float32 arrays (variable v's channel LLRs); alph[v] = B_v.  Returns (sums list, symbols)."""
    H = np.asarray(H)
    R, N = H.shape
    rows = [np.flatnonzero(H[r]) for r in range(R)]  # a check's edges in ascending column (decoder.rs:507-539)
    cols = [np.flatnonzero(H[:, v]) for v in range(N)]  # a variable's edges in ascending row
    v2c, c2v = {}, {}
    for v in range(N):
        for r in cols[v]:
            v2c[r, v] = llr_rows[v][::-1].copy() if H[r, v] < 0 else llr_rows[v].copy()
    sums = None
    for _ in range(max(1, iterations)):  # the loop body runs at least once (decoder.rs:578-579)
        for r in range(R):
            vs = rows[r]
            if special_B is None:
                beta, conf = _generic_check(np.stack([v2c[r, v] for v in vs]), alph[vs[0]])
                if not conf:
                    raise RuntimeError("a check node admits no finite configuration (decoder.rs:618)")
                for j, v in enumerate(vs):
                    c2v[r, v] = beta[j]
            else:
                beta, beta_s = special_check_enumerated(np.stack([v2c[r, v] for v in vs[:-1]]), v2c[r, vs[-1]], special_B, special_BSUM)
                for j, v in enumerate(vs[:-1]):
                    c2v[r, v] = beta[j]
                c2v[r, vs[-1]] = beta_s
        sums = []
        with np.errstate(invalid="ignore", over="ignore"):
            for v in range(N):
                s = llr_rows[v].copy()
                for r in cols[v]:
                    s = (s + (c2v[r, v][::-1] if H[r, v] < 0 else c2v[r, v])).astype(F)
                for r in cols[v]:
                    if H[r, v] > 0:
                        tmp = (s - c2v[r, v]).astype(F)
                    else:  # (sum - rev(in)), reversed again
                        tmp = (s - c2v[r, v][::-1]).astype(F)[::-1]
                    v2c[r, v] = (tmp - tmp[first_min(tmp)]).astype(F)
                sums.append(s)
    symbols = np.array([first_min(s) - alph[v] for v, s in enumerate(sums)], dtype=np.int8)
    return sums, symbols


def _pack(H, sums, symbols):
    return {
        "symbols": symbols,
        "cost": np.concatenate(sums).astype(F),
        "margin": np.array([margin_of(s) for s in sums], dtype=F),
        "unmet": unmet_checks(H, symbols),
    }


def _stack(per_cw):
    return {k: np.stack([d[k] for d in per_cw]) for k in per_cw[0]}


def min_sum_soft(oracle, H, B, pmf, iterations):
    """Decoder::min_sum with its last totals.  pmf float32 [batch, N, Q] ->
    dict(symbols int8 [batch, N], costs float32 [batch, N, Q], margins float32 [batch, N], unmet int32 [batch])."""
    H = np.asarray(H)
    N, Q = H.shape[1], 2 * B + 1
    pmf = np.ascontiguousarray(pmf, dtype=F)
    out = []
    for p in pmf:
        with np.errstate(divide="ignore"):
            llr = oracle.qary_into_llr(p)
        out.append(_pack(H, *_decode_one(H, [llr[v] for v in range(N)], [B] * N, iterations)))
    r = _stack(out)
    return {"symbols": r["symbols"], "costs": r["cost"].reshape(len(pmf), N, Q), "margins": r["margin"], "unmet": r["unmet"]}


def special_min_sum_soft(oracle, H, B, BSUM, pmf_b, pmf_s, iterations):
    """DecoderSpecial::min_sum with its last totals: costs [batch, N-R, 2B+1] and costs_sum [batch, R, 2BSUM+1]."""
    H = np.asarray(H)
    R, N = H.shape
    BV, QB, QS = N - R, 2 * B + 1, 2 * BSUM + 1
    pmf_b, pmf_s = np.ascontiguousarray(pmf_b, dtype=F), np.ascontiguousarray(pmf_s, dtype=F)
    out = []
    for pb, ps in zip(pmf_b, pmf_s):
        with np.errstate(divide="ignore"):
            lb, ls = oracle.qary_into_llr(pb), oracle.qary_into_llr(ps)
        rows = [lb[v] for v in range(BV)] + [ls[r] for r in range(R)]
        out.append(_pack(H, *_decode_one(H, rows, [B] * BV + [BSUM] * R, iterations, B, BSUM)))
    r = _stack(out)
    nb = len(pmf_b)
    return {"symbols": r["symbols"], "costs": r["cost"][:, : BV * QB].reshape(nb, BV, QB),
            "costs_sum": r["cost"][:, BV * QB:].reshape(nb, R, QS), "margins": r["margin"], "unmet": r["unmet"]}


def same_bits(a, b):
    """Float arrays equal as bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ------------------------------------------------------------------------------------------------ shared cases (graphs with cycles)
def q15_instance(batch):
    """The reference's 6 x 3, Q = 15 unit-test decoder (decoder.rs:771-799): its own channel output first, then random
    ones with five possible symbols per variable (the others have probability 0: +inf costs, short enumerations)."""
    H = np.array([[1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1], [1, 0, 0, 1, 1, 0]], dtype=np.int8)
    rng = np.random.RandomState(15)
    pmf = np.zeros((batch, 6, 15), dtype=F)
    pmf[0, :, 7] = 1.0
    pmf[0, 1, 7], pmf[0, 1, 14] = 0.1, 0.9
    for b in range(1, batch):
        for v in range(6):
            keep = np.sort(rng.choice(np.arange(4, 11), 5, replace=False))
            pmf[b, v, keep] = rng.dirichlet(np.ones(5) * 1.5)
    return H, 7, pmf


def cyclic_instance(B, batch, seed, R=6, N=12, signed=True):
    """A small graph WITH cycles (rows of 3 - 4 edges, columns of up to 3; one variable may sit in no check), +-1 entries."""
    rng = np.random.RandomState(seed)
    while True:
        H = np.zeros((R, N), dtype=np.int8)
        for r in range(R):
            k = 3 + r % 2
            H[r, rng.choice(N, k, replace=False)] = rng.choice([-1, 1], size=k) if signed else 1
        if np.abs(H).sum(axis=0).max() <= 3:
            break
    pmf = rng.dirichlet(np.ones(2 * B + 1) * 1.2, size=(batch, N)).astype(F)
    pmf[1::4, ::5, 0] = 0.0  # zero-probability symbols on some codewords
    pmf = (pmf / pmf.sum(axis=2, keepdims=True)).astype(F)
    return H, B, pmf
