"""The sparse settle gate (knob `settle_sparse`) restated in NumPy on top of tests/settle_ref.py: which rows and columns of
a tile run in which pass, and the two per-tile tables the device keeps for that decision.

The rule (scaldpc_bp_kernels.h, `Settle`; the passes that write and gate: scaldpc_bp_sched.h, settle_sparse_*):
  check pass t, tracked, for a row that runs: compare the records and the arg-min byte it stores with the ones it overwrites,
      over the tile's real codewords.  A first record differs somewhere -> dirty = all ones (the record's sign bit is the
      row's parity).  Otherwise dirty = OR of bit(old arg) | bit(new arg) over the codewords whose second record or arg byte
      differs (255 = no arg: no bit).  row_flag[row] = (t, dirty).
  variable pass t, tracked, for a column of degree > 1: it runs when some edge j of it has row_flag[row_j] = (t, a mask with
      the bit of the edge's index in that row), or when col_flag[col] == (t - 1) << 1 | 1 -- its own sign masks changed in
      its run before.  A column that runs stores col_flag[col] = t << 1 | (a sign mask it stored differs from the one it
      overwrote, in a real codeword).  Wide columns (minsum_rec = 2: more than 32 edges) are never gated and always stamp
      t << 1.
  check pass t + 1, for a row: it runs when some edge goes into a column with col_flag >> 1 == t.  Columns of degree <= 1
      never stamp.
  A pass gates only when the pass before it on the same tiles wrote flags: check passes first_test + 1 ... last_test,
  variable passes first_test ... last_test - 1 -- or from a later `start` on (variable passes from start, check passes from
  start + 1), which a handle learns from its last call (next_start).  Flags are written by the tracked passes: check passes first_test ...
  last_test, variable passes first_test - 1 ... last_test - 1.

`trace` is settle_ref.run with every pass's state kept (tests/test_settle_sparse.py holds its posteriors to settle_ref's);
`activity` walks the rule over one tile of it.  The full, ungated state is the gated one as long as the rule is
conservative -- a node that is gated out would have stored what is there -- which `violations` counts."""
import functools
import types

import numpy as np

import settle_ref as R

ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
WIDE_FROM = 33  # columns of this many edges or more run in the wide launch under minsum_rec = 2


def check_writes(t, first, last):
    return first <= t <= last


def var_writes(t, first, last):
    return first <= t + 1 <= last


LEAD = 2


def next_start(frozen_at, first):
    """The variable pass from which the call AFTER one with these frozen-at numbers gates (0 = from the first test): LEAD passes
    before the smallest of them, the first test at the earliest; 0 where no tile froze or nothing was learned (None)."""
    at = [f for f in (frozen_at or []) if f > 0]
    return max(min(at) - LEAD, first) if at else 0


def check_gates(t, first, last, start=0):
    return max(first, start) < t <= last


def var_gates(t, first, last, start=0):
    return max(first, start) <= t < last


def trace(g, prior, synd, max_iter, alpha=1.0):
    """settle_ref.run, keeping per iteration it (index 0: before iteration 1) the records r1, r2 (uint32 [B, m]), the arg-min
    index arg (int [B, m]) and the variable-to-check messages x after the variable pass (float32 [B, E], CSR edge order)."""
    prior = np.asarray(prior, dtype=np.float32)
    synd = np.asarray(synd, dtype=np.uint8)
    B, m, n, E = synd.shape[0], g.m, g.n, g.nnz
    row_ptr, col_idx = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    rows, rvalid = R._padded(row_ptr, np.arange(E), m)
    cols, cvalid = R._padded(np.asarray(g.col_ptr), np.asarray(g.csc_edge), n)
    kk = np.arange(rows.shape[1])[None, None, :]
    x = np.broadcast_to(prior[..., col_idx], (B, E)).copy()
    out = types.SimpleNamespace(r1=[None], r2=[None], arg=[None], x=[x.copy()], post=[None], g=g, max_iter=max_iter)
    for it in range(1, max_iter + 1):
        a = R.alpha_for(alpha, it)
        X = np.where(rvalid[None], x[:, np.where(rvalid, rows, 0)], np.float32(np.inf))
        neg = X <= 0
        ax = np.minimum(np.abs(X), R.FLT_MAX)
        srt = np.sort(ax, axis=2)
        m1 = srt[:, :, 0]
        m2 = srt[:, :, 1] if srt.shape[2] > 1 else np.full_like(m1, R.FLT_MAX)
        odd = (synd.astype(bool)) ^ ((neg.sum(axis=2) & 1).astype(bool))
        eq = np.abs(X) == m1[:, :, None]
        arg = np.where(eq.any(axis=2), eq.argmax(axis=2), R.NO_ARG)
        r1, r2 = m1 * a, m2 * a
        r1, r2 = np.where(odd, -r1, r1), np.where(odd, -r2, r2)
        out.r1.append(r1.view(np.uint32).copy())
        out.r2.append(r2.view(np.uint32).copy())
        out.arg.append(arg.copy())
        mag = np.where(kk == arg[:, :, None], r2[:, :, None], r1[:, :, None]).astype(np.float32)
        c2v_rows = (mag.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(np.float32)
        c2v = np.zeros((B, E), dtype=np.float32)
        c2v[:, rows[rvalid]] = c2v_rows[:, rvalid]
        C = c2v[:, np.where(cvalid, cols, 0)]
        dc = cols.shape[1]
        temp = np.broadcast_to(prior, (B, n)).copy()
        pp = []
        for k in range(dc):
            pp.append(temp)
            temp = np.where(cvalid[None, :, k], temp + C[:, :, k], temp)
        out.post.append(temp)
        suf = np.zeros((B, n), dtype=np.float32)
        for k in range(dc - 1, -1, -1):
            v = cvalid[:, k]
            x[:, cols[v, k]] = (pp[k] + suf)[:, v]
            suf = np.where(v[None], suf + C[:, :, k], suf)
        out.x.append(x.copy())
    return out


def _bits(idx):
    """OR of 1 << i over the entries of idx below 64 (255 = no arg: no bit), as uint64."""
    out = np.uint64(0)
    for i in np.unique(idx):
        if i < 64:
            out |= np.uint64(1) << np.uint64(int(i))
    return out


def activity(tr, tile, batch, first, last=None, wide=False, sparse=True, own_rule=True, start=0):
    """The rule on tile `tile` (codewords 64 * tile ... of the first `batch`) of a trace, tests first ... last (last = the
    trace's max_iter by default: a call without a horizon, or a tile decoded again).  Returns a namespace:
    row_runs / col_runs  dict pass -> bool [m] / [n]: the node runs (every pass from 2 on that the call enqueues before its
                         closing pass; columns of degree <= 1 are False: the slim passes leave them out)
    row_stamp, row_dirty, col_flag  the tables as the device holds them after the call
    frozen_at            the tile's frozen-at number (settle_ref.frozen_at's)
    sparse = False: nothing gates (every node of a tile that is not frozen runs); the tables are still written.
    start: the variable pass from which the call gates (check passes one later; 0 = the first test).
    own_rule = False: the WRONG rule in which a column does not look at its own sign_changed bit (what the tests show caught)."""
    g = tr.g
    last = tr.max_iter if last is None else last
    lanes = slice(64 * tile, min(64 * tile + 64, batch))
    m, n = g.m, g.n
    row_ptr, col_idx = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    col_ptr, csc_edge = np.asarray(g.col_ptr), np.asarray(g.csc_edge)
    cdeg = np.diff(col_ptr)
    edge_row = np.repeat(np.arange(m), np.diff(row_ptr))
    edge_idx = np.arange(g.nnz) - row_ptr[edge_row]
    row_stamp, row_dirty = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64)
    col_flag = np.zeros(n, dtype=np.uint32)
    row_runs, col_runs = {}, {}
    latest = 0  # the maximum of the tile's settle words
    for it in range(2, last + 1):
        # ---- check pass it ------------------------------------------------------------------------------------------
        done = it - 1 if it - 1 >= first else 0
        runs = np.diff(row_ptr) > 0
        if latest < done:
            runs = np.zeros(m, dtype=bool)  # the tile is frozen
        elif sparse and check_gates(it, first, last, start):
            hot = (cdeg[col_idx] > 1) & ((col_flag[col_idx] >> 1) == it - 1)
            runs = np.zeros(m, dtype=bool)
            np.logical_or.at(runs, edge_row, hot)
        row_runs[it] = runs
        if check_writes(it, first, last):
            d1 = tr.r1[it][lanes] != tr.r1[it - 1][lanes]
            d2 = (tr.r2[it][lanes] != tr.r2[it - 1][lanes]) | (tr.arg[it][lanes] != tr.arg[it - 1][lanes])
            for r in np.nonzero(runs)[0]:
                if d1[:, r].any():
                    dirty = ALL
                else:
                    w = d2[:, r]
                    dirty = _bits(tr.arg[it - 1][lanes][w, r]) | _bits(tr.arg[it][lanes][w, r])
                row_stamp[r], row_dirty[r] = it, dirty
                if d1[:, r].any() or d2[:, r].any():
                    latest = max(latest, it)
        # ---- variable pass it (pass `last` is the closing pass, or is not enqueued: neither gates nor writes) ----------
        if it == last:
            break
        done = it if first <= it <= last else 0
        runs = cdeg > 1
        if latest < done:
            runs = np.zeros(n, dtype=bool)
        elif sparse and var_gates(it, first, last, start):
            hit = (row_stamp[edge_row] == it) & (((row_dirty[edge_row] >> edge_idx.astype(np.uint64)) & np.uint64(1)) != 0)
            by_col = np.zeros(n, dtype=bool)
            np.logical_or.at(by_col, col_idx, hit)
            own = col_flag == np.uint32(((it - 1) << 1) | 1)
            gated = by_col | own if own_rule else by_col
            if wide:
                gated |= cdeg >= WIDE_FROM
            runs = runs & gated
        col_runs[it] = runs
        if var_writes(it, first, last):
            sg = (tr.x[it][lanes] <= 0) != (tr.x[it - 1][lanes] <= 0)  # [lanes, E]
            ch = np.zeros(n, dtype=bool)
            np.logical_or.at(ch, col_idx, sg.any(axis=0))
            col_flag[runs] = (np.uint32(it << 1) | ch[runs].astype(np.uint32))
            if wide:  # (a wide column's bit is never read -- it is never gated -- and stays 0)
                col_flag[runs & (cdeg >= WIDE_FROM)] = np.uint32(it << 1)
            if (ch & runs).any():
                latest = max(latest, it + 1)
    if last < first or latest >= last:
        frozen_at = 0
    else:
        frozen_at = max(latest + 1, first)
    return types.SimpleNamespace(row_runs=row_runs, col_runs=col_runs, row_stamp=row_stamp, row_dirty=row_dirty,
                                 col_flag=col_flag, frozen_at=frozen_at)


def violations(tr, act, tile, batch):
    """Conservative?  Counts the gated-out nodes whose output differs from the pass before in a codeword of the tile: rows
    by their two records and arg-min index, columns (degree > 1) by every outgoing message, bit for bit, and their
    posterior.  Passes in which the whole tile is frozen count too: nothing may differ there either."""
    g = tr.g
    lanes = slice(64 * tile, min(64 * tile + 64, batch))
    col_idx = np.asarray(g.col_idx)
    cdeg = np.diff(np.asarray(g.col_ptr))
    bad = 0
    for it, runs in act.row_runs.items():
        diff = ((tr.r1[it][lanes] != tr.r1[it - 1][lanes]) | (tr.r2[it][lanes] != tr.r2[it - 1][lanes]) |
                (tr.arg[it][lanes] != tr.arg[it - 1][lanes])).any(axis=0)
        bad += int((diff & ~runs).sum())
    for it, runs in act.col_runs.items():
        de = (tr.x[it][lanes].view(np.uint32) != tr.x[it - 1][lanes].view(np.uint32)).any(axis=0)
        diff = np.zeros(g.n, dtype=bool)
        np.logical_or.at(diff, col_idx, de)
        diff |= (tr.post[it][lanes].view(np.uint32) != tr.post[it - 1][lanes].view(np.uint32)).any(axis=0)
        bad += int((diff & ~runs & (cdeg > 1)).sum())
    return bad


@functools.lru_cache(maxsize=None)
def traced(name):
    """The trace of a settle_ref.case (computed once, never changed)."""
    c = R.case(name)
    return trace(c.H, R.prior_llr(c.probs), c.synd, R.MAX_ITER, c.alpha)


OWN_N, OWN_P, OWN_BATCH = 60, 0.08, 65


@functools.lru_cache(maxsize=None)
def own_case():
    """An input on which a column must run through its own sign_changed bit ALONE: the (3,6)-regular graph on 60 columns,
    every prior one float (messages are small multiples of it, so a sign flips at an unchanged magnitude), 65 codewords of
    which the last sits alone in tile 1.  There two sign flips in one row cancel in the record's parity bit while the first
    record keeps its bits and neither edge is an arg-min: the row marks nothing, and only the column's own bit brings it
    back.  With 64 codewords in the tile some other codeword marks the edge; alone, nothing else does.  Nothing freezes on
    this graph, and it is no [Hin | I]: a handle tracks it under settle = 2 given."""
    rng = np.random.RandomState(0)
    H = R.S.codes.make_regular_ldpc_graph(OWN_N, OWN_N // 2, 3, 6, rng)
    err = (rng.rand(64, OWN_N) < OWN_P).astype(np.uint8)
    synd = H.syndrome(err).astype(np.uint8)
    synd = np.ascontiguousarray(np.concatenate([synd, synd[:1]]))  # (codeword 0 again, alone in tile 1)
    probs = np.full(OWN_N, OWN_P)
    return types.SimpleNamespace(H=H, probs=probs, synd=synd, alpha=1.0, first=3, tr=trace(H, R.prior_llr(probs), synd, R.MAX_ITER, 1.0))
