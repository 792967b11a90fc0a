"""TEST INFRASTRUCTURE: the trial law of scaldpc_mc_qary_run_secret (include/scaldpc.h) restated in NumPy, on the Philox words of
oracle/mc_oracle.c (stream 1: the secret, stream 0: the outcomes -- the words of tests/qary_mc_ref.py), and the tables the CPU
and GPU tests of the entry share."""
import numpy as np

import qary_mc_ref as mc
from oracle import pyoracle


def words(seed, first, batch, n, stream=0):
    """Word x of `stream` of trial first + b, [batch, n]: counter (x >> 2, stream, trial_lo, trial_hi), key (seed_lo, seed_hi)."""
    if stream == 0:
        return mc.words(seed, first, batch, n)
    out = np.zeros((batch, (n + 3) // 4 * 4), dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for b in range(batch):
        t = first + b
        for blk in range((n + 3) // 4):
            out[b, 4 * blk : 4 * blk + 4] = pyoracle.philox4x32_10((blk, stream, t & 0xFFFFFFFF, t >> 32), key)
    return out[:, :n]


def conditional_levels(w, true_index, weights):
    """Per element the smallest k with word < T^s_k, s the element's true symbol index; weights [Q, K], every row through
    the threshold rule on its own."""
    T = np.array([mc.thresholds(row) for row in np.asarray(weights, dtype=np.float64)], dtype=np.uint64)  # [Q, K]
    return (w[..., None] < T[true_index]).argmax(axis=-1).astype(np.uint8)


def row_sums(H, coeffs):
    """t_r = -h_{r,id} * sum_j h_{r,j} s_j for H = [H' | +-I]: int64 [batch, R]."""
    H = np.asarray(H, dtype=np.int64)
    R, N = H.shape
    ident = H[np.arange(R), N - R + np.arange(R)]
    assert (np.abs(ident) == 1).all()
    return -ident * (coeffs.astype(np.int64) @ H[:, : N - R].T)


def draw(H, B, BSUM, seed, first, batch, prior, weights_b, weights_s):
    """(secret int8 [batch, N], levels uint8 [batch, N]) of trials first .. first + batch - 1."""
    R, N = np.asarray(H).shape
    BV = N - R
    s_idx = mc.levels_of(words(seed, first, batch, BV, stream=1), prior).astype(np.int64)  # the prior's thresholds: the same rule
    t = row_sums(H, s_idx - B)
    assert (np.abs(t) <= BSUM).all()
    w = words(seed, first, batch, N)
    lv = np.concatenate([conditional_levels(w[:, :BV], s_idx, weights_b), conditional_levels(w[:, BV:], t + BSUM, weights_s)], axis=1)
    return np.concatenate([s_idx - B, t], axis=1).astype(np.int8), lv


def best_symbols(levels, B):
    """The value a variable decides from a float32 pmf row alone: the first maximum (decoder.rs:668-704), [K]."""
    return np.asarray(levels, dtype=np.float32).argmax(axis=1) - B


def results(secret, levels, symbols, BV, levels_b, levels_s, B, BSUM):
    """success, wrong [batch, 2] and channel_wrong [batch, 2] as secret, levels and symbols define them."""
    best = np.concatenate([best_symbols(levels_b, B)[levels[:, :BV]], best_symbols(levels_s, BSUM)[levels[:, BV:]]], axis=1)
    wrong = np.stack([(symbols[:, :BV] != secret[:, :BV]).sum(axis=1), (symbols[:, BV:] != secret[:, BV:]).sum(axis=1)], axis=1)
    chan = np.stack([(best[:, :BV] != secret[:, :BV]).sum(axis=1), (best[:, BV:] != secret[:, BV:]).sum(axis=1)], axis=1)
    return dict(success=(wrong[:, 0] == 0).astype(np.uint8), wrong=wrong.astype(np.int32), channel_wrong=chan.astype(np.int32))


# ---------------------------------------------------------------------------------------------------- codings of the project's own
def expansion(symbols, bits):
    """The `bits`-bit binary expansion of the symbol index, most significant bit first."""
    assert symbols <= 1 << bits
    return [tuple((s >> (bits - 1 - i)) & 1 for i in range(bits)) for s in range(symbols)]


PARITY_5 = [(s & 1,) for s in range(5)]  # one oracle bit: the parity of the index
SHARED_5 = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 0)]  # two bits; the values -2 and +2 share a code word
