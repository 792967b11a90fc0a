"""TEST INFRASTRUCTURE: the trial law of scaldpc_mc_qary_run (include/scaldpc.h) restated in NumPy, on the Philox words of
oracle/mc_oracle.c, and the fixtures the CPU and GPU tests of the q-ary Monte-Carlo entry share."""
import numpy as np

from oracle import pyoracle

TWO32 = 1 << 32


def thr(p):
    """oracle/mc_oracle.c:42: floor(p 2^32), 0 for p <= 0, 2^32 for p >= 1."""
    return TWO32 if p >= 1.0 else 0 if p <= 0.0 else int(np.float64(p) * np.float64(4294967296.0))


def thresholds(weights):
    """T_k = thr(w_0 + ... + w_k), summed left to right in float64; 2^32 from the last level of nonzero weight on."""
    w = np.asarray(weights, dtype=np.float64)
    acc, T = np.float64(0.0), []
    for x in w:
        acc = acc + x
        T.append(thr(acc))
    last = int(np.flatnonzero(w > 0)[-1])
    return [TWO32 if k >= last else t for k, t in enumerate(T)]


def words(seed, first, batch, n):
    """Stream-0 word x of trial first + b, [batch, n]: counter (x >> 2, 0, trial_lo, trial_hi), key (seed_lo, seed_hi)."""
    out = np.zeros((batch, (n + 3) // 4 * 4), dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for b in range(batch):
        t = first + b
        for blk in range((n + 3) // 4):
            out[b, 4 * blk : 4 * blk + 4] = pyoracle.philox4x32_10((blk, 0, t & 0xFFFFFFFF, t >> 32), key)
    return out[:, :n]


def levels_of(w, weights):
    """The smallest k with word < T_k."""
    T = np.array(thresholds(weights), dtype=np.uint64)
    return (w[..., None] < T).argmax(axis=-1).astype(np.uint8)


def draw(seed, first, batch, n, weights, n_sum=0, weights_sum=None):
    """Levels [batch, n + n_sum]: the first n variables from `weights`, the others (DecoderSpecial's row sums) from `weights_sum`."""
    w = words(seed, first, batch, n + n_sum)
    lv = levels_of(w[:, :n], weights)
    return lv if not n_sum else np.concatenate([lv, levels_of(w[:, n:], weights_sum)], axis=1)


def reference_rows(B=1):
    """decode.py:232-237: (bad, good) as float32 -- the last level is the good row."""
    BB = 2 * B + 1
    p = 1 / BB
    good, bad = np.full(BB, p), np.full(BB, p)
    good[[B, -1]] = [1.75 * p, 0.25 * p]
    bad[[-1, B]] = [1.75 * p, 0.25 * p]
    return np.stack([bad, good]).astype(np.float32)
