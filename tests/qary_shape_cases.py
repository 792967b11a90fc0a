"""The graphs, inputs and answer keys of tests/test_qary_shapes_gpu.py (helper; not collected): one small case per branch of the
q-ary launch plan (csrc/scaldpc_qary_plan.h) that the other parity tests do not reach -- alphabets outside 3 / 5 / 7 / 15, lane
kernels with fewer than 64 codewords per block, the untiled conversion, digit words full to the last byte, columns of more than
four checks, DecoderSpecial with B >= 4.  tests/test_qary_plan.py holds every case to the branch it is named for on the CPU.

One generator, seeded RandomState: H has the given row degrees, entries +-1 on distinct random columns; pmfs are dirichlet(0.8)
rows in float32; where keep < Q all but `keep` symbols of a row (chosen per codeword and variable, the zero symbol always among
the kept ones, so every check has the all-zero configuration) are set to 0 and the row is renormalised.  3 iterations.

The key is the C restatement (oracle/qary_oracle.c): symbols and the last variable pass's totals, held bit for bit to the slow
NumPy restatement by tests/test_qary_soft.py; margins and unmet checks follow from them by tests/qary_soft_ref.py's rules."""
import functools
import zlib

import numpy as np

import qary_soft_ref as ref
from helpers import S

F = np.float32
ITERATIONS = 3
BATCH = 130  # three 64-blocks, ragged against every block size but 32 (whose raggedness comes from batches 31 and 33)
BIG = 300    # beyond 256: the plain decoder's automatic switch from the wave to the lane kernel
LDS = 64 * 1024

WAVE, LANE = dict(wave=1), dict(wave=0)
# name -> Q, row degrees, N, keep (None: every symbol), forced columns {column: number of checks}, block size T of the lane kernel,
# the forms to run as (knobs, check kernel), the conversion and the variable form the plan takes
PLAIN = {
    "q9": dict(Q=9, rows=(6, 5, 6, 3), N=24, keep=5, T=64, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="generic"),
    "q15_dc8": dict(Q=15, rows=(8, 8, 7, 5, 2, 1), N=40, keep=4, T=32, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="small"),
    "q15_dc8_dv5": dict(Q=15, rows=(8, 8, 7, 5, 2, 1), N=40, keep=4, T=32, cols={0: 5}, forms=((WAVE, "k_q_check_wave"),), llr="fused_each", var="generic"),
    "q31": dict(Q=31, rows=(4, 4, 3, 2, 1), N=16, keep=None, T=32, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="generic"),
    "q33": dict(Q=33, rows=(4, 4, 3, 2), N=16, keep=None, T=32, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="unfused", var="generic"),
    "q63": dict(Q=63, rows=(4, 3, 3), N=12, keep=40, T=16, forms=((dict(), "k_q_check"), (WAVE, "k_q_check")), llr="unfused", var="generic"),
    "q63_wave": dict(Q=63, rows=(3, 3, 2), N=12, keep=40, T=32, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="unfused", var="generic"),
    "q83": dict(Q=83, rows=(3, 3, 2, 1), N=10, keep=None, T=16, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="unfused", var="generic"),
    "q129": dict(Q=129, rows=(3, 2, 3), N=8, keep=None, T=16, forms=((dict(), "k_q_check"),), llr="unfused", var="generic"),
    "q255": dict(Q=255, rows=(3, 3, 2), N=8, keep=None, T=8, forms=((dict(), "k_q_check"),), llr="unfused", var="generic"),
    "q3_dc8": dict(Q=3, rows=(8, 7, 3, 8), N=24, keep=None, T=64, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="small"),
    "q5_dc8": dict(Q=5, rows=(8, 6, 7, 2), N=24, keep=3, T=64, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="small"),
    "q7_dc6": dict(Q=7, rows=(6, 6, 5, 1), N=24, keep=None, T=64, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")), llr="fused_each", var="small"),
    "q3_dc16": dict(Q=3, rows=(16, 13, 9, 8, 2), N=40, keep=2, T=64, forms=((dict(), "k_q_check"),), llr="fused_each", var="small"),
    "dv9_q3": dict(Q=3, rows=(7,) * 10, N=30, keep=None, T=64, cols={0: 9, 1: 5},
                   forms=((dict(), "k_q_check_dp<3,7>"), (dict(unroll=0), "k_q_check_wave")), llr="fused_each", var="generic"),
    "dv9_q15": dict(Q=15, rows=(7,) * 10, N=30, keep=4, T=64, cols={0: 9, 1: 5}, forms=((WAVE, "k_q_check_wave"), (LANE, "k_q_check")),
                    llr="fused_each", var="generic"),
}  # fmt: skip
# DecoderN{N}R{R}SW{SW}B{B}: H = [H' | I], rows of SW coefficient edges, every third row one edge shorter; 9/10 of the row-sum
# alphabet finite.  name -> SW, B, T, forms, conversion
DP_ANY = dict(dp_any=1)
SPECIAL = {
    "SW3B7": dict(SW=3, B=7, T=64, forms=((WAVE, "k_q_special_check_wave"), (LANE, "k_q_special_check")), llr="unfused"),  # 15 / 43: tiled + plain, k_q_init
    "SW2B7": dict(SW=2, B=7, T=64, forms=((WAVE, "k_q_special_check_wave"), (LANE, "k_q_special_check")), llr="fused_both"),  # 15 / 29: VT 2 and 1
    "SW7B1": dict(SW=7, B=1, T=64, forms=((dict(dp_any=0), "k_q_special_check_wave"), (LANE, "k_q_special_check"), (DP_ANY, "k_q_special_check_dp_any")),
                  llr="fused_both"),  # 3 / 15, rows of 8 edges
    "SW4B4": dict(SW=4, B=4, T=64, forms=((WAVE, "k_q_special_check_wave"), (LANE, "k_q_special_check")), llr="unfused"),  # 9 / 33
    "SW5B3": dict(SW=5, B=3, T=64, forms=((WAVE, "k_q_special_check_wave"), (LANE, "k_q_special_check"), (DP_ANY, "k_q_special_check_dp_any")),
                  llr="fused_both"),  # 7 / 31
    "SW2B63": dict(SW=2, B=63, T=16, forms=((dict(), "k_q_special_check"),), llr="unfused"),  # 127 / 253: var_T = 32
}  # fmt: skip
SPECIAL_R, SPECIAL_BV = 6, 14
# the case of each family that also runs batch 300 with default knobs, the reversed batch and the device-pointer call
FAMILY = {"q9": ("k_q_check_wave", "k_q_check"), "SW4B4": ("k_q_special_check_wave", "k_q_special_check_wave")}  # kernel at 130, at 300


def block_size(per_codeword_bytes):
    """Threads (= codewords) per block of an LDS-staged kernel: as many (<= 64, >= 8) as fit 64 KB (include/scaldpc.h)."""
    T = 64
    while T > 8 and per_codeword_bytes * T > LDS:
        T //= 2
    return T


def batches(T):
    return (1, T - 1, T + 1, BATCH)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def make_H(rng, rows, N, cols=None):
    """Row r has rows[r] entries +-1 on distinct random columns; cols = {column: k} puts that column into exactly k rows (the first
    k that are long enough), the rest of every row lands on the other columns."""
    cols = cols or {}
    H = np.zeros((len(rows), N), dtype=np.int8)
    free = np.array([c for c in range(N) if c not in cols])
    taken = np.zeros(len(rows), dtype=int)
    for c, k in cols.items():
        H[:k, c] = 1
        taken[:k] += 1
    for r, k in enumerate(rows):
        H[r, rng.choice(free, k - taken[r], replace=False)] = 1
    H *= rng.choice(np.array([-1, 1], dtype=np.int8), size=H.shape)
    assert tuple(np.abs(H).sum(axis=1)) == tuple(rows)
    return H


def make_pmf(rng, batch, nv, Q, keep):
    pmf = rng.dirichlet(np.full(Q, 0.8), size=(batch, nv)).astype(F)
    if keep is not None and keep < Q:
        zero = (Q - 1) // 2
        score = rng.rand(batch, nv, Q)
        score[..., zero] = -1.0  # the zero symbol is always kept
        drop = np.argsort(score, axis=2)[..., keep:]
        np.put_along_axis(pmf, drop, 0.0, axis=2)
        pmf = (pmf / pmf.sum(axis=2, keepdims=True, dtype=F)).astype(F)
    assert (pmf[..., (Q - 1) // 2] > 0).all()
    return pmf


def _soft(H, symbols, tables, alphabets):
    """margins and unmet checks out of totals and symbols, by tests/qary_soft_ref.py's rules; tables[i]: [batch, nv_i, Q_i]."""
    margins = []
    v0 = 0
    for tab, Bv in zip(tables, alphabets):
        m = np.empty(tab.shape[:2], dtype=F)
        for b in range(tab.shape[0]):
            for v in range(tab.shape[1]):
                m[b, v] = ref.margin_of(tab[b, v], int(symbols[b, v0 + v]) + Bv)
        margins.append(m)
        v0 += tab.shape[1]
    return np.concatenate(margins, axis=1), ref.unmet_checks(H, symbols)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def plain_graph(name):
    c = PLAIN[name]
    return make_H(_rng(name), c["rows"], c["N"], c.get("cols"))


def special_graph(name):
    c = SPECIAL[name]
    rows = tuple(c["SW"] - (1 if r % 3 == 2 else 0) for r in range(SPECIAL_R))
    return np.concatenate([make_H(_rng(name), rows, SPECIAL_BV), np.eye(SPECIAL_R, dtype=np.int8)], axis=1)


def shape_of(name):
    """What qary_build works out of the case's H: the plan's input (tests/test_qary_plan.py)."""
    if name in PLAIN:
        H, Q = plain_graph(name), PLAIN[name]["Q"]
        QS, special = Q, 0
    else:
        H, Q = special_graph(name), 2 * SPECIAL[name]["B"] + 1
        QS, special = 2 * SPECIAL[name]["SW"] * SPECIAL[name]["B"] + 1, 1
    dc, dv = np.abs(H).sum(axis=1), np.abs(H).sum(axis=0)
    return dict(special=special, R=H.shape[0], N=H.shape[1], E=int(dc.sum()), Q=Q, QS=QS, W=max(Q, QS), maxdc=int(dc.max()),
                mindc=int(dc.min()), maxdv=int(dv.max()))


@functools.lru_cache(maxsize=None)
def plain_case(name, batch=BATCH):
    """dict(H, B, pmf [batch, N, Q], symbols, costs, margins, unmet): the key computed once, shared, never modified."""
    from oracle import pyoracle

    c = PLAIN[name]
    rng = _rng(name)
    H = make_H(rng, c["rows"], c["N"], c.get("cols"))
    Q = c["Q"]
    pmf = make_pmf(rng, batch, c["N"], Q, c["keep"])
    with np.errstate(divide="ignore", invalid="ignore"):
        symbols, costs = pyoracle.qary_min_sum_soft_batch(S.TannerGraph.from_dense(H), Q, pmf, ITERATIONS, threads=8)  # (raises if it refuses)
        margins, unmet = _soft(H, symbols, [costs], [(Q - 1) // 2])
    return _freeze(dict(H=H, B=(Q - 1) // 2, pmf=pmf, symbols=symbols, costs=costs, margins=margins, unmet=unmet))


@functools.lru_cache(maxsize=None)
def special_case(name, batch=BATCH):
    """dict(H, B, BSUM, pmf, pmf_sum, symbols, costs, costs_sum, margins, unmet)."""
    from oracle import pyoracle

    c = SPECIAL[name]
    B, BSUM = c["B"], c["SW"] * c["B"]
    QS = 2 * BSUM + 1
    H = special_graph(name)
    rng = _rng(name + " pmf")
    pb = make_pmf(rng, batch, SPECIAL_BV, 2 * B + 1, None)
    ps = make_pmf(rng, batch, SPECIAL_R, QS, (9 * QS) // 10)
    with np.errstate(divide="ignore", invalid="ignore"):
        symbols, cb, cs = pyoracle.qary_special_soft_batch(S.TannerGraph.from_dense(H), B, BSUM, pb, ps, ITERATIONS, threads=8)
        margins, unmet = _soft(H, symbols, [cb, cs], [B, BSUM])
    return _freeze(dict(H=H, B=B, BSUM=BSUM, pmf=pb, pmf_sum=ps, symbols=symbols, costs=np.ascontiguousarray(cb),
                        costs_sum=np.ascontiguousarray(cs), margins=margins, unmet=unmet))


def case(name, batch=BATCH):
    return plain_case(name, batch) if name in PLAIN else special_case(name, batch)


def sparse_support(name):
    """The case sets symbols to probability 0: its totals must then hold +inf or NaN entries next to finite ones."""
    return name in SPECIAL or PLAIN[name]["keep"] is not None
