"""TEST INFRASTRUCTURE: the trial laws of scaldpc_mc_fer_run and scaldpc_mc_hqc_run (include/scaldpc.h) restated in NumPy on
the generators of oracle/mc_oracle.c, and the instances the CPU and GPU edge tests of the two entries share
(tests/test_mc_edges.py pins what makes them hard enough, tests/test_mc_edges_gpu.py holds the kernels to them)."""
import functools

import numpy as np

from helpers import hqc_instance
from oracle import pyoracle

SEED = 0xC0FFEE12345  # both key words in use: seed >> 32 = 0xC0F
FIRST = 2**32 - 30  # the trial index crosses 2^32 inside the first tile of every batch of more than 30
MAX_ITER = 30
RUNS = 130  # two full tiles and a ragged third of 2 codewords
SAMPLE = 24  # trials of each instance that go through the CPU decoder


def fer(seed, first, batch, graph, probs):
    """FER trials first .. first + batch - 1: (errors uint8 [batch, n], syndromes uint8 [batch, m])."""
    err = pyoracle.mc_bernoulli(seed, first, batch, graph.n, probs)
    return err, graph.syndrome(err)


def secret_vectors(y, N):
    """Indicator vectors uint8 [batch, N] of the positions y int32 [batch, omega]."""
    yv = np.zeros((y.shape[0], N), dtype=np.uint8)
    if y.shape[1]:
        np.put_along_axis(yv, y.astype(np.int64), 1, axis=1)
    return yv


def hqc(seed, first, batch, Hin, omega, eps):
    """HQC trials first .. first + batch - 1 on [Hin | I]: (y int32 [batch, omega] in draw order, msg uint8 [batch, N + R] =
    [0]*N ++ (Hin y ^ flips), flips ~ Bernoulli(eps) on the stream-0 words of the checks)."""
    N, R = Hin.n, Hin.m
    y = pyoracle.mc_hqc_secret(seed, first, batch, N, omega)
    checks = Hin.syndrome(secret_vectors(y, N)) ^ pyoracle.mc_bernoulli(seed, first, batch, R, None, eps)
    return y, np.concatenate([np.zeros((batch, N), dtype=np.uint8), checks], axis=1)


# ------------------------------------------------------------------------------------------------------------------ instances
@functools.lru_cache(maxsize=None)
def instance(name):
    """dict(H, Hin, probs, N, R, omega, eps).  Built once per session, shared, left unchanged.
      F    FER on the 70 x 201 graph of an HQC shape: n = 201 is no multiple of 4, 16 or 64; priors 0.02 / 0.05 with p = 0,
           p = 1 and p < 2^-32 among them, at the first and the last column and on both sides of the identity block
      H1   HQC N = 67, R = 45, omega = 3, eps = 0.05
      H2   HQC N = 131, R = 70, omega = 4, eps = 0.06
      H2_eps1  H2's graph, every check flipped and the priors saying so
      S499 the N = 499, R = 260 graph of tests/test_mc_gpu.py (secrets of weight 0 and 256)
      S7, S16  N = 7, R = 3 and N = 16, R = 13: secrets that are permutations of all positions"""
    shape = dict(F=(131, 5, 70, 3, 0.05), H1=(67, 5, 45, 3, 0.05), H2=(131, 5, 70, 4, 0.06), H2_eps1=(131, 5, 70, 4, 1.0),
                 S499=(499, 7, 260, 5, 0.04), S7=(7, 2, 3, 7, 0.05), S16=(16, 3, 13, 16, 0.05))[name]
    N, W, R, omega, eps = shape
    H, Hin, probs, _, _ = hqc_instance(N, W, R, omega, eps, 1, seed=11, flip=False)
    if name == "F":
        probs = np.array([0.02] * N + [0.05] * R)
        probs[[0, 1, 2, N, -1]] = [0.0, 1.0, 2.0**-33, 1.0, 0.0]
    probs.setflags(write=False)
    return dict(H=H, Hin=Hin, probs=probs, N=N, R=R, omega=omega, eps=eps)


@functools.lru_cache(maxsize=None)
def fer_law(name="F", first=FIRST, runs=RUNS, seed=SEED):
    i = instance(name)
    err, synd = fer(seed, first, runs, i["H"], i["probs"])
    return dict(errors=err, synd=synd)


@functools.lru_cache(maxsize=None)
def hqc_law(name, first=FIRST, runs=RUNS, seed=SEED, omega=None, eps=None):
    i = instance(name)
    y, msg = hqc(seed, first, runs, i["Hin"], i["omega"] if omega is None else omega, i["eps"] if eps is None else eps)
    return dict(y=y, msg=msg)


ORACLE_METHOD = {"min_sum": "min_sum", "product_sum": "tanh_complement"}


@functools.lru_cache(maxsize=None)
def oracle_decode(name, method, runs=RUNS, early_exit=True, max_iter=MAX_ITER, eps=None):
    """The f32 CPU decoder on the first `runs` trials of an instance: dict(bits, llr, iters, converged, success)."""
    i = instance(name)
    with np.errstate(divide="ignore", invalid="ignore"):
        if name == "F":
            law = fer_law()
            d = pyoracle.bp_decode_batch(i["H"], i["probs"], law["synd"][:runs], 0, max_iter, ORACLE_METHOD[method], dtype="f32",
                                         threads=4, early_exit=early_exit)
            d["success"] = (d["bits"] == law["errors"][:runs]).all(axis=1).astype(np.uint8)
        else:
            law = hqc_law(name, eps=eps)
            d = pyoracle.bp_decode_batch(i["H"], i["probs"], law["msg"][:runs], 1, max_iter, ORACLE_METHOD[method], dtype="f32",
                                         threads=4, early_exit=early_exit)
            d["success"] = hqc_success(d["bits"], law["y"][:runs], i["N"])
    return d


def hqc_success(bits, y, N):
    """decoded[:N] is the indicator of y (simulate/hqc.py:742-749)."""
    return (bits[:, :N] == secret_vectors(y, N)).all(axis=1).astype(np.uint8)
