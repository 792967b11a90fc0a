"""Shared inputs of tests/test_soft_priors.py (CPU) and tests/test_soft_priors_gpu.py: decodes whose codewords bring their
OWN priors (`BpDecoder.decode_batch(..., channel_probs=)`, scaldpc_bp_decode_batch_soft).

The answer key is the existing oracle, called once per codeword with that codeword's full prior vector.  Probabilities
are float32 values (widened for the oracle), so both sides see the same numbers."""
import functools
import importlib

import numpy as np

from helpers import ORACLE_METHOD, S, hqc_first_rows, sample_rows

trials = importlib.import_module("sca-ldpc_amd.trials")

# The two full-size points (HQC-128, first row N17669_W50_s0): per check a certainty drawn from `levels` with `weights`,
# the answer flipped with probability 1 - certainty; certainty 1.0 gives p = 0 (LLR +inf, hqc.py:689) next to finite ones.
SOFT_POINTS = {
    "hqc128_W50_R2000_soft": dict(name="hqc128", key="N17669_W50_s0", R=2000, levels=(1.0, 0.95, 0.8), weights=(0.5, 0.3, 0.2),
                                  base_seed=2, batch=4096),
    "hqc128_W50_R4000_soft": dict(name="hqc128", key="N17669_W50_s0", R=4000, levels=(1.0, 0.9, 0.7), weights=(0.2, 0.4, 0.4),
                                  base_seed=12, batch=4096),  # (the first base seed, counted up from 2, whose min-sum sample holds a stuck codeword)
}
MAX_ITER = 100
SAMPLE = sample_rows(4096, 4)  # the oracle sample: the first 4 codewords of the first, a middle and the last tile


@functools.lru_cache(maxsize=None)
def soft_graph(label):
    p = SOFT_POINTS[label]
    H, Hin, _ = S.codes.hqc_bench_graph(p["name"], hqc_first_rows()[p["key"]], R=p["R"])
    N, omega = S.codes.HQC_PARAMS[p["name"]]
    return H, Hin, N, omega


def soft_trials(label, indices):
    """Trials `indices` of a point (each seeded by its own index: the same trial whatever else is drawn).
    Returns (msg uint8 [k, n], ys, check_probs float32 [k, R])."""
    p = SOFT_POINTS[label]
    _, Hin, _, omega = soft_graph(label)
    parts = [trials.hqc_soft_trials(Hin, omega, p["levels"], p["weights"], 1, base_seed=p["base_seed"], first_index=int(i))
             for i in indices]
    msg = np.concatenate([q[0] for q in parts])
    ys = np.concatenate([q[1] for q in parts])
    cert = np.concatenate([q[2] for q in parts])
    return msg, ys, (1.0 - cert).astype(np.float32)


@functools.lru_cache(maxsize=None)
def soft_batch(label):
    """The whole GPU batch of a point (generated once per session)."""
    p = SOFT_POINTS[label]
    _, Hin, _, omega = soft_graph(label)
    msg, ys, cert = trials.hqc_soft_trials(Hin, omega, p["levels"], p["weights"], p["batch"], base_seed=p["base_seed"])
    return msg, ys, (1.0 - cert).astype(np.float32)


def shared_priors(label):
    """The decoder's own priors at a point: [omega / N] * N ++ [0.05] * R -- the check part is what a soft call with
    prob_cols = R replaces, so its value must not matter."""
    _, _, N, omega = soft_graph(label)
    R = SOFT_POINTS[label]["R"]
    return np.concatenate([np.full(N, omega / N), np.full(R, 0.05)])


def oracle_per_codeword(oracle, H, shared, tail_probs, x, kind, max_iter, method, early_exit=True, alpha=1.0):
    """The answer key: the f32 oracle in the kernels' operation order, ONE call per codeword with that codeword's full
    prior vector (the shared priors with their last k entries replaced by the codeword's row of `tail_probs`)."""
    tail_probs = np.asarray(tail_probs)
    k = tail_probs.shape[1]
    outs = []
    with np.errstate(divide="ignore"):
        for b in range(x.shape[0]):
            probs = np.concatenate([np.asarray(shared, dtype=np.float64)[: H.n - k], tail_probs[b].astype(np.float64)])
            outs.append(oracle.bp_decode_batch(H, probs, x[b : b + 1], kind, max_iter, ORACLE_METHOD[method], alpha=alpha,
                                               dtype="f32", threads=1, early_exit=early_exit))
    return {key: np.concatenate([o[key] for o in outs]) for key in outs[0]}


@functools.lru_cache(maxsize=None)
def sample_key(label, method, early_exit, max_iter):
    """Oracle result on SAMPLE of a full-size point (computed once per session, shared by the tests that need it)."""
    from oracle import pyoracle

    H, _, _, _ = soft_graph(label)
    msg, _, cp = soft_trials(label, SAMPLE)
    return oracle_per_codeword(pyoracle, H, shared_priors(label), cp, msg, 1, max_iter, method, early_exit=early_exit)


def take(res, idx):
    return {k: (v[idx] if v is not None else None) for k, v in res.items()}
