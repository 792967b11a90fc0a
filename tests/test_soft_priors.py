"""Per-codeword channel priors (scaldpc_bp_decode_batch_soft), the host side -- no GPU.

  * `driver.hqc_decode_batch` with an oracle-backed decoder double equals `driver.hqc_decode` trial by trial;
  * `trials.hqc_soft_trials` is reproducible and independent of batch position;
  * the preconditions of tests/test_soft_priors_gpu.py, pinned from the oracle alone (as tests/test_production_range.py
    does for its points): the 12-codeword oracle sample of each full-size point holds, for both rules at max_iter 100, at
    least 3 distinct iteration counts, a converged and a stuck codeword, and +-inf next to finite check priors."""
import importlib

import numpy as np
import pytest

import soft_cases
from helpers import S
from oracle import pyoracle

driver = importlib.import_module("sca-ldpc_amd.driver")
trials = importlib.import_module("sca-ldpc_amd.trials")


class SoftOracleBp:
    """A decoder double with the product's surface, `channel_probs=` of `decode_batch` included: the CPU oracle called
    once per codeword with that codeword's priors (float32 values, as the library takes them)."""

    built = 0

    def __init__(self, H, max_iter=0, bp_method=0, channel_probs=(None,)):
        type(self).built += 1
        self.g = S.TannerGraph.coerce(H)
        self.n, self.m = self.g.n, self.g.m
        self.max_iter = max_iter or self.n
        self.method = {"product_sum": "product_sum", "min_sum": "min_sum"}[bp_method]
        self.probs = np.asarray(channel_probs, dtype=np.float64).astype(np.float32).astype(np.float64)  # (the library computes its LLRs from float32 values)

    def decode_batch(self, inputs, early_exit=True, input_vector_type=None, channel_probs=None):
        x = np.asarray(inputs, dtype=np.uint8)
        kind = {"syndrome": 0, "received_vector": 1}[input_vector_type]
        if channel_probs is None:
            return pyoracle.bp_decode_batch(self.g, self.probs, x, kind, self.max_iter, self.method, early_exit=early_exit)
        cp = np.asarray(channel_probs)
        assert cp.dtype == np.float32 and cp.ndim == 2 and cp.shape[0] == x.shape[0] and 1 <= cp.shape[1] <= self.n
        outs = []
        for b in range(x.shape[0]):
            probs = np.concatenate([self.probs[: self.n - cp.shape[1]], cp[b].astype(np.float64)])
            outs.append(pyoracle.bp_decode_batch(self.g, probs, x[b : b + 1], kind, self.max_iter, self.method, early_exit=early_exit))
        return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def _small_attack(seed, batch, weights_differ=False):
    N, W, R, omega = 997, 9, 300, 6
    rng = np.random.RandomState(seed)
    sup = S.codes.make_random_ldpc_first_row(N, W, rng)
    Hin = S.codes.hqc_check_graph(sup, N, rng.permutation(N)[:R])
    checks, ys = [], []
    for b in range(batch):
        w = omega + (b % 3 if weights_differ else 0)
        msg, y, cert = trials.hqc_soft_trials(Hin, w, (1.0, 0.9375, 0.75), (0.5, 0.4, 0.1), 1, base_seed=seed, first_index=b)
        checks.append([(int(v), float(c)) for v, c in zip(msg[0, N:], cert[0])])  # (certainties exact in float32)
        ys.append([int(j) for j in y[0]])
    return N, Hin, checks, ys


@pytest.mark.parametrize("weights_differ", [False, True])
def test_hqc_decode_batch_equals_hqc_decode_trial_by_trial(weights_differ):
    N, Hin, checks, ys = _small_attack(13, 9, weights_differ)
    SoftOracleBp.built = 0
    with np.errstate(divide="ignore"):
        got = driver.hqc_decode_batch(N, Hin, checks, ys, bp_decoder=SoftOracleBp, max_iter=30)
        assert SoftOracleBp.built == 1  # one decoder, one call
        want = [driver.hqc_decode(N, Hin, c, y, bp_decoder=SoftOracleBp, max_iter=30) for c, y in zip(checks, ys)]
    assert got == want
    assert any(s for s, _ in want) and len({st["unsatisfied"] for _, st in want}) > 1  # (the trials are not all alike)


def test_hqc_decode_batch_refuses_ragged_input():
    N, Hin, checks, ys = _small_attack(11, 3)
    with pytest.raises(ValueError):
        driver.hqc_decode_batch(N, Hin, checks, ys[:2], bp_decoder=SoftOracleBp)
    with pytest.raises(ValueError):
        driver.hqc_decode_batch(N, Hin, [checks[0], checks[1][:-1], checks[2]], ys, bp_decoder=SoftOracleBp)


def test_generator_is_reproducible_and_independent_of_batch_position():
    _, Hin, N, omega = soft_cases.soft_graph("hqc128_W50_R2000_soft")
    lv, wt = (1.0, 0.95, 0.8), (0.5, 0.3, 0.2)
    a = trials.hqc_soft_trials(Hin, omega, lv, wt, 6, base_seed=9)
    b = trials.hqc_soft_trials(Hin, omega, lv, wt, 6, base_seed=9)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = trials.hqc_soft_trials(Hin, omega, lv, wt, 2, base_seed=9, first_index=3)
    assert all(np.array_equal(x[3:5], y) for x, y in zip(a, c))
    d = trials.hqc_soft_trials(Hin, omega, lv, wt, 2, base_seed=12)  # trial i is seeded base_seed + i
    assert all(np.array_equal(x[3:5], y) for x, y in zip(a, d))
    msg, ys, cert = a
    assert msg.shape == (6, N + Hin.m) and ys.shape == (6, omega) and cert.shape == (6, Hin.m)
    assert set(np.unique(cert).tolist()) == set(lv) and not msg[:, :N].any()
    # the secrets are hqc_trials' own; the answers differ from the noise-free ones only where the certainty is below 1
    clean, ys0 = trials.hqc_trials(Hin, omega, 0.0, 6, base_seed=9)
    assert np.array_equal(ys, ys0)
    flipped = msg[:, N:] != clean[:, N:]
    assert flipped.any() and not flipped[cert == 1.0].any()
    share = np.array([(cert == v).mean() for v in lv])
    assert np.abs(share - np.array(wt)).max() < 0.03
    assert abs(flipped[cert == 0.8].mean() - 0.2) < 0.03
    with pytest.raises(ValueError):
        trials.hqc_soft_trials(Hin, omega, (1.0, 1.5), (0.5, 0.5), 1)


@pytest.mark.parametrize("label", list(soft_cases.SOFT_POINTS))
@pytest.mark.parametrize("method", ["min_sum", "product_sum"])
def test_oracle_sample_is_hard_enough(label, method):
    msg, _, cp = soft_cases.soft_trials(label, soft_cases.SAMPLE)
    assert soft_cases.SAMPLE.size == 12 and cp.dtype == np.float32
    assert (cp == 0.0).any(axis=1).all() and ((cp > 0.0) & (cp < 0.5)).any(axis=1).all()  # +-inf and finite priors side by side
    assert len({row.tobytes() for row in cp}) == 12  # every codeword has priors of its own
    r = soft_cases.sample_key(label, method, True, soft_cases.MAX_ITER)
    conv = r["converged"].astype(bool)
    counts = sorted(set(r["iters"].tolist()))
    print(label, method, "converged %d of 12" % conv.sum(), "iteration counts", counts)
    assert len(counts) >= 3, counts
    assert conv.any() and not conv.all()
    assert (r["iters"][~conv] == soft_cases.MAX_ITER).all()
