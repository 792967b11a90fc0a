"""DecoderSpecial on checks of any length: k_q_special_check_dp_any (csrc/scaldpc_qary_special.h) on the GPU, through the
three-field names DecoderN{N}R{R}SW{SW}B{B} and the C ABI.  Every decoder here beyond seven coefficient edges per check is
refused without the kernel (SCALDPC_EDEGREE at creation).

  1. forced (dp_any = 1) onto shapes the other kernels run: the same symbols as theirs, and as the oracle's on the small ones;
  2. rows of up to 12 coefficient edges, mixed with rows of 0 - 3, against the oracle (decoder_special.rs:471-617 restated);
  3. cycle-free graphs against exact min-marginals (tests/exact.py): no decoder in the answer key;
  4. 256 x 1024 at sum weight 9: B = 1 against the oracle; B = 2 (1.95 M assignments per check: no oracle) on what can be said
     without one -- valid words are fixed points, batch positions do not matter, soft == plain, unmet == H x != 0;
  5. the message-level equivalence program (profiles/microbench/qary_dp_any_equivalence.hip);
  6. limits and lifetime.
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exact
from helpers import S

pytestmark = pytest.mark.gpu
qary = importlib.import_module("sca-ldpc_amd.qary")
lib = importlib.import_module("sca-ldpc_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_q_special_check_dp_any"


def random_special_H(rng, coeffs, BV):
    """[H' | I]: row r has coeffs[r] entries of +-1 among the BV coefficient columns."""
    R = len(coeffs)
    H = np.zeros((R, BV + R), dtype=np.int8)
    for r, k in enumerate(coeffs):
        H[r, rng.choice(BV, k, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), size=k)
        H[r, BV + r] = 1
    return H


def special_class(H, B, SW):
    R, N = H.shape
    return qary.decoder_class(f"DecoderN{N}R{R}SW{SW}B{B}")


def draw_pmfs(rng, batch, BV, R, B, BSUM, ab=0.6, asum=0.6, zeros=False):
    pb = rng.dirichlet(np.ones(2 * B + 1) * ab, size=(batch, BV)).astype(np.float32)
    ps = rng.dirichlet(np.ones(2 * BSUM + 1) * asum, size=(batch, R)).astype(np.float32)
    if zeros:  # some costs are +inf
        pb[:, ::7, 0] = 0.0
        pb /= pb.sum(axis=2, keepdims=True)
    return pb, ps


def timed_kernel(dec, pb, ps):
    dec.configure(timing=1)
    out = dec.min_sum_batch(pb, ps)
    name = dec.last_timing()["check_kernel"]
    dec.configure(timing=0)
    return out, name


# ------------------------------------------------------------------------------- 1. forced onto shapes other kernels run
def _forced_cases(golden):
    g = S.codes.make_qary_qc_graph(16, 3, 3, S.codes.make_random_state(0), 2)  # 32 x 80, SW 3
    yield "sw3", g.to_dense(np.int8), 2, 3, 70, 4, True
    gk = S.TannerGraph.from_coo(golden["generators"]["qary_qc_256_6_3_s0_cb1"])  # DecoderN1024R256SW6
    yield "kyber_sw6", gk.to_dense(np.int8), 2, 6, 70, 2, False
    yield "b3_sw4", random_special_H(np.random.RandomState(31), [4, 4, 2, 1, 3, 4, 1], 14), 3, 4, 70, 3, True
    yield "b1_sw5", random_special_H(np.random.RandomState(32), [5, 1, 5, 3, 2, 4, 5, 2], 16), 1, 5, 70, 3, True


@pytest.mark.parametrize("which", ["sw3", "kyber_sw6", "b3_sw4", "b1_sw5"])
def test_forced_onto_shapes_other_kernels_run(oracle, golden, which):
    name, H, B, SW, batch, iters, small = next(c for c in _forced_cases(golden) if c[0] == which)
    R, N = H.shape
    pb, ps = draw_pmfs(np.random.RandomState(len(which) + SW), batch, N - R, R, B, SW * B, zeros=small)
    dec = special_class(H, B, SW)(H, iters)
    with np.errstate(divide="ignore"):
        want, default_kernel = timed_kernel(dec, pb, ps)
        assert default_kernel != KERNEL  # the default for these shapes is what it was
        dec.configure(dp_any=1)
        got, kernel = timed_kernel(dec, pb, ps)
        assert kernel == KERNEL
        assert np.array_equal(got, want)
        soft = dec.min_sum_soft_batch(pb, ps)
        assert np.array_equal(soft["symbols"], want)
        dec.configure(dp_any=-1)
        assert timed_kernel(dec, pb, ps)[1] == default_kernel
        if small:
            ref = oracle.qary_special_batch(S.TannerGraph.from_dense(H), B, SW * B, pb, ps, iters, threads=8)
            assert np.array_equal(got, ref)
    dec.close()


# ------------------------------------------------------------------------------ 2. rows beyond eight edges against the oracle
LONG_ROWS = {
    "b2": (2, [9, 9, 8, 9, 3, 0, 1], 24, 3, 2),
    "b1": (1, [12, 10, 9, 12, 11, 2, 0, 1], 30, 8, 3),
    "b3": (3, [8, 3, 8, 6, 0], 20, 2, 2),
}


@pytest.mark.parametrize("which", sorted(LONG_ROWS))
def test_long_rows_against_the_oracle(oracle, which):
    B, coeffs, BV, batch, iters = LONG_ROWS[which]
    SW, R = max(coeffs), len(coeffs)
    BSUM = SW * B
    H = random_special_H(np.random.RandomState(50 + B), coeffs, BV)
    pb, ps = draw_pmfs(np.random.RandomState(60 + B), batch, BV, R, B, BSUM, zeros=True)
    dec = special_class(H, B, SW)(H, iters)
    with np.errstate(divide="ignore"):
        ref = oracle.qary_special_batch(S.TannerGraph.from_dense(H), B, BSUM, pb, ps, iters, threads=8)
        got, kernel = timed_kernel(dec, pb, ps)
        assert kernel == KERNEL
        assert np.array_equal(got, ref)
        assert (ref != 0).any()
        # the same codewords at lanes 0, 63, 64 and 69 of a ragged batch of other draws (two blocks per check)
        fb, fs = draw_pmfs(np.random.RandomState(70 + B), 70, BV, R, B, BSUM, zeros=True)
        pos = [0, 63, 64, 69]
        for i, p in enumerate(pos):
            fb[p], fs[p] = pb[i % batch], ps[i % batch]
        big = dec.min_sum_batch(fb, fs)
        soft = dec.min_sum_soft_batch(fb, fs)
    for i, p in enumerate(pos):
        assert np.array_equal(big[p], ref[i % batch]), p
    assert np.array_equal(soft["symbols"], big)
    assert np.array_equal(soft["unmet"], (big.astype(np.int64) @ H.T.astype(np.int64) != 0).sum(axis=1))
    dec.close()


# ------------------------------------------------------------------------------------ 3. exact inference on cycle-free graphs
TREES = {
    "b1": (1, [12, 9, 10, 11, 2, 9], 901, 8, 14),
    "b2_three": (2, [9, 8, 9], 902, 3, 8),
    "b2_four": (2, [10, 3, 9, 8], 903, 3, 10),
}


def special_tree_case(B, coeffs, seed, batch):
    """A cycle-free [H' | +-I] (tests/exact.py: random_special_tree, the identity part signed as large_special_tree_case of
    tests/test_exact_inference.py signs it) with its exact min-marginals and that case's clearness rule."""
    rng = np.random.RandomState(seed)
    R = len(coeffs)
    BSUM = max(coeffs) * B
    H = exact.random_special_tree(rng, R, coeffs)
    H[:, H.shape[1] - R:] *= rng.choice(np.array([-1, 1], dtype=np.int8), size=R)[None, :]
    BV = H.shape[1] - R
    pb = rng.dirichlet(np.ones(2 * B + 1) * 1.2, size=(batch, BV)).astype(np.float32)
    ps = rng.dirichlet(np.ones(2 * BSUM + 1) * 0.6, size=(batch, R)).astype(np.float32)
    dec = np.zeros((batch, H.shape[1]), dtype=np.int8)
    ok = np.zeros((batch, H.shape[1]), dtype=bool)
    alph = [B] * BV + [BSUM] * R
    for b in range(batch):
        llr = [exact.pmf_to_llr64(pb[b][v]) for v in range(BV)] + [exact.pmf_to_llr64(ps[b][r]) for r in range(R)]
        mm = exact.tree_exact_qary(H, llr, alph)
        top = max(float(np.min(m)) for m in mm)
        for v, m in enumerate(mm):
            srt = np.sort(m)
            dec[b, v] = int(np.argmin(m)) - alph[v]
            ok[b, v] = srt[1] - srt[0] > 1e-3 * max(1.0, top)
    return H, BSUM, pb, ps, dec, ok


@pytest.mark.parametrize("which", sorted(TREES))
def test_cycle_free_graphs_against_exact_min_marginals(which):
    B, coeffs, seed, batch, iters = TREES[which]
    H, BSUM, pb, ps, want, ok = special_tree_case(B, coeffs, seed, batch)
    assert exact.is_forest(H)
    dec = special_class(H, B, max(coeffs))(H, iters)
    got, kernel = timed_kernel(dec, pb, ps)
    dec.close()
    assert kernel == KERNEL
    assert ok.mean() >= 0.95 and np.array_equal(got[ok], want[ok])


# ------------------------------------------------------------------------------------------------------------ 4. full size
@pytest.fixture(scope="module")
def sw9_graph():
    g = S.codes.make_qary_qc_graph(256, 9, 3, S.codes.make_random_state(0), 1)
    H = g.to_dense(np.int8)
    assert H.shape == (256, 1024) and set(np.abs(H).sum(axis=1)) == {10}
    return g, H


def test_full_size_b1_against_the_oracle(oracle, sw9_graph):
    g, H = sw9_graph
    pb, ps = draw_pmfs(np.random.RandomState(80), 4, 768, 256, 1, 9, ab=1.0, asum=1.0)
    dec = qary.decoder_class("DecoderN1024R256SW9B1")(H, 5)
    got, kernel = timed_kernel(dec, pb, ps)
    dec.close()
    assert kernel == KERNEL
    assert np.array_equal(got, oracle.qary_special_batch(g, 1, 9, pb, ps, 5, threads=8))


def test_full_size_b2_without_an_oracle(sw9_graph):
    _, H = sw9_graph
    B, BSUM, BV, R, batch = 2, 18, 768, 256, 256
    rng = np.random.RandomState(81)
    dec = qary.decoder_class("DecoderN1024R256SW9B2")(H, 5)
    assert (dec.B, dec.BSUM, dec.Q, dec.QS, dec.DC) == (2, 18, 5, 37, 10)
    # valid words: any coefficient vector, row-sum values -H' x; the channel output peaked at them
    x = rng.randint(-B, B + 1, size=(batch, BV))
    s = -(x @ H[:, :BV].T.astype(np.int64))
    assert np.abs(s).max() <= BSUM
    word = np.concatenate([x, s], axis=1).astype(np.int8)
    assert not (word.astype(np.int64) @ H.T.astype(np.int64)).any()
    pb = np.full((batch, BV, 2 * B + 1), 0.1 / (2 * B), dtype=np.float32)
    ps = np.full((batch, R, 2 * BSUM + 1), 0.1 / (2 * BSUM), dtype=np.float32)
    np.put_along_axis(pb, (x + B)[:, :, None], 0.9, axis=2)
    np.put_along_axis(ps, (s + BSUM)[:, :, None], 0.9, axis=2)
    got, kernel = timed_kernel(dec, pb, ps)
    assert kernel == KERNEL
    assert np.array_equal(got, word)
    soft = dec.min_sum_soft_batch(pb, ps, costs=False, margins=False)
    assert np.array_equal(soft["symbols"], word) and not soft["unmet"].any()
    # noisy inputs: soft == plain, unmet == H x != 0, and the batch position does not matter
    nb_, ns_ = draw_pmfs(rng, batch, BV, R, B, BSUM, ab=0.5, asum=0.3)
    noisy_b, noisy_s = (0.5 * pb + 0.5 * nb_).astype(np.float32), (0.5 * ps + 0.5 * ns_).astype(np.float32)
    noisy_b[200], noisy_s[200] = nb_[200], ns_[200]  # (one codeword of pure noise: unmet checks for certain)
    for p in (0, 63, 64, 255):
        noisy_b[p], noisy_s[p] = noisy_b[100], noisy_s[100]
    plain = dec.min_sum_batch(noisy_b, noisy_s)
    soft = dec.min_sum_soft_batch(noisy_b, noisy_s, costs=False, margins=False)
    unmet = (plain.astype(np.int64) @ H.T.astype(np.int64) != 0).sum(axis=1)
    assert np.array_equal(soft["symbols"], plain) and np.array_equal(soft["unmet"], unmet) and unmet.any()
    for p in (0, 63, 64, 255):
        assert np.array_equal(plain[p], plain[100]), p
    assert np.array_equal(dec.min_sum_batch(noisy_b[100:101], noisy_s[100:101])[0], plain[100])
    assert np.array_equal(dec.min_sum_batch(noisy_b[90:160], noisy_s[90:160]), plain[90:160])
    dec.close()


# ------------------------------------------------------------------------------------------ 5. the equivalence program
def test_the_kernel_equals_the_enumeration_message_for_message():
    mb = os.path.join(ROOT, "profiles", "microbench")
    subprocess.check_call(["make", "-C", mb, "qary_dp_any_equivalence"], stdout=subprocess.DEVNULL)  # (a no-op when built)
    out = subprocess.run([os.path.join(mb, "qary_dp_any_equivalence")], capture_output=True, text=True, timeout=300)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("CASE")]
    bad = [ln for ln in lines if any(int(n) for n in re.findall(r"(\d+) differ", ln))]
    assert out.returncode == 0 and not bad, "\n".join(bad) + out.stderr[-2000:]
    assert len(lines) == 15 * 2 * 6  # 15 row shapes x 2 row-sum alphabets x 6 input flavours
    assert sum("dp<5,6,1>" in ln for ln in lines) == 12  # the Kyber kernel, held to the same messages
    assert all(re.search(r"(\d+) differ", ln) for ln in lines)


# ------------------------------------------------------------------------------------------------ 6. limits and lifetime
def test_limits_and_lifetime(sw9_graph):
    L = lib.load()
    keys = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")
    base = lib.live_blocks()
    # B = 4 at degree 10: no kernel, SCALDPC_EDEGREE from the C ABI with the limit in the message
    H = random_special_H(np.random.RandomState(5), [9, 2], 12)
    h = C.c_void_p()
    rc = L.scaldpc_qary_special_create(2, 14, 4, 36, lib.ptr(H), 2, C.byref(h))
    assert rc != 0 and rc != lib.EINVAL and not h.value
    msg = L.scaldpc_last_error()
    assert b"check degree 10" in msg and b"85" in msg
    b4 = type("DecoderB4", (qary.QarySpecialDecoder,), dict(N=14, R=2, DV=2, DC=10, B=4, Q=9, BSUM=36, QS=73))
    with pytest.raises(lib.ScaldpcError, match=rf"\[{rc}\]"):
        b4(H, 2)
    # B = 3 at degree 16 (91 table entries) likewise; degree 15 (85) is built
    H16 = random_special_H(np.random.RandomState(6), [15, 1], 15)
    assert L.scaldpc_qary_special_create(2, 17, 3, 45, lib.ptr(H16), 1, C.byref(h)) == rc and not h.value
    H15 = random_special_H(np.random.RandomState(6), [14, 1], 15)
    d15 = qary.decoder_class("DecoderN17R2SW14B3")(H15, 1)
    pb, ps = draw_pmfs(np.random.RandomState(7), 2, 15, 2, 3, 42, ab=1.0, asum=1.0)
    assert timed_kernel(d15, pb, ps)[1] == KERNEL  # (65 280 bytes of LDS per block)
    d15.close()
    assert all(lib.live_blocks()[k] == base[k] for k in keys)
    # a shape the knob refuses: nothing is queued, nothing allocated, the output untouched; the handle decodes afterwards
    H9 = random_special_H(np.random.RandomState(8), [9, 9, 4], 20)
    dec = qary.decoder_class("DecoderN23R3SW9B2")(H9, 2)
    pb, ps = draw_pmfs(np.random.RandomState(9), 3, 20, 3, 2, 18)
    before = lib.live_blocks()
    dec.configure(dp_any=0)
    out = np.full((3, 23), 77, dtype=np.int8)
    assert L.scaldpc_qary_special_min_sum_batch(dec._h, lib.ptr(pb), lib.ptr(ps), 3, 0, None, lib.ptr(out)) == rc
    assert b"dp_any" in L.scaldpc_last_error() and (out == 77).all()
    sym = np.full((3, 23), 77, dtype=np.int8)
    unmet = np.full(3, -5, dtype=np.int32)
    assert L.scaldpc_qary_special_min_sum_batch_soft(dec._h, lib.ptr(pb), lib.ptr(ps), 3, 0, None, lib.ptr(sym), None, None, None,
                                                     lib.ptr(unmet)) == rc
    assert (sym == 77).all() and (unmet == -5).all()
    assert all(lib.live_blocks()[k] == before[k] for k in keys)
    dec.configure(dp_any=-1)
    got = dec.min_sum_batch(pb, ps)
    soft = dec.min_sum_soft_batch(pb, ps)
    assert np.array_equal(soft["symbols"], got)
    assert np.array_equal(soft["unmet"], (got.astype(np.int64) @ H9.T.astype(np.int64) != 0).sum(axis=1))
    dec.close()
    # create / call / close on the full-size shape returns every block
    _, H = sw9_graph
    big = qary.decoder_class("DecoderN1024R256SW9B2")(H, 1)
    pb, ps = draw_pmfs(np.random.RandomState(10), 2, 768, 256, 2, 18, ab=1.0, asum=1.0)
    big.min_sum_soft_batch(pb, ps)
    assert lib.live_blocks()["device_blocks"] > base["device_blocks"]
    big.close()
    assert all(lib.live_blocks()[k] == base[k] for k in keys)
    drop = os.path.join(ROOT, "sca-ldpc_amd", "dropin")
    if drop not in sys.path:
        sys.path.insert(0, drop)
    import simulate_rs

    assert getattr(simulate_rs, "DecoderN33R5SW9B2") is qary.decoder_class("DecoderN33R5SW9B2")
