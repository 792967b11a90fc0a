"""tests/settle_ref.py -- the NumPy float32 restatement of the min-sum record form that says when a codeword's message state
has stopped changing -- held to the float32 oracle, bit for bit: decisions and posteriors at every max_iter from 1 to 12 and
at 50, on the graphs of tests/test_settle_gpu.py.  The second half asserts what those GPU cases rely on: that their inputs
contain what they claim."""
import numpy as np
import pytest

import settle_ref as R

ITERS = tuple(range(1, 13)) + (50,)


@pytest.mark.parametrize("name", ["hqc", "schedule", "regular"])
def test_restatement_is_the_oracle(oracle, name):
    c = R.case(name)
    for mi in ITERS:
        ref = R.oracle_at(name, mi)
        post = c.post[mi]
        assert (post.view(np.uint32) == ref["llr"].view(np.uint32)).all(), (name, mi)
        assert ((post <= 0).astype(np.uint8) == ref["bits"]).all(), (name, mi)
        assert (ref["iters"] == mi).all()


def test_settled_is_a_fixed_point():
    """A codeword whose test t found no difference shows none in any later test, and its posterior stays what it is."""
    for name in ("hqc", "schedule", "regular"):
        c = R.case(name)
        s = c.same[c.first :]
        assert (s[1:] >= s[:-1]).all()
        at = R.settled_at(c.same, c.first, R.MAX_ITER)
        for b in np.flatnonzero(at)[:40]:
            p = c.post[at[b] :, b].view(np.uint32)
            assert (p == p[0]).all()


def test_hqc_inputs_settle_at_different_iterations():
    c = R.case("hqc")
    at = R.settled_at(c.same, 3, R.MAX_ITER)
    settled = at[at > 0]
    lo, hi = int(settled.min()), int(settled.max())
    print("settled-at histogram:", np.bincount(at), "frozen-at:", R.frozen_at(c.same, 3, R.MAX_ITER))
    assert 4 <= lo < hi <= 12  # the GPU cases sweep max_iter over [lo - 1, hi + 1]: keep that a dozen values
    assert (at == 0).sum() >= 1  # some codeword never settles: its tile never freezes
    fz = R.frozen_at(c.same, 3, R.MAX_ITER)
    assert len(fz) == 6 and 0 in fz and max(fz) == hi and sum(1 for f in fz if f) >= 3
    # batch 70: both tiles freeze, the partial one earlier -- and with K = largest + 2 a horizon is worth learning
    fz70 = R.frozen_at(c.same, 3, R.MAX_ITER, batch=70)
    assert len(fz70) == 2 and 0 < fz70[1] < fz70[0] and 2 * (fz70[0] + 2) < R.MAX_ITER
    # at every max_iter strictly between the first and the last settle iteration, some tile holds both settled and
    # unsettled codewords; that holds inside the first 70 codewords too
    for batch in (R.BATCH, 70):
        for mi in range(lo, hi):
            mixed = [t0 for t0 in range(0, batch, R.TW)
                     if len({bool(0 < a <= mi) for a in at[t0 : min(t0 + R.TW, batch)]}) == 2]  # fmt: skip
            assert mixed, (batch, mi)
    # a forced horizon of 8 is below the largest frozen-at number and above the smallest
    assert min(f for f in fz if f) <= 8 < max(fz)


def test_regular_inputs_never_settle():
    c = R.case("regular")
    assert not c.same[3:].any()
    assert R.frozen_at(c.same, 3, R.MAX_ITER) == [0, 0]
    assert (np.asarray(c.H.col_degrees()) == 3).all() and (np.asarray(c.H.row_degrees()) == 6).all()


def test_schedule_inputs():
    """The 1 - 2^-it schedule is one float (1.0f) from iteration 25 on: no test before 26, and tiles do freeze after it."""
    c = R.case("schedule")
    assert R.alpha_for(0.0, 24) < 1 and R.alpha_for(0.0, 25) == 1
    assert c.first == 26 and R.first_test(0.0, 20) == 21 and R.first_test(1.0, 50) == 3
    fz = R.frozen_at(c.same, c.first, R.MAX_ITER)
    print("schedule frozen-at:", fz)
    assert len(fz) == 2 and any(fz)
