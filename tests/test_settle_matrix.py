"""tests/settle_matrix_cases.py -- the inputs of tests/test_settle_matrix_gpu.py -- held to what the GPU tests rely on.  On
every case the restatement's posteriors and decisions at max_iter are the float32 oracle's, bit for bit; every graph sits on
the kernel instantiation it is meant for; every case has a tile that freezes and one that does not; every codeword with a
random syndrome never settles; the horizon cases give a horizon by the rules of scaldpc_bp_sched.h and the forced-horizon
cases tiles to decode again.  These are conditions on the inputs: without them the GPU file could pass and exercise nothing.
No GPU."""
import numpy as np
import pytest

import settle_matrix_cases as M
import settle_ref as R

LADDER = ["base", "row32", "row64", "col32", "ties32", "ties64"]
STATIC = LADDER + ["wide_one", "wide_three", "base100", "grown", "extra"]


def _is_the_oracle(c, ref):
    assert (c.post.view(np.uint32) == ref["llr"].view(np.uint32)).all()
    assert ((c.post <= 0).astype(np.uint8) == ref["bits"]).all()
    assert (ref["iters"] == M.MAX_ITER).all()


@pytest.mark.parametrize("name", STATIC)
def test_restatement_is_the_oracle(oracle, name):
    _is_the_oracle(M.case(name), M.oracle_of(name))


def test_restatement_is_the_oracle_on_the_soft_call_and_the_sweeps(oracle):
    _is_the_oracle(M.soft(), M.soft_oracle())
    for kind in ("hqc", "fer"):
        for first in (0, M.SWEEP_FIRST2):
            _is_the_oracle(M.sweep(kind, first), M.sweep_oracle(kind, first))


def test_degrees_put_every_graph_on_its_instantiation():
    """k_check_minsum_rec<16 | 32 | 64> by the widest row, k_var_rec<16 | 32> by the widest column."""
    deg = {n: (np.asarray(M.case(n).H.row_degrees()), np.asarray(M.case(n).H.col_degrees())) for n in LADDER}
    print({n: (int(r.max()), int(c.min()), int(c.max())) for n, (r, c) in deg.items()})
    assert deg["base"][0].max() <= 16 and deg["base"][1].max() <= 16
    assert 17 <= deg["row32"][0].max() <= 32 and deg["row32"][1].max() <= 16
    assert 33 <= deg["row64"][0].max() <= 64 and deg["row64"][1].max() <= 16
    assert 17 <= deg["col32"][1].max() <= 32 and 17 <= deg["col32"][0].max() <= 32
    # (the compare-what-you-overwrite code is per degree: what the ladder adds to the base graph's rows of 11 and columns of 0 ... 8)
    assert set(deg["row32"][0].tolist()) == {18} and set(deg["row64"][0].tolist()) == {34}
    assert set(range(9, 18)) <= set(deg["col32"][1].tolist())
    for ties, shape in (("ties32", "row32"), ("ties64", "row64")):
        assert (deg[ties][0] == deg[shape][0]).all() and (deg[ties][1] == deg[shape][1]).all()
    # the partial last tile
    assert [len(M.case(n).synd) for n in LADDER] == [140, 140, 70, 140, 140, 70]


@pytest.mark.parametrize("name", ["ties32", "ties64"])
def test_tie_cases_end_on_an_arg_min_index_alone(name):
    """Every prior is one float, so rows are full of edges of equal magnitude; in some tile the last test that sees a difference
    sees it in arg-min indices alone: a check pass that left them out of its compare would report the tile frozen one test
    early.  (Such a change moves the index between two edges whose messages are equal, so the records say all there is to say
    about the messages -- but the state the device compares is (records, arg-min, signs), and so is the restatement's.)"""
    c = M.case(name)
    print(name, c.want, c.want_but_arg)
    assert len(set(np.asarray(c.probs).tolist())) == 1
    early = [t for t, (f, g) in enumerate(zip(c.want, c.want_but_arg)) if f and g == f - 1]
    assert early and all(g == f or t in early for t, (f, g) in enumerate(zip(c.want, c.want_but_arg)))


@pytest.mark.parametrize("name", LADDER + ["wide_one", "wide_three"])
def test_every_case_has_a_tile_that_freezes_and_one_that_does_not(name):
    c = M.case(name)
    print(name, c.want)
    assert any(c.want) and not all(c.want)
    at = R.settled_at(c.same, 3, M.MAX_ITER)
    assert all(at[b] == 0 for b in c.replaced)
    # a forced horizon below the largest frozen-at number is usable and leaves tiles to decode again
    K = M.short_horizon(c.want)
    assert M.usable(K) and K < max(c.want) and M.rerun(c.want, K) > 0
    # ... and, where more than one tile freezes, it also leaves one alone
    if sum(1 for f in c.want if f) > 1:
        assert M.rerun(c.want, K) < len(c.want)


def test_a_tile_freezes_at_the_next_to_last_test():
    assert any(f >= M.MAX_ITER - 1 for n in LADDER for f in M.case(n).want)
    assert M.case("row32").want[1] == M.MAX_ITER - 1


def test_the_soft_call_freezes_elsewhere():
    s, c = M.soft(), M.case("col32")
    print(s.want, c.want)
    assert any(s.want) and not all(s.want) and s.want != c.want[: len(s.want)]
    K = M.short_horizon(s.want)
    assert M.usable(K) and 0 < M.rerun(s.want, K) < len(s.want)
    assert s.cp.shape == (M.SOFT_BATCH, c.H.m) and (s.cp[0] != s.cp[1]).all()


def test_wide_cases_place_their_unfrozen_tiles():
    one, three = M.case("wide_one"), M.case("wide_three")
    assert len(one.synd) == len(three.synd) == M.WIDE == 64 * 9 + 3 and len(one.want) == 10
    assert [t for t, f in enumerate(one.want) if not f] == [5]
    assert [t for t, f in enumerate(three.want) if not f] == [2, 3, 6]
    # wide_one: a horizon is learned (at least 7/8 of the tiles freeze, 2 K < max_iter), and the call under it decodes one tile
    # again -- few enough to keep the horizon
    K = M.next_horizon(one.want, 0)
    assert K == max(one.want) + 2 and 2 * K < M.MAX_ITER and 8 * 9 >= 7 * 10
    assert M.rerun(one.want, K) == 1 and M.next_horizon(one.want, K) == K
    # wide_three: too few tiles freeze, nothing is learned; a forced horizon above every frozen-at number decodes the three again
    assert M.next_horizon(three.want, 0) == 0 and M.rerun(three.want, max(three.want) + 2) == 3
    # the frozen tiles do not all freeze at one test (a wrong word index would often go unseen otherwise)
    assert len({f for f in one.want if f}) >= 3


def test_the_growing_handle_learns_a_horizon_at_every_step():
    first, grown, extra = M.case("base100"), M.case("grown"), M.case("extra")
    print(first.want, grown.want, extra.want)
    assert first.H.m == M.GROW_FIRST and first.H.n == grown.H.n - 50 and extra.H.m == grown.H.m + 1 and extra.H.n == grown.H.n
    for c in (first, grown):
        assert all(c.want) and M.next_horizon(c.want, 0) == max(c.want) + 2
    assert any(extra.want)
    # the extra row: a column of Hin that had degree 1, and the identity column of row 7 (then the last edge of two rows)
    row = M.extra_row(grown.H)
    N = grown.H.n - grown.H.m
    before, after = np.asarray(grown.H.col_degrees()), np.asarray(extra.H.col_degrees())
    assert row[0] < N and before[row[0]] == 1 and row[1] == N + 7 and before[row[1]] == 1
    assert (after[row] == 2).all() and after.sum() == before.sum() + 2


@pytest.mark.parametrize("kind", ["hqc", "fer"])
def test_the_sweeps_learn_on_their_first_call(kind):
    """Trials 0 ... 139 freeze all three tiles: the second call (trials 1000 ... 1139) runs under their horizon, which is too
    short for one of its tiles; a forced horizon of 5 is too short for every tile of the first."""
    a, b = M.sweep(kind, 0), M.sweep(kind, M.SWEEP_FIRST2)
    print(kind, a.want, b.want)
    K = M.next_horizon(a.want, 0)
    assert all(a.want) and K == max(a.want) + 2
    assert M.rerun(b.want, K) == 1
    assert M.usable(M.SWEEP_HORIZON) and M.rerun(a.want, M.SWEEP_HORIZON) == 3


def test_rules_are_those_of_the_scheduler():
    """next_horizon / rerun / usable against the cases tests/test_settle_gpu.py already pins on the device."""
    assert M.next_horizon([11, 6], 0) == 13 and M.next_horizon([11, 0, 10], 0) == 0 and M.next_horizon([0, 0], 0) == 0
    assert M.next_horizon([23, 6], 0) == 0  # 2 K >= max_iter
    assert M.next_horizon([11], 8) == 0 and M.next_horizon([6], 13) == 8  # (test_nothing_carries_over_between_inputs)
    assert M.rerun([11, 0, 10, 9, 6, 6], 8) == 4 and M.rerun([11, 0], 0) == 0
    assert M.usable(3) and M.usable(48) and not M.usable(49) and not M.usable(2)
