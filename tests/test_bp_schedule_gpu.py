"""Every branch of the early-exit tile scheduler, driven on the device and held to the oracle.

Batches are COMPOSED: the f32 oracle decodes a pool of 3000 trials of `hqc_instance(997, 9, 450, omega, 0.03, seed=21)`
with early exit and 40 iterations, and codewords are picked by the oracle's iteration count (repeats allowed: codewords
are independent), so that each group's remainders send the scheduler down one chosen path.  What the call computed is
compared with the oracle's results of the picked codewords -- min-sum bit for bit (decisions, posteriors, iteration counts,
flags), the tanh rule by `helpers.compare` -- and the schedule it ran (`BpDecoder.last_schedule`) with what
tests/sched_model.py predicts from the oracle's iteration counts alone: integer for integer in min-sum; for the tanh
rule, where a tie may move one count by one, the facts each case names."""
import functools
import importlib

import numpy as np
import pytest

import sched_model as M
from helpers import ORACLE_METHOD, compare, hqc_instance

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")

N, W, R, EPS, POOL, MAX_ITER, SEED = 997, 9, 450, 0.03, 3000, 40, 21
SOFT_ROWS = (np.float32(0.03), np.float32(0.031))  # a soft call's check priors: pool codeword i brings row i % 2
FORMS = [("min_sum", 0), ("min_sum", 1), ("product_sum", 0), ("product_sum", 1)]


@functools.lru_cache(maxsize=None)
def instance(omega):
    H, _, probs, msg, _ = hqc_instance(N, W, R, omega, EPS, POOL, seed=SEED)
    return H, probs, msg


@functools.lru_cache(maxsize=None)
def pool(omega, method, soft=False):
    """The oracle's results on the whole pool (computed once, shared, never changed)."""
    from oracle import pyoracle

    H, probs, msg = instance(omega)
    threads = max(1, min(8, pyoracle.max_threads()))

    def run(p):
        return pyoracle.bp_decode_batch(H, p, msg, 1, MAX_ITER, ORACLE_METHOD[method], dtype="f32", threads=threads, early_exit=True)

    if not soft:
        ref = run(probs)
    else:  # one oracle call per prior row, each codeword takes the results of its own row
        rows = [run(np.concatenate([probs[:N], np.full(R, float(p))])) for p in SOFT_ROWS]
        pick = np.arange(POOL) % 2
        ref = {k: np.where(pick.reshape((-1,) + (1,) * (rows[0][k].ndim - 1)) == 0, rows[0][k], rows[1][k]) for k in rows[0]}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def classes(ref):
    """Pool indices by the oracle's iteration count: {k: converged after exactly k iterations}, "never": not converged."""
    conv = ref["converged"].astype(bool)
    out = {k: np.flatnonzero(conv & (ref["iters"] == k)) for k in range(1, MAX_ITER + 1)}
    out["never"] = np.flatnonzero(~conv)
    return out


def take(rng, cls, keys, count):
    """`count` pool indices whose class is one of `keys` (asserted to exist), cycling through them if there are fewer."""
    have = np.concatenate([cls[k] for k in keys])
    assert have.size >= min(count, 20), f"the pool holds {have.size} codewords of classes {keys}: {count} wanted"
    return have[rng.permutation(have.size)][np.arange(count) % have.size]


def decoder(omega, method, minsum_rec, **knobs):
    H, probs, _ = instance(omega)
    dec = bp.bp_decoder(H, max_iter=MAX_ITER, bp_method=method, channel_probs=probs)
    dec.configure(minsum_rec=minsum_rec, **knobs)
    return dec


def run_and_check(dec, omega, method, idx, *, G, compact_after=-1, el_limit=0, soft=False):
    """Decode pool codewords `idx` in one call; results against the oracle's, the schedule against the model's."""
    ref_pool = pool(omega, method, soft)
    _, _, msg = instance(omega)
    cp = np.stack([np.full(R, SOFT_ROWS[i % 2], dtype=np.float32) for i in idx]) if soft else None
    got = dec.decode_batch(msg[idx], early_exit=True, want_llr=True, channel_probs=cp)
    sched, stats = dec.last_schedule(), dec.last_stats()
    ref = {k: v[idx] for k, v in ref_pool.items()}
    T = -(-len(idx) // M.TW)
    G = min(G, T)
    model = M.predict(ref["iters"], ref["converged"], G=G, lanes=2, compact_after=compact_after, max_iter=MAX_ITER,
                      el_limit=el_limit, ring_rows=M.ring_rows_wanted(T, G))
    print(method, "device:", sched, stats, "\nmodel: ", model["counters"], model["levels"], flush=True)
    compare(got, ref, method)
    if method == "min_sum":
        assert sched == model["counters"]
        assert stats == {"compacted": model["compacted"], "row_parallel": model["row_parallel"], "levels": model["levels"]}
    assert sched["open_at_clear"] == 0 and sched["continued"] == sched["left_open"]
    return sched, stats, model


# ---- three levels down --------------------------------------------------------------------------------------------------


def three_level_batch(cls):
    rng = np.random.RandomState(5)
    idx = np.concatenate([take(rng, cls, (1, 2), 244), take(rng, cls, (3, 4), 70), take(rng, cls, (5, 6, 7), 50),
                          take(rng, cls, ("never",), 20)])  # fmt: skip
    return idx[rng.permutation(idx.size)]  # (every class in every tile: the levels gather from and scatter to all of them)


@pytest.mark.parametrize("path,soft", [("stream", False), ("edge", False), ("stream", True)])
@pytest.mark.parametrize("method,minsum_rec", FORMS)
def test_three_levels_down(method, minsum_rec, path, soft):
    """384 codewords in one group of 6 tiles, hand-over point 2: 140 are still running after iteration 2 and go to level 1
    (3 tiles), 70 of those after iteration 4 go to level 2 (2 tiles), 20 after iteration 8 to level 3 -- one tile, on the
    row-parallel kernels under path="edge".  The soft call gives every codeword one of two check-prior rows: a level that
    gathered another codeword's priors would change posterior bits."""
    cls = classes(pool(10, method, soft))
    idx = three_level_batch(cls)
    dec = decoder(10, method, minsum_rec, path=path, compact_after=2)
    sched, stats, model = run_and_check(dec, 10, method, idx, G=6, compact_after=2, el_limit=64 if path == "edge" else 0, soft=soft)
    dec.close()
    assert model["levels"] == 3 and model["counters"]["handed_down"] == [140, 70, 20]  # (the composition does what it says)
    assert stats["levels"] == 3 and sched["handed_down"] == [140, 70, 20] and stats["compacted"] == 140
    assert stats["row_parallel"] == (20 if path == "edge" else 0)
    assert sched["groups"] == ([1, 1, 1, 0] if path == "edge" else [1, 1, 1, 1])
    assert (sched["row_parallel_polls"] > 0) == (path == "edge")


# ---- unseen, chained, re-polled -----------------------------------------------------------------------------------------

STRAGGLER = tuple(range(5, MAX_ITER + 1)) + ("never",)  # more than 4 iterations
QUICK = (1, 2, 3, 4)


def unseen_batch(cls, groups=22, last=70, wrong=None):
    """`groups` groups of 128 codewords (the last one: `last`) with exactly 6 stragglers each, anywhere in the group;
    group `wrong` (counted from 1) holds 128 stragglers instead."""
    rng = np.random.RandomState(9)
    parts = []
    for g in range(groups):
        size = last if g == groups - 1 else 128
        part = np.concatenate([take(rng, cls, STRAGGLER, 6), take(rng, cls, QUICK, size - 6)])
        if wrong is not None and g == wrong - 1:
            part = take(rng, cls, STRAGGLER, size)
        parts.append(part[rng.permutation(size)])
    return np.concatenate(parts)


@pytest.mark.parametrize("method,minsum_rec", FORMS)
def test_unseen_chained_and_repolled(method, minsum_rec):
    """21 groups of 2 tiles and a ragged one of 70 codewords, 6 stragglers each: groups 1 and 2 poll, groups 3 .. 17 stop
    at the hand-over point unseen and are chained lane to lane, group 18 -- the 16th -- polls for real, 19 .. 22 stop
    unseen again."""
    cls = classes(pool(6, method))
    idx = unseen_batch(cls)
    dec = decoder(6, method, minsum_rec, path="stream", split=2)
    dec.set_tile_group(2)
    sched, stats, model = run_and_check(dec, 6, method, idx, G=2)
    dec.close()
    rec0 = model["records"][0]
    assert [r["polls"] for r in rec0[:2]] == [[1, 4], [4]] and rec0[17]["polls"] == [4]
    assert sum(r["stop"][0] == "unseen" for r in rec0) == 19 and sum(r["chain"] & 1 for r in rec0) == 17
    assert sched["unseen"] >= 17 and sched["continued"] >= 14 and sched["polls"] == model["counters"]["polls"]
    assert sched["groups"][0] == 22 and sched["handed_down"][0] == 22 * 6 and sched["clears"] == 0


@pytest.mark.parametrize("method,minsum_rec", FORMS)
def test_a_wrong_guess_changes_no_result(method, minsum_rec):
    """The same batch with 128 stragglers in group 7: nobody looks, the group is stopped unseen like its neighbours, all
    128 go to level 1 -- and every result is the oracle's."""
    cls = classes(pool(6, method))
    idx = unseen_batch(cls, wrong=7)
    dec = decoder(6, method, minsum_rec, path="stream", split=2)
    dec.set_tile_group(2)
    sched, stats, model = run_and_check(dec, 6, method, idx, G=2)
    dec.close()
    assert model["records"][0][6]["stop"] == ("unseen", 4) and model["records"][0][6]["chain"] == 3
    assert sched["handed_down"][0] == 21 * 6 + 128 == stats["compacted"]
    assert sched["unseen"] >= 17 and sched["continued"] >= 14 and sched["polls"] == model["counters"]["polls"]


# ---- across the wrap of the counter ring ------------------------------------------------------------------------------------


@pytest.mark.parametrize("tiles,group", [(1040, 2), (520, 1)])
@pytest.mark.parametrize("method,minsum_rec", FORMS)
def test_across_the_wrap(method, minsum_rec, tiles, group):
    """More groups in one call than the ring of counter rows has rows (512): 21 distinct groups of the unseen batch,
    repeated to 1040 tiles (520 groups of 2; the last holds 70 codewords), and its first 520 tiles less 58 codewords in
    groups of ONE tile.  The ring is cleared again in the middle of the call and no group is left open into the clear;
    the results are the repeated pattern's (the oracle decodes the distinct codewords only).
    About 96 MB in and 480 MB out per call; measured on an MI355X: 0.2 s per min-sum case, 2 s per tanh-rule case."""
    cls = classes(pool(6, method))
    base = unseen_batch(cls, groups=22, last=128)[: 21 * 128]
    reps = -(-1040 * M.TW // base.size)
    idx = np.concatenate([np.tile(base, reps)[: 519 * 128], unseen_batch(cls)[-70:]])
    if tiles == 520:
        idx = idx[: 520 * M.TW - 58]
    assert -(-idx.size // M.TW) == tiles
    dec = decoder(6, method, minsum_rec, path="stream", split=2)
    dec.set_tile_group(group)
    sched, stats, model = run_and_check(dec, 6, method, idx, G=group)
    dec.close()
    assert model["counters"]["clears"] >= 1 and model["counters"]["ring_rows"] == M.REM_SLOTS
    assert sched["ring_rows"] == M.REM_SLOTS and sched["clears"] >= 1 and sched["open_at_clear"] == 0
    assert sched["groups"][0] == tiles // group and sched["ring_takes"] > M.REM_SLOTS
    if group == 2:
        assert sched["unseen"] >= 470 and sched["continued"] >= 400
    else:
        assert sched["continued"] == 0  # (one tile, one lane: nothing to chain)
