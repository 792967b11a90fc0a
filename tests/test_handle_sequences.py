"""The committed call sequences of tests/handle_sequence_cases.py, without a GPU: replayed against the oracle-backed double
(tests/fakes.OracleLiveBp), they must keep the model's books right, decide something, and contain every transition the GPU
file (tests/test_handle_sequences_gpu.py) claims to hold -- each in at least three sequences.  The coverage conditions are
computed from the op lists and the model alone."""
import functools
import os
import re
from collections import Counter

import numpy as np
import pytest

import handle_sequence_cases as C
import settle_ref
from fakes import OracleLiveBp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the thresholds the families are built on ---------------------------------------------------------------------------------
def test_thresholds_are_the_librarys():
    """The model's restatement of small_lds, el_limit and rec_form reads the numbers the library's source states."""
    src = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_bp.hip")).read()
    assert "return (size_t)2 * h->E * sizeof(float) + (size_t)2 * h->n + h->m + 64;" in src  # small_lds_bytes
    assert re.search(r"fits = h->E > 0 && lds <= 60 \* 1024;", src) and C.LDS_LIMIT == 60 * 1024
    assert "int lim = method == SCALDPC_BP_MIN_SUM ? 6 : 4;" in src and C.EL_DEFAULT == {"min_sum": 6, "product_sum": 4}
    assert "const int col_cap = h->kn.minsum_rec == 2 ? 64 : 32;" in src and C.REC_COLS == {0: 0, 1: 32, 2: 64}
    assert "int settle = -1;" in src and "int minsum_rec = 1;" in src and "int first_fused = 1;" in src  # the defaults the model starts from


@pytest.mark.parametrize("family,seed", C.SEQUENCES)
def test_graph_families_sit_where_they_claim(family, seed):
    m = C.Model(family, seed)
    need = C.small_lds_bytes(m.E, m.n, m.m)
    deg = m.col_degrees()
    assert m.max_row() <= 64 and all(r[-1] == m.N + i for i, r in enumerate(m.rows))  # [Hin | I]
    if family == "C":
        assert need <= C.LDS_LIMIT and m.path_of(130, "min_sum", "float32") == "lds"
        return
    # just too large: the same graph with a tenth of its rows fewer would fit
    assert C.LDS_LIMIT < need < 1.1 * C.LDS_LIMIT and m.path_of(130, "min_sum", "float32") == "tile"
    assert m.path_of(6, "min_sum", "float32") == "edge" and m.path_of(7, "min_sum", "float32") == "tile"
    assert m.path_of(4, "product_sum", "float32") == "edge" and m.path_of(5, "product_sum", "float32") == "tile"
    if family == "A":
        assert deg.max() <= 16 and m.rec_form("min_sum")
    else:
        assert 1 <= len(m.heavy) <= 3 and all(30 <= deg[c] <= 48 for c in m.heavy) and np.delete(deg, m.heavy).max() <= 16
        forms = []
        for v in (0, 1, 2):
            m.knobs["minsum_rec"] = v
            forms.append(m.rec_form("min_sum"))
        assert forms == [False, bool(deg.max() <= 32), True]


# ---- the replay against the double -----------------------------------------------------------------------------------------------
def _books(step, model, dec):
    """After an append or a prior update: what the model hands to the oracle is what a double built from scratch holds, and
    what the live double has put together from the calls."""
    g = model.graph()
    scratch = OracleLiveBp(g, model.probs, {})
    for d in (scratch, dec):
        assert (d.m, d.n) == (model.m, model.n) == (g.m, g.n)
        assert np.array_equal(d.row_ptr, g.row_ptr) and np.array_equal(d.col_idx, g.col_idx)
        assert np.array_equal(d.probs, model.probs) and model.probs.shape == (model.n,)
    assert all((np.diff(r) > 0).all() and r[-1] == model.N + i for i, r in enumerate(model.rows))
    assert ((model.probs >= 0) & (model.probs <= 1)).all()


@functools.lru_cache(maxsize=None)
def records(family, seed):
    ops = C.sequence(family, seed)
    assert ops == C.sequence(family, seed) and C.MIN_OPS <= len(ops) - 1 <= C.MAX_OPS  # deterministic, 10 to 16 operations
    assert all(isinstance(op, tuple) for op in ops) and eval(repr(ops)) == ops  # plain tuples: printable, replayable
    return C.replay(ops, OracleLiveBp, on_state=_books)


@pytest.mark.parametrize("family,seed", C.SEQUENCES)
def test_replay_keeps_the_books(family, seed):
    recs = records(family, seed)
    assert len(recs) == len(C.sequence(family, seed))
    for r in recs:
        if r["kind"] == "decode":
            a, got = r["args"], r["got"]
            assert a["x"].dtype == np.uint8 and a["x"].shape[0] == r["batch"]
            assert a["cp"] is None or (a["cp"].dtype == np.float32 and a["cp"].shape[0] == r["batch"] and (a["cp"] == 0).any())
            assert got["bits"].shape == (r["batch"], a["x"].shape[1] if a["kind"] == "received" else got["bits"].shape[1])
            if not r["early"]:
                assert (got["iters"] == r["max_iter"]).all()


def test_the_set_is_about_forty_sequences_over_three_families():
    assert 36 <= len(C.SEQUENCES) <= 44 and {f for f, _ in C.SEQUENCES} == set(C.FAMILIES)


def test_a_failure_names_family_seed_step_and_the_prefix_that_reproduces_it():
    ops = C.sequence("C", 1)
    first = next(i for i, op in enumerate(ops) if op[0] == "decode")

    def failing(step, model, args, got, dec):
        assert step != first, "planted"

    with pytest.raises(C.SequenceFailure) as e:
        C.replay(ops, OracleLiveBp, on_decode=failing)
    text = str(e.value)
    assert f"family C seed 1: step {first}" in text and "planted" in text
    prefix = eval(text.split("ops = ", 1)[1])
    assert prefix == list(ops[: first + 1])
    with pytest.raises(C.SequenceFailure, match=f"step {first}"):
        C.replay(prefix, OracleLiveBp, on_decode=failing)


# ---- the sequences decide something --------------------------------------------------------------------------------------------
def _all_decodes():
    return [r for f, s in C.SEQUENCES for r in records(f, s) if r["kind"] == "decode"]


def test_decodes_converge_at_once_later_and_never():
    first = later = never = 0
    for r in _all_decodes():
        if r["early"]:
            conv, it = r["got"]["converged"].astype(bool), r["got"]["iters"]
            first += int((conv & (it == 1)).sum())
            later += int((conv & (it > 1)).sum())
            never += int((~conv).sum())
    assert first > 100 and later > 100 and never > 100, (first, later, never)
    for f, s in C.SEQUENCES:  # and the sweeps: both outcomes, more than one iteration count
        for r in records(f, s):
            if r["kind"] == "sweep":
                assert r["got"]["success"].shape == (C.SWEEP_RUNS,) and r["got"]["iters"].shape == (C.SWEEP_RUNS,)
    sweeps = [r["got"] for f, s in C.SEQUENCES for r in records(f, s) if r["kind"] == "sweep"]
    assert any(len(set(g["success"].tolist())) == 2 for g in sweeps) and any(len(set(g["iters"].tolist())) > 2 for g in sweeps)


def _frozen(r, model_graph, probs):
    a = r["args"]
    synd = a["x"] if a["kind"] == "syndrome" else model_graph.syndrome(a["x"])
    prior = settle_ref.prior_llr(probs if a["cp"] is None else C.full_priors(probs, a["cp"]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = settle_ref.run(model_graph, prior, synd, r["max_iter"], r["alpha"])
    first = settle_ref.first_test(r["alpha"], r["max_iter"])
    return settle_ref.frozen_at(out["same"], first, r["max_iter"], batch=r["batch"]), first


def test_tracked_decodes_hold_tiles_that_freeze_and_tiles_that_do_not():
    """settle_ref on fixed-iteration record-form decodes of families A and B: over them there are tiles that freeze and tiles
    that never do; learning calls after which a horizon IS learned (every tile frozen, 2 (latest + 2) < max_iter:
    settle_next_horizon), so the next call runs under it and saves launches; and calls under a forced horizon that is too
    short for a tile, which is then decoded again (collect_settle)."""
    froze = stayed = learned = rerun = 0
    for f, s in C.SEQUENCES:
        if f == "C" or learned >= 3 and rerun >= 2 and froze and stayed:
            continue
        ops = C.sequence(f, s)
        recs = records(f, s)
        for i, r in enumerate(recs):
            if r["kind"] != "decode" or not r["tracked"] or not (r["learn"] or r["forced"]):
                continue
            model = _model_at(ops, i)
            at, first = _frozen(r, model.graph(), model.probs)
            froze += sum(1 for t in at if t)
            stayed += sum(1 for t in at if not t)
            if r["learn"] and all(at) and 2 * (max(at) + 2) < r["max_iter"]:
                learned += 1
            K = r["forced"]
            if K and K >= first and K + 1 < r["max_iter"] and any(t == 0 or t > K for t in at):
                rerun += 1
    assert froze > 0 and stayed > 0 and learned >= 3 and rerun >= 2, (froze, stayed, learned, rerun)


def _model_at(ops, step):
    """The model as it stands when op `step` runs."""
    model = C.Model(ops[0][1], ops[0][2])
    for op in ops[1:step]:
        if op[0] == "configure":
            model.configure(op[1])
        elif op[0] == "update_probs":
            model.probs = model.new_probs(op[1])
        elif op[0] == "append":
            _, _, _, tail, rows = model.new_rows(*op[1:])
            model.append(rows, tail)
    return model


# ---- coverage: conditions on the op lists and the model ---------------------------------------------------------------------------
CONDITIONS = (
    "record form, tanh, record form", "first_fused, update, decode", "first_fused: two alphas", "first_fused: two methods",
    "learn, same key", "learn, other max_iter", "learn, other alpha", "learn, then soft", "learn, append", "learn, update",
    "learn, tile group", "minsum_rec 0 1 2 on B", "two appends, tile decode", "two appends, row-parallel decode", "32 -> 33 under 2",
    "64 -> 65 under 2", "1 tile, 3 tiles, 1 tile", "max_iter grows", "float64 between fp32", "float64 after update",
    "sweep after update", "sweep after append", "compaction, then smaller", "compaction, then larger",
    "async, host calls, append", "refused, decode", "probe between equal decodes", "forced horizon too short",
    "time_kernels after record form", "time_kernels after message form", "row-parallel decode", "lds decode", "stale tables on lds",
)


def coverage(recs):
    hit = set()
    idx = [i for i, r in enumerate(recs) if r["kind"] == "decode"]
    D = [recs[i] for i in idx]
    between = lambda a, b: recs[idx[a] + 1 : idx[b]]
    quiet = lambda mid: all(r["kind"] == "probe" for r in mid)
    for a in range(len(D) - 1):
        p, q, mid = D[a], D[a + 1], between(a, a + 1)
        kinds = [r["kind"] for r in mid]
        if a + 2 < len(D):
            r3 = D[a + 2]
            if p["rec"] and not p["early"] and q["method"] == "product_sum" and q["precision"] == "float32" and q["path"] == "tile" and r3["rec"]:
                hit.add("record form, tanh, record form")
            if all(d["path"] == "tile" for d in (p, q, r3)) and (p["T"], q["T"], r3["T"]) == (1, 3, 1):
                hit.add("1 tile, 3 tiles, 1 tile")
            if (p["precision"], q["precision"], r3["precision"]) == ("float32", "float64", "float32"):
                hit.add("float64 between fp32")
            if all(d["path"] in ("tile", "edge") for d in (p, q, r3)) and p["max_iter"] < q["max_iter"] < r3["max_iter"]:
                hit.add("max_iter grows")
        if p["ff"] and q["ff"]:
            if "update_probs" in kinds and p["method"] == q["method"] and p["alpha1"] == q["alpha1"]:
                hit.add("first_fused, update, decode")
            if quiet(mid) and p["method"] == q["method"] == "min_sum" and p["alpha1"] != q["alpha1"]:
                hit.add("first_fused: two alphas")
            if quiet(mid) and p["method"] != q["method"]:
                hit.add("first_fused: two methods")
        if p["learn"] and q["settle2"]:
            same = p["key"] == q["key"]
            if same and quiet(mid):
                hit.add("learn, same key")
            if quiet(mid) and p["key"][0] != q["key"][0] and p["key"][1:] == q["key"][1:]:
                hit.add("learn, other max_iter")
            if quiet(mid) and p["key"][1] != q["key"][1] and p["key"][0] == q["key"][0] and p["key"][2] == q["key"][2]:
                hit.add("learn, other alpha")
            if quiet(mid) and q["key"][2] and not p["key"][2] and p["key"][:2] == q["key"][:2]:
                hit.add("learn, then soft")
            if same and kinds == ["append"]:
                hit.add("learn, append")
            if same and kinds == ["update_probs"]:
                hit.add("learn, update")
            if same and kinds == ["configure"] and [k for k, _ in mid[0]["op"][1]] == ["tile_group"]:
                hit.add("learn, tile group")
        if kinds[-2:] == ["append", "append"]:
            hit.add({"tile": "two appends, tile decode", "edge": "two appends, row-parallel decode",
                     "lds": "stale tables on lds"}.get(q["path"], "two appends, float64"))
        if (p["precision"], q["precision"]) == ("float64", "float64") and kinds == ["update_probs"]:
            hit.add("float64 after update")
        if p["compacts"] and quiet(mid) and q["path"] in ("tile", "edge") and q["batch"] != p["batch"]:
            hit.add("compaction, then smaller" if q["batch"] < p["batch"] else "compaction, then larger")
        if quiet(mid) and kinds and p["op"] == q["op"]:
            hit.add("probe between equal decodes")
    for a, p in enumerate(D):
        later = recs[idx[a] + 1 :]
        if p["io"] == "async":
            k = [r["kind"] if r["kind"] != "decode" else "decode:" + r["io"] for r in later]
            if "decode:host" in k and "append" in k[k.index("decode:host") :] and "decode:host" in k[k.index("append") :]:
                hit.add("async, host calls, append")
        if p["forced"] and p["mix"] == "hard" and p["forced"] + 1 < p["max_iter"]:
            hit.add("forced horizon too short")
        if p["path"] == "edge":
            hit.add("row-parallel decode")
        if p["path"] == "lds":
            hit.add("lds decode")
        if later and later[0]["kind"] == "probe" and later[0]["timed"]:
            hit.add("time_kernels after record form" if p["rec"] else "time_kernels after message form")
    if D and D[0]["family"] == "B" and {d["minsum_rec"] for d in D if d["path"] == "tile" and d["method"] == "min_sum"} == {0, 1, 2}:
        hit.add("minsum_rec 0 1 2 on B")
    for i, r in enumerate(recs):
        if r["kind"] == "append" and r["minsum_rec"] == 2:
            if (32, 33) in r["crossings"] or any(a <= 32 < b for a, b in r["crossings"]):
                hit.add("32 -> 33 under 2")
            if any(a <= 64 < b for a, b in r["crossings"]):
                hit.add("64 -> 65 under 2")
        if r["kind"] == "refused" and i + 1 < len(recs) and recs[i + 1]["kind"] == "decode":
            hit.add("refused, decode")
        if r["kind"] == "sweep":
            before = recs[:i]
            prev = [j for j, b in enumerate(before) if b["kind"] == "sweep" and b["sweep"] == r["sweep"]]
            if prev:
                mid = [b["kind"] for b in before[prev[-1] + 1 :]]
                if mid == ["update_probs"]:
                    hit.add("sweep after update")
                if mid == ["append"]:
                    hit.add("sweep after append")
    return hit


def test_every_transition_occurs_in_at_least_three_sequences():
    count = Counter()
    for f, s in C.SEQUENCES:
        count.update(coverage(C.replay(C.sequence(f, s))))  # (the model alone: no decoder)
    print({k: count[k] for k in CONDITIONS})
    short = {k: count[k] for k in CONDITIONS if count[k] < 3}
    assert not short, f"transitions in fewer than three sequences: {short}"
    # the two methods' sweeps: a thresholds table (mc_fer_run) and an [Hin | I] sweep in each family
    for f in C.FAMILIES:
        kinds = {op[1] for s in C.SEQUENCE_SEEDS[f] for op in C.sequence(f, s) if op[0] == "sweep"}
        assert kinds == {"fer", "hqc"}, (f, kinds)
