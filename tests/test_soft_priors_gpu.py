"""Per-codeword channel priors on the GPU: `BpDecoder.decode_batch(..., channel_probs=[batch, k])`, i.e.
scaldpc_bp_decode_batch_soft -- the priors of the last k columns come with each codeword (hqc.decode()'s `1 - certainty`
per check, simulate/hqc.py:684-699), the columns below keep the decoder's own.

The answer key is the existing oracle called once per codeword with that codeword's full prior vector
(tests/soft_cases.py); values are compared with `helpers.compare` at its existing tolerances: min-sum bit for bit,
posteriors included, the tanh rule at 2e-4 + 2e-4 |L|.  tests/test_soft_priors.py pins, without a GPU, that the samples of
the full-size points are hard enough.  Every test here needs the entry point, so every one fails on a library without it.
The file also passes with SCALDPC_POISON=1 in the environment (every block handed out 0xFF-filled)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import exact
import soft_cases
from helpers import S, compare, hqc_instance, staircase_graph
from soft_cases import oracle_per_codeword, take
from test_exact_inference import large_tree_case
from test_exact_inference_gpu import TOL

pytestmark = pytest.mark.gpu
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")

R4000 = "hqc128_W50_R4000_soft"
METHODS = ["min_sum", "product_sum"]


@pytest.fixture(autouse=True)
def own_schedule(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_MINSUM_REC", "SCALDPC_FIRST_FUSED", "SCALDPC_FUSE_TEST",
              "SCALDPC_COMPACT_AFTER"):
        monkeypatch.delenv(v, raising=False)


def _decoder(H, probs, method, max_iter, **knobs):
    with np.errstate(divide="ignore"):
        dec = bp.bp_decoder(H, max_iter=max_iter, bp_method=method, channel_probs=probs)
    if knobs:
        dec.configure(**knobs)
    return dec


def _same(a, b):
    for k in ("bits", "iters", "converged"):
        assert np.array_equal(a[k], b[k]), k
    if a["llr"] is not None:
        assert np.array_equal(a["llr"], b["llr"], equal_nan=True), "posteriors differ"


# ------------------------------------------------------------------------------------------------ 1. same priors, same answer
def _same_priors_case(graph):
    if graph == "lds":  # E = 3000: the LDS-resident single launch on `auto`
        H, _, probs, msg, _ = hqc_instance(997, 9, 300, 6, 0.03, 130, seed=5)
        return H, probs, msg, "received_vector", 300, 30
    if graph == "tree":
        g, probs, synds, _, _ = large_tree_case(6000, 70, seed=321, hard=6)
        return g, probs, synds, "syndrome", g.m, 40
    H, _, _, _ = soft_cases.soft_graph(R4000)
    msg, _, cp = soft_cases.soft_batch(R4000)
    probs = np.concatenate([soft_cases.shared_priors(R4000)[: H.n - H.m], cp[7].astype(np.float64)])  # p = 0 next to finite ones
    return H, probs, msg, "received_vector", H.m, 50


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("graph,path", [("lds", "auto"), ("lds", "stream"), ("lds", "edge"), ("tree", "auto"), ("tree", "edge"),
                                        ("hqc128", "auto"), ("hqc128", "edge")])
def test_same_priors_same_answer(graph, path, method):
    """A soft call whose every row repeats the decoder's own priors equals the plain call bit for bit: the last m columns
    and all n, fixed iterations and early exit, with posteriors."""
    H, probs, x, kind, k_part, max_iter = _same_priors_case(graph)
    nb = x.shape[0] if path != "edge" else 5
    x = x[:nb]
    dec = _decoder(H, probs, method, max_iter, path=path)
    p32 = probs.astype(np.float32)
    for early in (False, True):
        plain = dec.decode_batch(x, early_exit=early, want_llr=True, input_vector_type=kind)
        for k in (k_part, H.n):
            rows = np.ascontiguousarray(np.broadcast_to(p32[H.n - k :], (nb, k)))
            soft = dec.decode_batch(x, early_exit=early, want_llr=True, input_vector_type=kind, channel_probs=rows)
            _same(soft, plain)
            if path == "edge":
                assert dec.last_stats()["row_parallel"] == nb
    _same(dec.decode_batch(x, early_exit=True, want_llr=True, input_vector_type=kind), plain)  # a plain call afterwards: as before
    if graph == "hqc128" and path == "auto":
        assert dec.time_kernels(2)["launches_check"] > 0  # (shared priors; still works after a soft call)
    dec.close()


# ------------------------------------------------------------------------------------------------ 2. full size against the oracle
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("label", list(soft_cases.SOFT_POINTS))
def test_full_size_against_oracle(label, method):
    """Batch 4096, prob_cols = R, early exit at max_iter 100 and 50 fixed iterations: the oracle sample (first 4 codewords
    of the first, a middle and the last tile).  The early-exit run hands stragglers to the compact pass, so the level's
    plane is gathered; the sample alone goes through the row-parallel kernels as well."""
    H, _, _, _ = soft_cases.soft_graph(label)
    msg, _, cp = soft_cases.soft_batch(label)
    R = H.m
    dec = _decoder(H, soft_cases.shared_priors(label), method, soft_cases.MAX_ITER)
    for early, max_iter in ((True, soft_cases.MAX_ITER), (False, 50)):
        ref = soft_cases.sample_key(label, method, early, max_iter)
        got = dec.decode_batch(msg, max_iter=max_iter, early_exit=early, want_llr=True, channel_probs=cp)
        st = dec.last_stats()
        print(label, method, "early" if early else "fixed", st, "converged %.3f" % got["converged"].mean())
        compare(take(got, soft_cases.SAMPLE), ref, method)
        if early:
            assert st["compacted"] > 0, st
            assert np.array_equal(got["converged"].astype(bool), (H.syndrome(got["bits"]) == 0).all(axis=1))
        dec.configure(path="edge")
        few = dec.decode_batch(msg[soft_cases.SAMPLE], max_iter=max_iter, early_exit=early, want_llr=True,
                               channel_probs=cp[soft_cases.SAMPLE])
        assert dec.last_stats()["row_parallel"] == soft_cases.SAMPLE.size
        compare(few, ref, method)
        dec.configure(path="auto")
    dec.close()
    assert cp.shape == (4096, R)


# ------------------------------------------------------------------------------------------------ 3. every degree
@pytest.mark.parametrize("method", METHODS)
def test_every_degree(oracle, method):
    """Rows of every degree 1 .. 64, columns of every degree 0 .. 32, prob_cols = n, 130 codewords (two tiles and a ragged
    one) with priors of their own on both sides of 1/2 and a few 0 / 1; record and message form, the convergence test
    riding on the check pass and stand-alone.  18 codewords against the oracle, from both full tiles and the ragged one."""
    rng = np.random.RandomState(905)
    G, _ = staircase_graph(rng, rows_per_degree=3, colmax=32, fillers=600)
    batch, max_iter = 130, 10 if method == "min_sum" else 8
    p = np.where(rng.rand(batch, G.n) < 0.85, rng.uniform(0.01, 0.2, (batch, G.n)), rng.uniform(0.55, 0.9, (batch, G.n)))
    hard = rng.rand(batch, G.n) < 0.004
    p[hard] = rng.randint(0, 2, size=int(hard.sum()))
    p = p.astype(np.float32)
    scale = np.array([0.0, 0.03, 0.1, 0.3, 1.0])[np.arange(batch) % 5]
    # errors from each codeword's own likeliest word (scale 0: stops at iteration 1) to draws from its priors (some never stop)
    err = (rng.rand(batch, G.n) < np.where(p < 0.5, p * scale[:, None], 1.0 - (1.0 - p) * scale[:, None])).astype(np.uint8)
    assert not err[p == 0.0].any() and err[p == 1.0].all()  # (syndromes the codeword's own priors allow)
    synd = G.syndrome(err)
    pick = np.r_[0:6, 64:70, 124:130]
    shared = np.full(G.n, 0.3)  # (replaced column by column: must not matter)
    refs = {early: oracle_per_codeword(oracle, G, shared, p[pick], synd[pick], 0, max_iter, method, early_exit=early)
            for early in (True, False)}
    assert len(np.unique(refs[True]["iters"])) > 1
    outs = []
    for rec in ((1, 0) if method == "min_sum" else (0,)):
        for ft in (1, 0):
            dec = _decoder(G, shared, method, max_iter, path="stream", minsum_rec=rec, fuse_test=ft, compact_after=0)
            dec.set_tile_group(2)
            for early in (True, False):
                got = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome", channel_probs=p)
                compare(take(got, pick), refs[early], method)
                outs.append((early, got))
            dec.close()
    for early, got in outs[2:]:  # every form gives the first form's answer on the whole batch
        _same(got, outs[0 if early else 1][1])


@pytest.mark.parametrize("method", METHODS)
def test_wide_rows_and_columns_soft(oracle, method):
    """The graph of test_bp_gpu.test_wide_rows_and_columns (90 x 200: a row of 101 edges and one of 62, a column of 79 and
    one of 42, a degree-1 row, an isolated variable) on the tile kernels, 130 codewords with priors of their own for all
    n columns: the min-sum loop form's first pass, the initialisation pass in front of the tanh rule's any-degree rows,
    and the variable pass at its widest build with any-degree columns -- none of which test_every_degree's 64-edge rows and
    32-edge columns reach.  18 codewords against the oracle; the decoder's own priors in every row equal the plain call."""
    rng = np.random.RandomState(5)
    H = (rng.rand(90, 200) < 0.04).astype(np.int8)
    H[0, :100] = 1  # row of degree >= 100
    H[2, 100:150] = 1  # row of degree ~50
    H[:80, 3] = 1  # column of degree >= 80
    H[:40, 5] = 1  # column of degree ~40
    H[1, :] = 0
    H[1, 7] = 1  # degree-1 row
    H[:, 150] = 0  # isolated variable
    G = S.TannerGraph.from_dense(H)
    deg_r, deg_c = H.sum(axis=1), H.sum(axis=0)
    # any-degree row and column (> 64), the 33 .. 64 register builds, a degree-1 row, an isolated variable
    assert deg_r[0] > 64 and deg_c[3] > 64 and 32 < deg_r[2] <= 64 and 32 < deg_c[5] <= 64 and deg_r[1] == 1 and deg_c[150] == 0
    batch, max_iter = 130, 15
    p = np.where(rng.rand(batch, G.n) < 0.85, rng.uniform(0.01, 0.2, (batch, G.n)), rng.uniform(0.55, 0.9, (batch, G.n)))
    hard = rng.rand(batch, G.n) < 0.004
    p[hard] = rng.randint(0, 2, size=int(hard.sum()))
    p = p.astype(np.float32)
    scale = np.array([0.0, 0.03, 0.1, 0.3, 1.0])[np.arange(batch) % 5]
    err = (rng.rand(batch, G.n) < np.where(p < 0.5, p * scale[:, None], 1.0 - (1.0 - p) * scale[:, None])).astype(np.uint8)
    assert not err[p == 0.0].any() and err[p == 1.0].all()  # (syndromes the codeword's own priors allow)
    synd = G.syndrome(err)
    pick = np.r_[0:6, 64:70, 124:130]
    shared = rng.uniform(0.02, 0.1, size=G.n)
    own = np.ascontiguousarray(np.broadcast_to(shared.astype(np.float32), (batch, G.n)))
    own_synd = G.syndrome((rng.rand(batch, G.n) < 0.03).astype(np.uint8))
    dec = _decoder(G, shared, method, max_iter, path="stream")  # (on `auto` this graph fits LDS)
    for early in (True, False):
        ref = oracle_per_codeword(oracle, G, shared, p[pick], synd[pick], 0, max_iter, method, early_exit=early)
        got = dec.decode_batch(synd, early_exit=early, want_llr=True, input_vector_type="syndrome", channel_probs=p)
        assert dec.last_stats()["row_parallel"] == 0
        compare(take(got, pick), ref, method)
        plain = dec.decode_batch(own_synd, early_exit=early, want_llr=True, input_vector_type="syndrome")
        _same(dec.decode_batch(own_synd, early_exit=early, want_llr=True, input_vector_type="syndrome", channel_probs=own), plain)
    dec.close()


# ------------------------------------------------------------------------------------------------ 4. no decoder in the key
@functools.lru_cache(maxsize=None)
def _tree_case():
    """70 codewords on the 6000-variable tree, each with priors of its own and a syndrome those priors allow, and the exact
    posteriors (both rules) of 16 of them -- 8 from either tile, the first 5 among them -- computed once per session
    (16 eliminations over 6000 variables in Python: about 7 s, paid by whichever of the four cases runs first)."""
    g, _, _, _, _ = large_tree_case(6000, 1, seed=321, hard=6)
    Hd = g.to_dense(np.int8)
    rng = np.random.RandomState(77)
    batch = 70
    p = np.stack([exact.random_priors(rng, g.n, hard=6) for _ in range(batch)]).astype(np.float32)
    e = (rng.rand(batch, g.n) < 0.5).astype(np.uint8)
    e[p == 0.0] = 0
    e[p == 1.0] = 1
    synd = g.syndrome(e)
    pick = np.r_[0:8, 62:70]
    ex = [exact.tree_exact_binary(Hd, p[b].astype(np.float64), synd[b : b + 1]) for b in pick]
    return g, p, synd, pick, {k: np.concatenate([x[k] for x in ex]) for k in ("sp", "ms")}


@pytest.mark.parametrize("path", ["auto", "edge"])
@pytest.mark.parametrize("method", METHODS)
def test_tree_exact_per_codeword(method, path):
    """The 6000-variable tree of `large_tree_case`, priors drawn per codeword (`exact.random_priors`, hard = 6), syndromes
    feasible under each codeword's own priors, against `exact.tree_exact_binary` per codeword -- no decoder in the key --
    at TOL of tests/test_exact_inference_gpu.py: 16 codewords spread over two tiles; 5 on the row-parallel kernels."""
    g, p, synd, pick, ex = _tree_case()
    rtol, atol, key = TOL[method]
    nb = 70 if path == "auto" else 5
    sel = np.arange(pick.size) if path == "auto" else np.arange(5)
    dec = _decoder(g, np.full(g.n, 0.25), method, 150, path=path)
    got = dec.decode_batch(synd[:nb], early_exit=False, want_llr=True, channel_probs=p[:nb])
    assert dec.last_stats()["row_parallel"] == (nb if path == "edge" else 0)
    dec.close()
    worst = exact.check_binary_llr(got["llr"][pick[sel]], got["bits"][pick[sel]], ex[key][sel], rtol, atol, f"{method} {path}")
    print(f"{method} {path}: per-codeword priors on the 6000-variable tree, worst |dL| vs exact = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 5. small calls, 6. equivariance
@pytest.mark.parametrize("method", METHODS)
def test_small_calls_and_equivariance(method):
    """Batches of 1 to 6 on HQC-128 take the row-parallel kernels and agree with the tile result of the same codewords;
    permuting the codewords of a 4096 batch together with their prior rows permutes the outputs."""
    H, _, _, _ = soft_cases.soft_graph(R4000)
    msg, _, cp = soft_cases.soft_batch(R4000)
    max_iter = 30
    dec = _decoder(H, soft_cases.shared_priors(R4000), method, max_iter)
    full = dec.decode_batch(msg, early_exit=True, want_llr=True, channel_probs=cp)
    for nb in range(1, 7):
        idx = np.arange(64 * nb, 64 * nb + nb)
        dec.configure(el_max=6)  # (the tanh rule's default limit is 4)
        few = dec.decode_batch(msg[idx], early_exit=True, want_llr=True, channel_probs=cp[idx])
        assert dec.last_stats()["row_parallel"] == nb
        _same(few, take(full, idx))
    perm = np.random.RandomState(3).permutation(msg.shape[0])
    moved = dec.decode_batch(msg[perm], early_exit=True, want_llr=True, channel_probs=cp[perm])
    _same(moved, take(full, perm))
    dec.close()


# ------------------------------------------------------------------------------------------------ 7. device pointers
@pytest.mark.parametrize("method", METHODS)
def test_device_pointers(method):
    """torch tensors, SCALDPC_F_ASYNC on the caller's stream: equal to the host-array call.  A NaN probability on the
    device path surfaces as ValueError at a synchronising call (an asynchronous call does not look)."""
    import torch

    H, _, _, _ = soft_cases.soft_graph(R4000)
    msg, _, cp = soft_cases.soft_batch(R4000)
    nb, max_iter = 300, 20
    msg, cp = msg[:nb], cp[:nb]
    dec = _decoder(H, soft_cases.shared_priors(R4000), method, max_iter)
    host = dec.decode_batch(msg, early_exit=False, want_llr=True, channel_probs=cp)
    d_in, d_cp = torch.from_numpy(msg).cuda(), torch.from_numpy(cp).cuda()
    d_out = torch.empty((nb, H.n), dtype=torch.uint8, device="cuda")
    d_llr = torch.empty((nb, H.n), dtype=torch.float32, device="cuda")
    d_conv = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d_iters = torch.empty(nb, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = dict(early_exit=False, stream=stream, d_out_llr=d_llr.data_ptr(), d_out_conv=d_conv.data_ptr(),
                d_out_iters=d_iters.data_ptr(), prob_cols=H.m)
    dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, nb, d_out.data_ptr(), asynchronous=True,
                            d_channel_probs=d_cp.data_ptr(), **args)
    torch.cuda.synchronize()
    _same({"bits": d_out.cpu().numpy(), "llr": d_llr.cpu().numpy(), "iters": d_iters.cpu().numpy(), "converged": d_conv.cpu().numpy()}, host)
    bad = d_cp.clone()
    bad[123, 45] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=r"codeword 123, column %d" % (H.n - H.m + 45)):
        dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, nb, d_out.data_ptr(), d_channel_probs=bad.data_ptr(), **args)
    dec.decode_batch_device(d_in.data_ptr(), lib.IN_RECEIVED, nb, d_out.data_ptr(), d_channel_probs=d_cp.data_ptr(), **args)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), host["bits"])  # the handle is as usable as before
    dec.close()


# ------------------------------------------------------------------------------------------------ 8. live handle
@pytest.mark.parametrize("method", METHODS)
def test_live_handle_after_append_rows(oracle, method):
    """W50 grown from 1900 to 2100 rows on a live decoder: a soft call with prob_cols = the current R equals a fresh
    decoder's soft call and the oracle -- 70 codewords on the tile kernels, 3 on the row-parallel ones."""
    from helpers import PRODUCTION_GROWTH, growth_run, prefix_point

    g = PRODUCTION_GROWTH["W50_across_16"]
    Hin, probs, msg = growth_run("W50_across_16", 70)
    N, R0, R1 = Hin.n, g["R0"], g["R1"]
    rng = np.random.RandomState(8)
    cert = np.array([1.0, 0.95, 0.8])[rng.choice(3, (70, R1), p=[0.5, 0.3, 0.2])]
    msg = msg.copy()
    msg[:, N:] ^= (rng.rand(70, R1) < 1.0 - cert).astype(np.uint8)
    cp = (1.0 - cert).astype(np.float32)
    H0, p0, _ = prefix_point(Hin, probs, msg, R0)
    H1, p1, x1 = prefix_point(Hin, probs, msg, R1)
    max_iter = 30
    ref = oracle_per_codeword(oracle, H1, p1, cp[:6], x1[:6], 1, max_iter, method)
    for path, nb in (("stream", 70), ("edge", 3)):
        live = _decoder(H0, p0, method, max_iter, path=path)
        live.decode_batch(msg[:nb, : N + R0], channel_probs=cp[:nb, :R0])  # (its tables exist before the graph grows)
        rp = Hin.row_ptr[R0 : R1 + 1].astype(np.int64)
        cols = np.concatenate([Hin.col_idx[rp[0] : rp[-1]].reshape(R1 - R0, -1), N + np.arange(R0, R1, dtype=np.int32)[:, None]], axis=1)
        with np.errstate(divide="ignore"):
            live.append_rows(np.arange(R1 - R0 + 1, dtype=np.int32) * cols.shape[1], cols.reshape(-1), N + R1, p1[N + R0 :])
        got = live.decode_batch(x1[:nb], want_llr=True, channel_probs=cp[:nb])
        fresh = _decoder(H1, p1, method, max_iter, path=path)
        _same(got, fresh.decode_batch(x1[:nb], want_llr=True, channel_probs=cp[:nb]))
        compare(take(got, np.arange(min(nb, 6))), take(ref, np.arange(min(nb, 6))), method)
        live.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ 9. errors and lifetime
def test_errors_leave_the_handle_usable_and_nothing_leaks():
    H, _, probs, msg, _ = hqc_instance(1201, 9, 420, 6, 0.03, 70, seed=9)
    L = lib.load()
    base = lib.live_blocks()
    for cycle in range(3):
        dec = _decoder(H, probs, "min_sum", 20, path="stream")
        cp = np.ascontiguousarray(np.broadcast_to(probs[-420:].astype(np.float32), (70, 420)))
        good = dec.decode_batch(msg, want_llr=True, channel_probs=cp)
        with pytest.raises(ValueError):
            dec.decode_batch(msg, channel_probs=cp[:69])  # wrong batch dimension
        with pytest.raises(ValueError):
            dec.decode_batch(msg, channel_probs=np.zeros((70, H.n + 1), dtype=np.float32))  # k > n
        with pytest.raises(ValueError):
            dec.decode_batch(msg, channel_probs=np.zeros((70, 0), dtype=np.float32))  # k = 0
        bits = np.empty((70, H.n), dtype=np.uint8)
        for probs_ptr, cols in ((lib.ptr(cp), 0), (lib.ptr(cp), H.n + 1), (None, 420)):  # the C ABI itself: bad prob_cols, NULL
            rc = L.scaldpc_bp_decode_batch_soft(dec._h, lib.ptr(msg), lib.IN_RECEIVED, 70, probs_ptr, cols, 20, lib.BP_MIN_SUM,
                                                C.c_float(1.0), lib.F_EARLY_EXIT, None, lib.ptr(bits), None, None, None)
            assert rc == lib.EINVAL, (rc, cols)
        worse = cp.copy()
        worse[17, 5] = 1.5
        with pytest.raises(ValueError, match=r"codeword 17, column %d" % (H.n - 420 + 5)):
            dec.decode_batch(msg, channel_probs=worse)
        _same(dec.decode_batch(msg, want_llr=True, channel_probs=cp), good)  # still usable
        _same(dec.decode_batch(msg, want_llr=True), good)  # ... and its own priors untouched: the plain call
        dec.close()
        end = lib.live_blocks()
        assert all(end[k] == base[k] for k in ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")), (cycle, base, end)
