"""The reference's own arithmetic on the device: `precision="float64"`, i.e. scaldpc_bp_decode_batch_f64 -- product-sum in
the probability-ratio domain, float64, operation for operation the oracle's method 0.

The bar (tests/ref64_cases.hold_to_bar): bits, iteration counts and converged flags EQUAL the oracle's on every codeword,
settled or not; posteriors with +-inf / NaN in the same places and within 4 ulp of the oracle's value elsewhere (the two
log() implementations' error bounds, doubled).  Stuck trials are the sensitive detector: one ulp of slip in any message shows
in later iterations.  tests/test_ref64.py pins, without a GPU, that the instances are hard enough.  Every test here needs the
entry point, so every one fails on a library without it.
The file also passes with SCALDPC_POISON=1 in the environment (every block handed out 0xFF-filled)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import mc_ref
import ref64_cases as cases
from helpers import compare_with_reference_form, reference_floor
from ref64_cases import equal_bit_for_bit, hold_to_bar, oracle64

pytestmark = pytest.mark.gpu
S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
lib = importlib.import_module("sca-ldpc_amd._lib")
trials = importlib.import_module("sca-ldpc_amd.trials")

KINDS = {0: "syndrome", 1: "received_vector"}


@pytest.fixture(autouse=True)
def own_environment(monkeypatch):
    for v in ("SCALDPC_PATH", "SCALDPC_EL_MAX", "SCALDPC_GROUP_MB", "SCALDPC_PRECISION"):
        monkeypatch.delenv(v, raising=False)


def _decoder(H, probs, max_iter, precision="float64", method="product_sum"):
    with np.errstate(divide="ignore"):
        return bp.bp_decoder(H, max_iter=max_iter, bp_method=method, channel_probs=probs, precision=precision)


def take(r, idx):
    return {k: (v[idx] if v is not None else None) for k, v in r.items()}


# ---------------------------------------------------------------------------------------------------------- 1. F, H1, H2
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("name", ["F", "H1", "H2"])
def test_mc_instances_against_oracle(name, early):
    """130 trials (two tiles and a ragged third), early exit and 30 fixed iterations, at the bar; prefixes of 1, 63, 64 and 65
    codewords give the same rows; tile groups of 1 and 2 give the same bits, llr bit for bit."""
    H, probs, x, kind = cases.mc_case(name)
    ref = cases.mc_oracle(name, early)
    dec = _decoder(H, probs, mc_ref.MAX_ITER)
    got = dec.decode_batch(x, early_exit=early, want_llr=True, input_vector_type=KINDS[kind])
    assert got["llr"].dtype == np.float64
    hold_to_bar(got, ref, f"{name} {'early' if early else 'fixed'}")
    for nb in (1, 63, 64, 65):
        part = dec.decode_batch(x[:nb], early_exit=early, want_llr=True, input_vector_type=KINDS[kind])
        assert equal_bit_for_bit(part, take(got, slice(0, nb))), nb
    for group in (1, 2):
        dec.set_tile_group(group)
        assert equal_bit_for_bit(dec.decode_batch(x, early_exit=early, want_llr=True, input_vector_type=KINDS[kind]), got), group
    dec.set_tile_group(0)
    without = dec.decode_batch(x, early_exit=early, input_vector_type=KINDS[kind])  # no posterior plane asked for
    assert without["llr"] is None and equal_bit_for_bit(without, dict(got, llr=None))
    dec.close()


# ---------------------------------------------------------------------------------------------------------- 2. staircase
@pytest.mark.parametrize("colmax", [32, 64])
def test_staircase_every_degree(colmax):
    """Row degrees 1 .. 64 and column degrees 0 .. colmax in one graph, batch 150."""
    G, probs, synd = cases.staircase_case(colmax)
    dec = _decoder(G, probs, cases.STAIRCASE_ITERS[colmax])
    hold_to_bar(dec.decode_batch(synd, want_llr=True), cases.staircase_oracle(colmax), f"staircase {colmax}")
    dec.close()


# ----------------------------------------------------------------------------------------------------------- 3. wide toy
@pytest.mark.parametrize("early", [True, False])
def test_wide_rows_and_columns(early):
    """Rows of 200 and 65 edges, a column of 70, p = 0 and p = 1 priors: the any-degree loops."""
    G, probs, synd = cases.wide_case()
    ref = cases.wide_oracle(early)
    if early:
        conv = ref["converged"].astype(bool)
        assert len(np.unique(ref["iters"])) >= 2 and conv.any() and (~conv).any()
    dec = _decoder(G, probs, cases.WIDE_ITERS)
    hold_to_bar(dec.decode_batch(synd, early_exit=early, want_llr=True), ref, f"wide toy {'early' if early else 'fixed'}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------- 4. full size
def test_full_size_and_the_fp32_kernels_against_it():
    """hqc128_W50_R2000 (eps = 0: p = 0 check priors), batch 130, 50 iterations, early exit: 16 rows -- stuck ones among them
    -- against the oracle at the bar; then ALL 130 codewords of the same handle's fp32 product_sum decode against the float64
    decode on the device (`helpers.compare_with_reference_form`), on the codewords the float64 run converged on with the fp32
    iteration count."""
    H, probs, msg = cases.full_size_case()
    ref = cases.full_size_oracle()
    dec = _decoder(H, probs, cases.FULL_SIZE_ITERS)
    got = dec.decode_batch(msg, want_llr=True)
    hold_to_bar(take(got, cases.FULL_SIZE_ROWS), ref, "hqc128_W50_R2000")
    f32 = dec.decode_batch(msg, want_llr=True, precision="float32")
    assert f32["llr"].dtype == np.float32
    keep = got["converged"].astype(bool) & (f32["iters"] == got["iters"])
    floor = reference_floor(f32)
    print(f"fp32 against float64 on the device: {int(keep.sum())} of {keep.size} codewords compared (floor {floor:.3f})")
    assert keep.mean() >= floor and keep.sum() > 16
    compare_with_reference_form(take(f32, keep), take(got, keep))
    dec.close()


# ----------------------------------------------------------------------------------------------- 5. per-codeword priors
def test_per_codeword_priors():
    """H1's graph, prob_cols = R: certainties per trial, 0 and 1 among them, against the oracle called once per codeword;
    the same priors for every codeword equal the plain call bit for bit; prob_cols = n."""
    i = mc_ref.instance("H1")
    H, Hin, probs, N, R = i["H"], i["Hin"], i["probs"], i["N"], i["R"]
    nb = 70
    msg, _, cert = trials.hqc_soft_trials(Hin, i["omega"], [1.0, 0.97, 0.85, 0.0], [0.3, 0.4, 0.25, 0.05], nb, base_seed=64)
    cp = 1.0 - cert
    assert (cp == 0.0).any() and (cp == 1.0).any()
    dec = _decoder(H, probs, mc_ref.MAX_ITER)
    got = dec.decode_batch(msg, want_llr=True, channel_probs=cp)
    full = np.concatenate([np.broadcast_to(probs[:N], (nb, N)), cp], axis=1)
    refs = [oracle64(H, full[b], msg[b : b + 1], 1, mc_ref.MAX_ITER, True, threads=1) for b in range(nb)]
    ref = {k: np.concatenate([r[k] for r in refs]) for k in ("bits", "llr", "iters", "converged")}
    assert len(np.unique(ref["iters"])) >= 3 and 0 < ref["converged"].sum() < nb
    hold_to_bar(got, ref, "per-codeword priors, R columns")
    assert equal_bit_for_bit(dec.decode_batch(msg, want_llr=True, channel_probs=full), got)  # prob_cols = n
    fixed = dec.decode_batch(msg, want_llr=True, channel_probs=cp, early_exit=False)
    assert (fixed["iters"] == mc_ref.MAX_ITER).all()
    x = mc_ref.hqc_law("H1")["msg"]
    plain = dec.decode_batch(x, want_llr=True)  # (the decoder's own priors are as they were)
    hold_to_bar(plain, cases.mc_oracle("H1", True))
    for k in (R, H.n):
        rows = np.ascontiguousarray(np.broadcast_to(probs[H.n - k :], (x.shape[0], k)))
        assert equal_bit_for_bit(dec.decode_batch(x, want_llr=True, channel_probs=rows), plain), k
    dec.close()


# ----------------------------------------------------------------------------------------------------------- 6. live handle
def test_live_handle_grown_by_append_rows():
    """H2's graph grown from 40 to 70 rows in steps of 10: after every step the live decoder equals a fresh one bit for bit
    (llr included); at the end it equals the oracle."""
    i = mc_ref.instance("H2")
    H, probs, N = i["H"], i["probs"], i["N"]
    msg = mc_ref.hqc_law("H2")["msg"]

    def part(r):
        g = S.TannerGraph.from_csr(r, N + r, H.row_ptr[: r + 1].copy(), H.col_idx[: H.row_ptr[r]].copy())
        return g, np.concatenate([probs[:N], probs[N : N + r]]), np.ascontiguousarray(msg[:, : N + r])

    g0, p0, x0 = part(40)
    live = _decoder(g0, p0, mc_ref.MAX_ITER)
    live.decode_batch(x0, want_llr=True)  # (its workspace exists before the graph grows)
    for r in (50, 60, 70):
        rp = H.row_ptr[r - 10 : r + 1].astype(np.int64)
        live.append_rows((rp - rp[0]).astype(np.int32), H.col_idx[rp[0] : rp[-1]], N + r, probs[N + r - 10 : N + r])
        g, p, x = part(r)
        got = live.decode_batch(x, want_llr=True)
        fresh = _decoder(g, p, mc_ref.MAX_ITER)
        assert equal_bit_for_bit(got, fresh.decode_batch(x, want_llr=True)), r
        fresh.close()
    hold_to_bar(got, cases.mc_oracle("H2", True), "H2 grown by append_rows")
    live.close()


# ------------------------------------------------------------------------------------------- 7. invisible to what exists
def test_invisible_to_the_fp32_paths_and_follows_new_priors():
    """fp32 product_sum, min-sum, float64, then both again on ONE handle: the fp32 and min-sum results are unchanged bit for
    bit.  update_channel_probs between two float64 calls takes effect."""
    H, probs, x, kind = cases.mc_case("H2")
    L = lib.load()
    dec = _decoder(H, probs, mc_ref.MAX_ITER, precision="float32")
    nb = x.shape[0]

    def min_sum():  # the same handle through the C ABI (a Python decoder has one method)
        out = dict(bits=np.empty((nb, H.n), np.uint8), llr=np.empty((nb, H.n), np.float32), iters=np.empty(nb, np.int32),
                   converged=np.empty(nb, np.uint8))
        rc = L.scaldpc_bp_decode_batch(dec._h, lib.ptr(x), kind, nb, mc_ref.MAX_ITER, lib.BP_MIN_SUM, 1.0, lib.F_EARLY_EXIT, None,
                                       lib.ptr(out["bits"]), lib.ptr(out["llr"]), lib.ptr(out["iters"]), lib.ptr(out["converged"]))
        assert rc == 0
        return out

    def same32(a, b):
        return all(np.array_equal(a[k], b[k]) for k in ("bits", "iters", "converged")) and np.array_equal(
            a["llr"].view(np.uint32), b["llr"].view(np.uint32))

    ps0, ms0 = dec.decode_batch(x, want_llr=True), min_sum()
    assert ps0["llr"].dtype == np.float32
    f64 = dec.decode_batch(x, want_llr=True, precision="float64")
    hold_to_bar(f64, cases.mc_oracle("H2", True))
    assert same32(dec.decode_batch(x, want_llr=True), ps0) and same32(min_sum(), ms0)
    other = np.clip(probs * 1.7, 0.0, 1.0)
    dec.update_channel_probs(other)
    f64b = dec.decode_batch(x, want_llr=True, precision="float64")
    hold_to_bar(f64b, oracle64(H, other, x, kind, mc_ref.MAX_ITER, True, threads=4))
    assert not np.array_equal(f64b["iters"], f64["iters"])  # (26 of the 130 counts move, on the oracle)
    dec.update_channel_probs(probs)
    assert equal_bit_for_bit(dec.decode_batch(x, want_llr=True, precision="float64"), f64)
    assert same32(dec.decode_batch(x, want_llr=True), ps0)
    dec.close()


# ------------------------------------------------------------------------------------------------------- 8. device pointers
@pytest.mark.parametrize("optional", [True, False])
def test_device_pointers_on_the_callers_stream(optional):
    """torch tensors on a stream of the caller's, every output between guard rows; with and without the optional outputs;
    per-codeword priors from device memory too."""
    import torch

    H, probs, x, kind = cases.mc_case("H1")
    nb, n, R = x.shape[0], H.n, H.m
    dec = _decoder(H, probs, mc_ref.MAX_ITER)
    host = dec.decode_batch(x, want_llr=True)
    rows = np.ascontiguousarray(np.broadcast_to(probs[n - R :], (nb, R)))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_in = torch.from_numpy(x).cuda()
        d_cp = torch.from_numpy(rows).cuda()
        d_bits = torch.full((nb + 2, n), 0xA5, dtype=torch.uint8, device="cuda")
        d_llr = torch.full((nb + 2, n), -7.25, dtype=torch.float64, device="cuda")
        d_iters = torch.full((nb + 2,), -9, dtype=torch.int32, device="cuda")
        d_conv = torch.full((nb + 2,), 0x5A, dtype=torch.uint8, device="cuda")
        opt = dict(d_out_llr=d_llr[1:].data_ptr(), d_out_iters=d_iters[1:].data_ptr(), d_out_conv=d_conv[1:].data_ptr()) if optional else {}
        for soft in (False, True):
            d_bits[1 : nb + 1] = 0xA5
            more = dict(d_channel_probs=d_cp.data_ptr(), prob_cols=R) if soft else {}
            dec.decode_batch_device(d_in.data_ptr(), kind, nb, d_bits[1:].data_ptr(), early_exit=True, stream=stream.cuda_stream,
                                    **opt, **more)
            assert np.array_equal(d_bits[1 : nb + 1].cpu().numpy(), host["bits"])
            if optional:
                got = {"bits": d_bits[1 : nb + 1].cpu().numpy(), "llr": d_llr[1 : nb + 1].cpu().numpy(),
                       "iters": d_iters[1 : nb + 1].cpu().numpy(), "converged": d_conv[1 : nb + 1].cpu().numpy()}
                assert equal_bit_for_bit(got, host)
        stream.synchronize()
        for t, fill in ((d_bits, 0xA5), (d_llr, -7.25), (d_iters, -9), (d_conv, 0x5A)):
            assert (t[0] == fill).all() and (t[nb + 1] == fill).all(), "a guard row was written"
            if not optional and t is not d_bits:
                assert (t == fill).all()
        with pytest.raises(ValueError, match="SCALDPC_F_ASYNC"):
            dec.decode_batch_device(d_in.data_ptr(), kind, nb, d_bits[1:].data_ptr(), stream=stream.cuda_stream, asynchronous=True)
    dec.close()


# ------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_write_nothing_and_leave_the_handle_as_before():
    import torch

    H, probs, x, kind = cases.mc_case("H1")
    nb, n, R = x.shape[0], H.n, H.m
    L = lib.load()
    dec = _decoder(H, probs, mc_ref.MAX_ITER)
    good = dec.decode_batch(x, want_llr=True)
    cp = np.ascontiguousarray(np.broadcast_to(probs[n - R :], (nb, R)))
    bits = np.full((nb, n), 0xAB, np.uint8)
    llr = np.full((nb, n), -3.5)
    iters = np.full(nb, -4, np.int32)
    conv = np.full(nb, 0xCD, np.uint8)

    def call(h=dec._h, inp=x, k=kind, batch=nb, p=None, cols=0, flags=lib.F_EARLY_EXIT, out=bits):
        return L.scaldpc_bp_decode_batch_f64(h, lib.ptr(inp), k, batch, lib.ptr(p), cols, mc_ref.MAX_ITER, flags, None,
                                             lib.ptr(out), lib.ptr(llr), lib.ptr(iters), lib.ptr(conv))

    nan, high = cp.copy(), cp.copy()
    nan[17, 5], high[129, R - 1] = np.nan, 1.0 + 2.0**-52
    cases_ = [("NULL handle", dict(h=None)), ("NULL input", dict(inp=None)), ("NULL out_bits", dict(out=None)),
              ("batch 0", dict(batch=0)), ("batch < 0", dict(batch=-3)), ("input kind", dict(k=2)),
              ("prob_cols > n", dict(p=cp, cols=n + 1)), ("probs without prob_cols", dict(p=cp, cols=0)),
              ("prob_cols without probs", dict(cols=R)), ("prob_cols < 0", dict(p=cp, cols=-1)),
              ("NaN probability", dict(p=nan, cols=R)), ("probability > 1", dict(p=high, cols=R)),
              ("async", dict(flags=lib.F_EARLY_EXIT | lib.F_ASYNC)), ("async, device", dict(flags=lib.F_DEVICE_IO | lib.F_ASYNC))]
    for what, kw in cases_:
        assert call(**kw) == lib.EINVAL, what
        assert (bits == 0xAB).all() and (llr == -3.5).all() and (iters == -4).all() and (conv == 0xCD).all(), what
    assert call(p=nan, cols=R) == lib.EINVAL and b"codeword 17, column %d" % (n - R + 5) in L.scaldpc_last_error()
    assert call(p=high, cols=R) == lib.EINVAL and b"codeword 129, column %d" % (n - 1) in L.scaldpc_last_error()
    # a bad probability in DEVICE memory: found by the conversion kernel, refused before the decode starts
    d_in, d_bad = torch.from_numpy(x).cuda(), torch.from_numpy(nan).cuda()
    d_bits = torch.full((nb, n), 0xAB, dtype=torch.uint8, device="cuda")
    d_llr = torch.full((nb, n), -3.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=r"codeword 17, column %d" % (n - R + 5)):
        dec.decode_batch_device(d_in.data_ptr(), kind, nb, d_bits.data_ptr(), early_exit=True, d_out_llr=d_llr.data_ptr(),
                                d_channel_probs=d_bad.data_ptr(), prob_cols=R)
    assert (d_bits == 0xAB).all() and (d_llr == -3.5).all()
    # the Python front end: shapes, and float64 has no min-sum form
    for bad_cp in (cp[: nb - 1], np.zeros((nb, n + 1)), np.zeros((nb, 0))):
        with pytest.raises(ValueError):
            dec.decode_batch(x, channel_probs=bad_cp)
    with pytest.raises(ValueError, match="min-sum"):
        bp.bp_decoder(H, max_iter=5, bp_method="min_sum", channel_probs=probs, precision="float64")
    ms = _decoder(H, probs, 5, precision="float32", method="min_sum")
    with pytest.raises(ValueError, match="min-sum"):
        ms.decode_batch(x, precision="float64")
    ms.close()
    assert equal_bit_for_bit(dec.decode_batch(x, want_llr=True), good)  # the handle as before
    assert equal_bit_for_bit(dec.decode_batch(x, want_llr=True, channel_probs=cp), good)
    dec.close()


# ------------------------------------------------------------------------------------------------------------ 10. lifetime
def test_lifetime_and_allocation_failures():
    """create / float64 decode / close returns every block; with the k-th allocation of the float64 call failing the call
    returns SCALDPC_ENOMEM (MemoryError) and the next call on the same handle succeeds."""
    H, probs, x, kind = cases.mc_case("H2")
    L = lib.load()
    keys = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")
    cp = np.ascontiguousarray(np.broadcast_to(probs[H.n - H.m :], (x.shape[0], H.m)))
    base = lib.live_blocks()
    for _ in range(2):
        dec = _decoder(H, probs, mc_ref.MAX_ITER)
        good = dec.decode_batch(x, want_llr=True, channel_probs=cp)
        dec.close()
        assert all(lib.live_blocks()[k] == base[k] for k in keys)
    assert L.scaldpc_debug_fail_alloc(0) == 0
    failed = succeeded = 0
    try:
        for k in range(1, 40):
            dec = _decoder(H, probs, mc_ref.MAX_ITER)
            assert L.scaldpc_debug_fail_alloc(k) == 0  # (armed: SCALDPC_DEBUG=1, tests/conftest.py)
            try:
                got = dec.decode_batch(x, want_llr=True, channel_probs=cp)
                succeeded += 1
            except MemoryError:
                failed += 1
                L.scaldpc_debug_fail_alloc(0)
                got = dec.decode_batch(x, want_llr=True, channel_probs=cp)  # the handle is usable: the next call succeeds
            L.scaldpc_debug_fail_alloc(0)
            assert equal_bit_for_bit(got, good), k
            dec.close()
            assert all(lib.live_blocks()[k2] == base[k2] for k2 in keys), k
            if succeeded >= 2:
                break
    finally:
        L.scaldpc_debug_fail_alloc(0)
    assert failed >= 8 and succeeded >= 2, (failed, succeeded)  # ratios, planes, both message arrays, posterior, counters, staging


# ------------------------------------------------------------------------------------------------- 11. environment default
def test_environment_default(monkeypatch):
    """SCALDPC_PRECISION=float64 at construction: decode() returns the float64 call's result.  Unset: nothing changes."""
    H, probs, x, kind = cases.mc_case("H1")
    ref = cases.mc_oracle("H1", True)
    plain = _decoder(H, probs, mc_ref.MAX_ITER, precision=None)
    assert plain.precision == "float32"
    b32 = plain.decode(x[3]).copy()
    llr32 = plain.log_prob_ratios.copy()
    monkeypatch.setenv("SCALDPC_PRECISION", "float64")
    dec = _decoder(H, probs, mc_ref.MAX_ITER, precision=None)
    assert dec.precision == "float64" and plain.precision == "float32"  # read once, at construction
    for b in (0, 3, 5):
        out = dec.decode(x[b])
        got = {"bits": out[None].astype(np.uint8), "llr": dec.log_prob_ratios[None], "iters": np.array([dec.iter], np.int32),
               "converged": np.array([dec.converge], np.uint8)}
        hold_to_bar(got, take(ref, slice(b, b + 1)))
    assert np.array_equal(plain.decode(x[3]), b32) and np.array_equal(plain.log_prob_ratios, llr32, equal_nan=True)
    assert np.array_equal(plain.log_prob_ratios.astype(np.float32).astype(np.float64), plain.log_prob_ratios)  # still fp32 values
    monkeypatch.delenv("SCALDPC_PRECISION")
    assert _decoder(H, probs, 5, precision=None).precision == "float32"
    dec.close()
    plain.close()
