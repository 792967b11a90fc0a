"""Soft output of the q-ary decoders on the GPU (scaldpc_qary_min_sum_batch_soft / _special_min_sum_batch_soft): the last
variable update's totals, the margins and the unmet-check counts, BIT FOR BIT against the NumPy float32 restatement of the
whole loop (tests/qary_soft_ref.py, held to the oracle and to exact inference by tests/test_qary_soft.py), in every form
of the variable kernel; then what no reference is needed for: the forms agree with each other, the outputs agree with the
plain call and with their own definitions, the transposing copy stays inside its arrays, device pointers, errors, lifetime."""
import ctypes as C
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest

import qary_soft_ref as ref
from helpers import S
from oracle import pyoracle
from test_exact_inference import qary_tree_case, special_tree_case

pytestmark = pytest.mark.gpu
qary = importlib.import_module("sca-ldpc_amd.qary")
lib = importlib.import_module("sca-ldpc_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("symbols", "costs", "costs_sum", "margins", "unmet")
SPECIAL_FORMS = (("dp", dict(wave=-1, tree=1, dp=1, dp_min=1, dp_split=0, dp_split2=0)),
                 ("dp halves", dict(wave=-1, tree=1, dp=1, dp_min=1, dp_split=0, dp_split2=1 << 20)),
                 ("dp quarters", dict(wave=-1, tree=1, dp=1, dp_min=1, dp_split=1 << 20)), ("tree", dict(wave=-1, tree=1, dp=0)),
                 ("generic", dict(wave=1, tree=0, dp=0)), ("lane", dict(wave=0, tree=0, dp=0)))
PLAIN_FORMS = (("dp", dict(wave=-1, unroll=1, dp=1)), ("unrolled", dict(wave=-1, unroll=1, dp=0)), ("wave", dict(wave=1, unroll=0, dp=0)),
               ("lane", dict(wave=0, unroll=0, dp=0)))


def same(got, want, rows=None, what=""):
    """Every output present on both sides equal: floats as bit patterns (NaN = NaN), integers exactly."""
    for k in KEYS:
        if k not in want:
            assert k not in got, (what, k)
            continue
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k])
        if a.dtype == np.float32:
            assert ref.same_bits(a, b), (what, k, np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5])
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), (what, k)


def plain_decoder(H, B, iterations):
    nz = H != 0
    return qary.decoder_class(f"DecoderN{H.shape[1]}R{H.shape[0]}V{max(1, nz.sum(axis=0).max())}C{nz.sum(axis=1).max()}B{B}")(H, iterations)


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", "generators.json")) as fh:
        return S.TannerGraph.from_coo(json.load(fh)[name])


def config4_pmf(batch, seed=40):
    """Config 4's channel outputs (decode.py:232-237): codewords with 0.5 % and with 8 % unlikely rows, in turn."""
    rng = np.random.RandomState(seed)
    p = 1 / 3
    good, bad = np.array([p, 1.75 * p, 0.25 * p]), np.array([p, 0.25 * p, 1.75 * p])
    rate = np.where(np.arange(batch) % 2 == 0, 0.005, 0.08)
    return np.where((rng.rand(batch, 450) < rate[:, None])[:, :, None], bad, good).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the instances and their references
@functools.lru_cache(maxsize=None)
def plain_case(name):
    """(H, B, pmf [70, N, Q], iterations, restatement on all 70 codewords) -- computed once, shared, never modified."""
    if name == "q15":
        H, B, pmf = ref.q15_instance(70)
        it = 3
    elif name == "tree_b1":
        H, pmf, _ = qary_tree_case(3, 1, batch=70)
        B, it = 1, H.shape[0] + 1
    elif name == "tree_b2":
        H, pmf, _ = qary_tree_case(1, 2, batch=70)
        B, it = 2, H.shape[0] + 1
    elif name == "cycles_q3":
        H, B, pmf = ref.cyclic_instance(1, 70, seed=3)
        it = 3
    elif name == "cycles_q7":  # four possible symbols per variable: enumerations of 4^3
        H, B, pmf = ref.cyclic_instance(3, 70, seed=7, R=5, N=10)
        rng = np.random.RandomState(70)
        for v in range(H.shape[1]):
            pmf[:, v, rng.choice(7, 3, replace=False)] = 0.0
        pmf = (pmf / pmf.sum(axis=2, keepdims=True)).astype(np.float32)
        it = 2
    elif name == "degree5":  # variable 0 sits in five checks: beyond the register kernels' four
        H = np.zeros((5, 11), dtype=np.int8)
        for r in range(5):
            H[r, [0, 1 + 2 * r, 2 + 2 * r]] = [1, -1, 1] if r % 2 else [-1, 1, 1]
        B, it = 1, 3
        pmf = np.random.RandomState(55).dirichlet(np.ones(3) * 1.3, size=(70, 11)).astype(np.float32)
    elif name == "isolated":  # variable 4 sits in no check
        H, B, pmf = ref.cyclic_instance(2, 70, seed=11, R=4, N=9)
        H[:, 4] = 0
        it = 2
    with np.errstate(divide="ignore"):
        want = ref.min_sum_soft(pyoracle, H, B, pmf, it)
    for v in want.values():
        v.setflags(write=False)
    return H, B, pmf, it, want


PLAIN_CASES = ("q15", "tree_b1", "tree_b2", "cycles_q3", "cycles_q7", "degree5", "isolated")


@pytest.mark.parametrize("generic", [False, True], ids=["var_small", "k_q_var"])
@pytest.mark.parametrize("name", PLAIN_CASES)
def test_bit_exact_against_the_restatement(name, generic):
    """Q = 15 (the 6 x 3 instance), 3, 5 (trees), 3, 7 (cycles) through k_q_var_small<Q, 4>, the same through the generic k_q_var
    (var_small = 0, llr_tiled = 0), a column of degree 5 and a variable without checks (generic kernel either way), at batch 1
    and 70: symbols, totals, margins, unmet counts equal the restatement's on every codeword."""
    H, B, pmf, it, want = plain_case(name)
    dec = plain_decoder(H, B, it)
    if generic:
        dec.configure(var_small=0, llr_tiled=0)
    with np.errstate(divide="ignore"):
        same(dec.min_sum_soft_batch(pmf), want, what=name)
        one = dec.min_sum_soft_batch(pmf[:1])
    same(one, {k: v[:1] for k, v in want.items()}, what=name + " batch 1")
    if name == "isolated":  # nothing comes in: the total IS the channel LLR, the margin its second smallest entry
        with np.errstate(divide="ignore"):
            llr = np.stack([pyoracle.qary_into_llr(p[4:5])[0] for p in pmf])
        assert ref.same_bits(want["costs"][:, 4], llr) and ref.same_bits(dec.min_sum_soft_batch(pmf)["costs"][:, 4], llr)
    if name == "q15":
        assert dec.min_sum_soft(pmf[0])["symbols"] == [0] * 6  # decoder.rs:771-799
    dec.close()


def test_zero_iterations_behave_as_one():
    H, B, pmf, _, _ = plain_case("cycles_q3")
    d0, d1 = plain_decoder(H, B, 0), plain_decoder(H, B, 1)
    with np.errstate(divide="ignore"):
        got = d0.min_sum_soft_batch(pmf)
        same(got, d1.min_sum_soft_batch(pmf))
        same(got, ref.min_sum_soft(pyoracle, H, B, pmf[:2], 0), rows=slice(0, 2))
    d0.close(), d1.close()


@functools.lru_cache(maxsize=None)
def special_case(name):
    """(H, B, BSUM, pmf_b, pmf_s, iterations, compared codewords, restatement on those)."""
    if name == "tree":  # B = 2, BSUM = 12: k_q_var_small_special<5, 4, 25>
        H, pb, ps, _ = special_tree_case(0, batch=70)
        B, BSUM, it, rows = 2, 12, H.shape[0] + 1, np.arange(0, 70, 7)
    elif name == "wide":  # BSUM = 14: the row-sum alphabet has 29 symbols -> generic kernel, two alphabets
        rng = np.random.RandomState(303)
        R, NB, B, BSUM = 10, 36, 2, 14
        Hp = np.zeros((R, NB), dtype=np.int8)
        for r in range(R):
            k = 6 if r % 4 else rng.randint(3, 6)
            Hp[r, rng.choice(NB, k, replace=False)] = rng.choice([-1, 1], size=k)
        H = np.concatenate([Hp, np.eye(R, dtype=np.int8)], axis=1)
        pb = rng.dirichlet(np.ones(5) * 0.7, size=(70, NB)).astype(np.float32)
        ps = rng.dirichlet(np.ones(2 * BSUM + 1) * 0.7, size=(70, R)).astype(np.float32)
        zs = rng.rand(70, R, 2 * BSUM + 1) < 0.1
        zs[..., BSUM] = False
        ps[zs] = 0.0
        ps = (ps / ps.sum(axis=2, keepdims=True)).astype(np.float32)
        it, rows = 3, np.array([0, 1, 69])
    elif name == "kyber":  # DecoderN1280R512SW6 on the graph of test_kyber_shape_sample
        H = golden("qary_qc_256_6_3_s0_cb2").to_dense(np.int8)
        r2 = np.random.RandomState(10)
        pb = r2.dirichlet(np.ones(5), size=(70, 768)).astype(np.float32)
        ps = r2.dirichlet(np.ones(25), size=(70, 512)).astype(np.float32)
        B, BSUM, it, rows = 2, 12, 2, np.array([0, 69])
    with np.errstate(divide="ignore", invalid="ignore"):
        want = ref.special_min_sum_soft(pyoracle, H, B, BSUM, pb[rows], ps[rows], it)
    for v in want.values():
        v.setflags(write=False)
    return H, B, BSUM, pb, ps, it, rows, want


def special_decoder(H, B, BSUM, iterations):
    R, N = H.shape
    base = qary.decoder_class(f"DecoderN{N}R{R}SW6")
    cls = base if BSUM == base.BSUM else type("DecoderSpecialWideSum", (base,), dict(BSUM=BSUM, QS=2 * BSUM + 1))
    return cls(H, iterations)


@pytest.mark.parametrize("name", ["tree", "wide", "kyber"])
def test_special_decoder_bit_exact_against_the_restatement(name):
    """DecoderSpecial: the Kyber alphabets on a tree (k_q_var_small_special<5, 4, 25>), a wider row-sum alphabet (generic
    kernel, mixed alphabets), and the Kyber N1280R512SW6 graph itself at batch 70 (codewords 0 and 69 compared)."""
    H, B, BSUM, pb, ps, it, rows, want = special_case(name)
    dec = special_decoder(H, B, BSUM, it)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = dec.min_sum_soft_batch(pb, ps)
        same(got, want, rows=rows, what=name)
        assert got["costs"].shape == pb.shape and got["costs_sum"].shape == ps.shape
        same(dec.min_sum_soft_batch(pb[:1], ps[:1]), {k: v[:1] for k, v in got.items()}, what=name + " batch 1")
        if name == "tree":
            dec.configure(var_small=0, llr_tiled=0)  # the same through the generic kernel
            same(dec.min_sum_soft_batch(pb, ps), got, what="generic kernel")
    dec.close()


@functools.lru_cache(maxsize=None)
def config4_case():
    H = golden("regular_identity_300_150_3_6_s1").to_dense(np.int8)
    pmf = config4_pmf(70)
    rows = np.array([0, 69])
    want = ref.min_sum_soft(pyoracle, H, 1, pmf[rows], 2)
    return H, pmf, rows, want


def test_config4_graph_bit_exact_against_the_restatement():
    """Config 4's 150 x 450 graph (Q = 3, checks of 7 edges), 2 iterations, batch 70: codewords 0 and 69."""
    H, pmf, rows, want = config4_case()
    dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, 2)
    same(dec.min_sum_soft_batch(pmf), want, rows=rows)
    dec.close()


# ------------------------------------------------------------------------------------------------------- invisible to the forms
def test_every_check_kernel_form_gives_the_same_soft_outputs():
    H, pmf, _, _ = config4_case()
    dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, 2)
    base = dec.min_sum_soft_batch(pmf)
    for name, kn in PLAIN_FORMS:
        dec.configure(**kn)
        same(dec.min_sum_soft_batch(pmf), base, what=name)
    dec.close()
    # DecoderSpecial, rows of 3 .. 6 coefficient edges, impossible symbols (tests/test_qary_gpu.py's mixed-degree case)
    rng = np.random.RandomState(170)
    R, NB, B, BSUM = 14, 40, 2, 12
    Hp = np.zeros((R, NB), dtype=np.int8)
    for r in range(R):
        k = 6 if r % 3 else rng.randint(3, 6)
        Hp[r, rng.choice(NB, k, replace=False)] = rng.choice([-1, 1], size=k)
    H = np.concatenate([Hp, np.eye(R, dtype=np.int8)], axis=1)
    pb = rng.dirichlet(np.ones(5) * 0.7, size=(70, NB)).astype(np.float32)
    ps = rng.dirichlet(np.ones(25) * 0.7, size=(70, R)).astype(np.float32)
    zb = rng.rand(70, NB, 5) < 0.1
    zb[..., B] = False
    pb[zb] = 0.0
    pb = (pb / pb.sum(axis=2, keepdims=True)).astype(np.float32)
    dec = special_decoder(H, B, BSUM, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        base = dec.min_sum_soft_batch(pb, ps)
        for name, kn in SPECIAL_FORMS:
            dec.configure(**kn)
            same(dec.min_sum_soft_batch(pb, ps), base, what=name)
            assert np.array_equal(dec.min_sum_batch(pb, ps), base["symbols"]), name
    dec.close()


# ------------------------------------------------------------------------------------------------- consistent with the plain call
def consistent(res, plain, H, alphabets):
    """symbols = the plain call's = first minimum of each cost row; margins and unmet counts follow from costs, symbols and H."""
    assert np.array_equal(res["symbols"], plain)
    tables = [res["costs"]] + ([res["costs_sum"]] if "costs_sum" in res else [])
    v0 = 0
    for tab, Bv in zip(tables, alphabets):
        for b in range(tab.shape[0]):
            for v in range(tab.shape[1]):
                ma = ref.first_min(tab[b, v])
                assert ma - Bv == res["symbols"][b, v0 + v], (b, v)
                assert ref.same_bits(ref.margin_of(tab[b, v], ma), res["margins"][b, v0 + v]), (b, v)
        v0 += tab.shape[1]
    assert np.array_equal(res["unmet"], ref.unmet_checks(H, res["symbols"]))


def test_outputs_agree_with_the_plain_call_and_with_each_other():
    """One iteration on config 4's graph (cycles, noisy codewords) leaves checks unmet; five iterations on clean and lightly
    noisy codewords end on valid words: both kinds occur, and the counts are those of H on the returned symbols."""
    H, _, _, _ = config4_case()
    pmf = config4_pmf(24, seed=77)
    kinds = set()
    for it in (1, 5):
        dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, it)
        res = dec.min_sum_soft_batch(pmf)
        consistent(res, dec.min_sum_batch(pmf), H, [1])
        kinds |= set((res["unmet"] > 0).tolist())
        assert res["unmet"].max() <= 150 and (res["margins"] >= 0).all()
        dec.close()
    assert kinds == {False, True}
    Hs, B, BSUM, pb, ps, it, _, _ = special_case("wide")
    dec = special_decoder(Hs, B, BSUM, it)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = dec.min_sum_soft_batch(pb[:9], ps[:9])
        consistent(res, dec.min_sum_batch(pb[:9], ps[:9]), Hs, [B, BSUM])
    dec.close()


# ------------------------------------------------------------------------------------------------------------ edges of the copy
SENT_F, SENT_I, PAD = np.float32(-7.5), -77, 200


def padded_call(dec, pmf, device, costs=True, margins=True, unmet=True):
    """The C entry point on arrays that are followed by a sentinel-filled tail; returns the outputs after checking the tails."""
    nb, N, Q = pmf.shape
    sizes = dict(symbols=(nb * N, np.int8, SENT_I), costs=(nb * N * Q, np.float32, SENT_F), margins=(nb * N, np.float32, SENT_F),
                 unmet=(nb, np.int32, SENT_I))
    asked = dict(symbols=True, costs=costs, margins=margins, unmet=unmet)
    host = {k: np.full(n + PAD, s, dtype=dt) for k, (n, dt, s) in sizes.items() if asked[k]}
    L = lib.load()
    if device:
        import torch

        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        d_in = torch.from_numpy(pmf).cuda()
        dec.min_sum_soft_batch_device(d_in.data_ptr(), nb, dev["symbols"].data_ptr(), *(dev[k].data_ptr() if k in dev else 0 for k in ("costs", "margins", "unmet")),
                                      stream=torch.cuda.current_stream().cuda_stream)
        host = {k: v.cpu().numpy() for k, v in dev.items()}
    else:
        lib.check(L.scaldpc_qary_min_sum_batch_soft(dec._h, lib.ptr(pmf), nb, 0, None, *(lib.ptr(host.get(k)) for k in ("symbols", "costs", "margins", "unmet"))))
    out = {}
    for k, a in host.items():
        n, _, s = sizes[k]
        assert (a[n:] == s).all(), f"{k}: written past [batch][rows] (batch {nb}, device {device})"
        out[k] = a[:n]
    out["symbols"] = out["symbols"].reshape(nb, N)
    if costs:
        out["costs"] = out["costs"].reshape(nb, N, Q)
    if margins:
        out["margins"] = out["margins"].reshape(nb, N)
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ragged_batches_and_rows_stay_inside_their_arrays(device):
    """N * Q = 1350 rows = 21 tiles of 64 and a tail of 6; batches 1, 63, 64, 65, 130: every output equals the corresponding rows
    of the batch-130 call (itself held to the host-buffer Python call), nothing is written behind [batch][rows]."""
    H, _, _, _ = config4_case()
    pmf = config4_pmf(130, seed=4)
    dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, 2)
    full = dec.min_sum_soft_batch(pmf)
    for nb in (130, 1, 63, 64, 65):
        same(padded_call(dec, pmf[:nb], device), {k: v[:nb] for k, v in full.items()}, what=f"batch {nb}")
    # any subset of the three outputs: the same values as the full call
    for mask in range(8):
        c, m, u = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        got = padded_call(dec, pmf[:65], device, costs=c, margins=m, unmet=u)
        want = {k: v[:65] for k, v in full.items() if dict(symbols=True, costs=c, margins=m, unmet=u)[k]}
        same(got, want, what=f"subset {mask}")
        py = dec.min_sum_soft_batch(pmf[:65], costs=c, margins=m, unmet=u)
        assert set(py) == set(want)
        same(py, want, what=f"python subset {mask}")
    dec.close()


# ------------------------------------------------------------------------------------------------------------- device pointers
def test_device_pointer_calls_plain_calls_around_them_and_batch_position():
    import torch

    H, _, _, _ = config4_case()
    pmf = config4_pmf(130, seed=5)
    dec = qary.decoder_class("DecoderN450R150V3C7B1")(H, 3)
    before = dec.min_sum_batch(pmf)
    host = dec.min_sum_soft_batch(pmf)
    assert np.array_equal(dec.min_sum_batch(pmf), before) and np.array_equal(host["symbols"], before)  # a soft call changes nothing
    assert np.array_equal(dec.min_sum_batch(pmf[:70]), before[:70])
    # a codeword's outputs depend neither on its place in the batch nor on the batch size
    same(dec.min_sum_soft_batch(pmf[::-1].copy()), {k: v[::-1] for k, v in host.items()}, what="reversed")
    for i in (0, 63, 64, 129):
        same(dec.min_sum_soft_batch(pmf[i : i + 1]), {k: v[i : i + 1] for k, v in host.items()}, what=f"alone {i}")
    dec.close()
    # DecoderSpecial through device pointers: two cost tables
    Hs, B, BSUM, pb, ps, it, _, _ = special_case("kyber")
    dk = special_decoder(Hs, B, BSUM, it)
    hostk = dk.min_sum_soft_batch(pb, ps)
    t = dict(b=torch.from_numpy(pb).cuda(), s=torch.from_numpy(ps).cuda(), symbols=torch.zeros((70, 1280), dtype=torch.int8, device="cuda"),
             costs=torch.zeros((70, 768, 5), device="cuda"), costs_sum=torch.zeros((70, 512, 25), device="cuda"),
             margins=torch.zeros((70, 1280), device="cuda"), unmet=torch.full((70,), -1, dtype=torch.int32, device="cuda"))
    dk.min_sum_soft_batch_device(t["b"].data_ptr(), t["s"].data_ptr(), 70, t["symbols"].data_ptr(), t["costs"].data_ptr(), t["costs_sum"].data_ptr(),
                                 t["margins"].data_ptr(), t["unmet"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    same({k: t[k].cpu().numpy() for k in KEYS}, hostk, what="special, device pointers")
    m_only = torch.zeros((70, 1280), device="cuda")
    dk.min_sum_soft_batch_device(t["b"].data_ptr(), t["s"].data_ptr(), 70, t["symbols"].data_ptr(), d_margins=m_only.data_ptr())
    assert ref.same_bits(m_only.cpu().numpy(), hostk["margins"])
    assert np.array_equal(dk.min_sum_batch(pb, ps), hostk["symbols"])
    dk.close()


# ---------------------------------------------------------------------------------------------------------- errors and lifetime
def test_errors_are_the_plain_calls():
    H, B, pmf, it, _ = plain_case("cycles_q3")
    dec = plain_decoder(H, B, it)

    def message(fn, *a):
        with pytest.raises(Exception) as e:
            fn(*a)
        return type(e.value), str(e.value)

    bad = pmf[:3].copy()
    bad[2, 5] = 0.5  # a row that does not sum to 1: SCALDPC_EPMF
    assert message(dec.min_sum_soft_batch, bad) == message(dec.min_sum_batch, bad) and "[4]" in message(dec.min_sum_soft_batch, bad)[1]
    dec.close()
    Hn = np.array([[1, 1]], dtype=np.int8)  # x0 + x1 = 0 with both pinned to +1: no finite configuration, SCALDPC_ENOCONF
    pn = np.zeros((2, 2, 3), dtype=np.float32)
    pn[:, :, 2] = 1.0
    dn = plain_decoder(Hn, 1, 2)
    with np.errstate(divide="ignore"):
        assert message(dn.min_sum_soft_batch, pn) == message(dn.min_sum_batch, pn) and "[5]" in message(dn.min_sum_soft_batch, pn)[1]
    L = lib.load()
    out = np.zeros((2, 2), dtype=np.int8)
    assert L.scaldpc_qary_min_sum_batch_soft(dn._h, lib.ptr(pn), 2, lib.F_ASYNC, None, lib.ptr(out), None, None, None) == lib.EINVAL
    assert L.scaldpc_qary_special_min_sum_batch_soft(dn._h, lib.ptr(pn), lib.ptr(pn), 2, 0, None, lib.ptr(out), None, None, None, None) == lib.EINVAL
    dn.close()
    Hs, B, BSUM, pb, ps, it, _, _ = special_case("tree")
    ds = special_decoder(Hs, B, BSUM, it)
    sym = np.zeros((2, Hs.shape[1]), dtype=np.int8)
    cb, cs = np.zeros((2,) + pb.shape[1:], dtype=np.float32), np.zeros((2,) + ps.shape[1:], dtype=np.float32)
    call = lambda *o: L.scaldpc_qary_special_min_sum_batch_soft(ds._h, lib.ptr(pb[:2]), lib.ptr(ps[:2]), 2, 0, None, lib.ptr(sym), *o)  # noqa: E731
    assert call(lib.ptr(cb), None, None, None) == lib.EINVAL and b"both or neither" in L.scaldpc_last_error()
    assert call(None, lib.ptr(cs), None, None) == lib.EINVAL
    assert call(lib.ptr(cb), lib.ptr(cs), None, None) == 0 and call(None, None, None, None) == 0
    assert np.array_equal(sym, ds.min_sum_batch(pb[:2], ps[:2]))
    assert L.scaldpc_qary_special_min_sum_batch_soft(ds._h, lib.ptr(pb[:2]), lib.ptr(ps[:2]), 2, lib.F_ASYNC | lib.F_DEVICE_IO, None, lib.ptr(sym), None, None, None, None) == lib.EINVAL
    assert L.scaldpc_qary_min_sum_batch_soft(ds._h, lib.ptr(pb[:2]), 2, 0, None, lib.ptr(sym), None, None, None) == lib.EINVAL
    ds.close()


def test_soft_buffers_are_released_and_a_failed_allocation_leaves_a_working_handle():
    """create / soft call / destroy returns every block; with the k-th allocation of the soft call failing (its own staging
    buffers: the workspaces exist after a plain call of the same batch) the call gives ENOMEM (MemoryError), and the SAME
    handle then decodes, plain and soft."""
    H, B, pmf, it, want = plain_case("cycles_q3")
    L = lib.load()
    base = lib.live_blocks()
    keys = ("device_blocks", "device_bytes", "pinned_blocks", "pinned_bytes")
    dec = plain_decoder(H, B, it)
    dec.min_sum_batch(pmf)
    plain_blocks = lib.live_blocks()["device_blocks"]
    with np.errstate(divide="ignore"):
        same(dec.min_sum_soft_batch(pmf), want)
    assert lib.live_blocks()["device_blocks"] == plain_blocks + 5  # totals, margins, their [batch][...] forms, unmet counts
    dec.close()
    assert all(lib.live_blocks()[k] == base[k] for k in keys)
    assert L.scaldpc_debug_fail_alloc(0) == 0
    failed = 0
    try:
        for k in range(1, 8):
            dec = plain_decoder(H, B, it)
            plain = dec.min_sum_batch(pmf)
            assert L.scaldpc_debug_fail_alloc(k) == 0  # (armed: SCALDPC_DEBUG=1, tests/conftest.py)
            try:
                with np.errstate(divide="ignore"):
                    got = dec.min_sum_soft_batch(pmf)
                L.scaldpc_debug_fail_alloc(0)
                assert k == 6  # five buffers of its own
            except MemoryError:
                L.scaldpc_debug_fail_alloc(0)
                failed += 1
                assert k <= 5
                assert np.array_equal(dec.min_sum_batch(pmf), plain)
                with np.errstate(divide="ignore"):
                    got = dec.min_sum_soft_batch(pmf)
            same(got, want, what=f"k = {k}")
            dec.close()
            assert all(lib.live_blocks()[k2] == base[k2] for k2 in keys), k
            if k == 6:
                break
    finally:
        L.scaldpc_debug_fail_alloc(0)
    assert failed == 5


# ----------------------------------------------------------------------------------------------------------------------- drop-in
def test_dropin_classes_expose_the_soft_methods():
    drop = os.path.join(ROOT, "sca-ldpc_amd", "dropin")
    if drop not in sys.path:
        sys.path.insert(0, drop)
    import simulate_rs

    assert callable(getattr(simulate_rs, "DecoderN1280R512SW6").min_sum_soft_batch)
    H, B, pmf, it, want = plain_case("tree_b1")
    nz = H != 0
    cls = getattr(simulate_rs, f"DecoderN{H.shape[1]}R{H.shape[0]}V{nz.sum(axis=0).max()}C{nz.sum(axis=1).max()}B1")
    d = cls(H, it)
    one = d.min_sum_soft(pmf[5])
    assert one["symbols"] == d.min_sum(pmf[5]) == [int(x) for x in want["symbols"][5]] and one["unmet"] == 0
    assert ref.same_bits(one["costs"], want["costs"][5]) and ref.same_bits(one["margins"], want["margins"][5])
    d.close()
