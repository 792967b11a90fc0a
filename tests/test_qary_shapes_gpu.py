"""The q-ary decoders against the oracle on every branch of the launch plan (csrc/scaldpc_qary_plan.h) that the other parity
tests leave alone: alphabets of 9 .. 255 symbols (k_q_var by default, with 32 codewords per block from 129 symbols on), random
pmfs over 15 symbols on rows of 8 edges, the lane kernels with 32, 16 and 8 codewords per block, the untiled conversion with
k_q_init, wave kernels whose radices exceed 64, digit words full to the last byte (8 edges in 64 bits, 16 in 128), columns of 5
and 9 checks, DecoderSpecial with B = 1 .. 63 on the wave, lane and any-length kernels.  The cases, their inputs and their keys
are tests/qary_shape_cases.py's; tests/test_qary_plan.py holds each case to the branch it is named for on the CPU.

Everything is compared bit for bit: symbols of the plain call; symbols, totals (uint32 patterns, NaN = NaN), margins and unmet
checks of the soft call -- an arg-min cannot see a last-bit difference in a message, the totals can.  The key is the C
restatement (oracle/qary_oracle.c), whose totals tests/test_qary_soft.py ties to the NumPy restatement of the whole loop."""
import importlib

import numpy as np
import pytest

import qary_shape_cases as shapes
import qary_soft_ref as ref

pytestmark = pytest.mark.gpu
qary = importlib.import_module("sca-ldpc_amd.qary")
FLOATS = ("costs", "costs_sum", "margins")
CASES = {**shapes.PLAIN, **shapes.SPECIAL}
FORMS = [(name, i) for name, c in CASES.items() for i in range(len(c["forms"]))]


def form_id(name, i):
    knobs = CASES[name]["forms"][i][0]
    return name + "-" + ("-".join(f"{k}{v}" for k, v in knobs.items()) or "default")


def decoder(name, H):
    R, N = H.shape
    if name in shapes.SPECIAL:
        c = shapes.SPECIAL[name]
        return qary.decoder_class(f"DecoderN{N}R{R}SW{c['SW']}B{c['B']}")(H, shapes.ITERATIONS)
    nz = H != 0
    B = (shapes.PLAIN[name]["Q"] - 1) // 2
    return qary.decoder_class(f"DecoderN{N}R{R}V{nz.sum(axis=0).max()}C{nz.sum(axis=1).max()}B{B}")(H, shapes.ITERATIONS)


def inputs(key, rows):
    return (key["pmf"][rows], key["pmf_sum"][rows]) if "pmf_sum" in key else (key["pmf"][rows],)


def held_to_the_key(dec, key, rows, kernel, what):
    """The plain and the soft call on the codewords `rows` of the case: the named check kernel ran, and every output is the key's."""
    args = inputs(key, rows)
    nb = len(args[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        plain = dec.min_sum_batch(*args)
        t = dec.last_timing()
        assert (t["check_kernel"], t["batch"], t["iterations"]) == (kernel, nb, shapes.ITERATIONS), what
        soft = dec.min_sum_soft_batch(*args)
        t = dec.last_timing()
        assert (t["check_kernel"], t["batch"]) == (kernel, nb), what
    bad = np.argwhere(plain != key["symbols"][rows])
    assert not len(bad), (what, "plain symbols", len(bad), bad[:5])
    assert soft["symbols"].dtype == np.int8 and np.array_equal(soft["symbols"], key["symbols"][rows]), (what, "soft symbols")
    for k in FLOATS:
        if k in key:
            a, b = soft[k], key[k][rows]
            diff = np.argwhere(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
            assert ref.same_bits(a, b), (what, k, len(diff), diff[:5])
    assert "costs_sum" in soft or "costs_sum" not in key
    assert soft["unmet"].dtype == np.int32 and np.array_equal(soft["unmet"], key["unmet"][rows]), (what, "unmet")


@pytest.mark.parametrize("name", list(CASES))
def test_the_key_is_not_vacuous(name):
    """The oracle takes the inputs (it raises otherwise); its symbols spread over the alphabet; where the case sets symbols to
    probability 0, the totals hold +inf or NaN next to finite numbers."""
    key = shapes.case(name)
    Q = 2 * key["B"] + 1
    assert key["symbols"].shape == (shapes.BATCH, key["H"].shape[1])
    assert len(np.unique(key["symbols"])) >= min(Q, 10)
    totals = np.concatenate([key[k].ravel() for k in ("costs", "costs_sum") if k in key])
    assert np.isfinite(totals).any()
    if shapes.sparse_support(name):
        assert (np.isposinf(totals) | np.isnan(totals)).any()
    assert key["margins"].shape == key["symbols"].shape and key["unmet"].shape == (shapes.BATCH,)


@pytest.mark.parametrize("name, form", FORMS, ids=[form_id(n, i) for n, i in FORMS])
def test_every_form_at_every_ragged_batch(name, form):
    """Batches 1, T - 1, T + 1 and 130 (T: codewords per block of the case's lane kernel) through one form of the check kernel."""
    c = CASES[name]
    knobs, kernel = c["forms"][form]
    key = shapes.case(name)
    dec = decoder(name, key["H"])
    dec.configure(timing=1, **knobs)
    for nb in shapes.batches(c["T"]):
        held_to_the_key(dec, key, slice(0, nb), kernel, f"{name} {knobs} batch {nb}")
    dec.close()


@pytest.mark.parametrize("name", list(shapes.FAMILY))
def test_batch_300_reversed_batch_and_device_pointers(name):
    """One case per decoder kind with default knobs: batch 300 (the plain decoder leaves the wave kernel for the lane kernel above
    256 codewords, DecoderSpecial keeps it) equals the oracle as batch 130 does; a codeword's outputs do not depend on its place
    in the batch; the device-pointer call on the caller's stream gives the same symbols."""
    import torch

    at_130, at_300 = shapes.FAMILY[name]
    key, big = shapes.case(name), shapes.case(name, shapes.BIG)
    dec = decoder(name, key["H"])
    dec.configure(timing=1)
    held_to_the_key(dec, key, slice(0, shapes.BATCH), at_130, f"{name} default batch 130")
    held_to_the_key(dec, big, slice(0, shapes.BIG), at_300, f"{name} default batch 300")
    held_to_the_key(dec, big, slice(None, None, -1), at_300, f"{name} reversed")
    held_to_the_key(dec, key, slice(70, 29, -1), at_130, f"{name} reversed slice")
    stream = torch.cuda.Stream()
    for k, nb in ((key, shapes.BATCH), (big, shapes.BIG)):
        d_in = [torch.from_numpy(np.array(a)).cuda() for a in inputs(k, slice(0, nb))]
        d_out = torch.full((nb, k["H"].shape[1]), 99, dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            dec.min_sum_batch_device(*(d.data_ptr() for d in d_in), nb, d_out.data_ptr(), stream=stream.cuda_stream)
        assert np.array_equal(d_out.cpu().numpy(), k["symbols"]), (name, nb)
    dec.close()
