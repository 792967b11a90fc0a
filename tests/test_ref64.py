"""The float64 ratio-domain decode (scaldpc_bp_decode_batch_f64), CPU side: the entry point is declared and exported, the
Python keywords bind, and the instances the GPU tests (tests/test_ref64_gpu.py) decode are what those tests need them to
be -- pinned here on the oracle alone (method 0, float64), so that a GPU test cannot pass by decoding something easy."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import mc_ref
import ref64_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = importlib.import_module("sca-ldpc_amd")
bp = importlib.import_module("sca-ldpc_amd.bp")
driver = importlib.import_module("sca-ldpc_amd.driver")
_lib = importlib.import_module("sca-ldpc_amd._lib")


def test_entry_point_declared_and_exported():
    with open(os.path.join(ROOT, "include", "scaldpc.h")) as fh:
        header = fh.read()
    proto = re.search(r"int scaldpc_bp_decode_batch_f64\(([^;]*)\);", header)
    assert proto, "include/scaldpc.h does not declare scaldpc_bp_decode_batch_f64"
    args = " ".join(proto.group(1).split())
    assert args == ("scaldpc_bp *h, const uint8_t *in, int32_t input_kind, int32_t batch, const double *probs, "
                    "int32_t prob_cols, int32_t max_iter, uint32_t flags, void *stream, uint8_t *out_bits, double *out_llr, "
                    "int32_t *out_iters, uint8_t *out_conv")
    assert "#define SCALDPC_VERSION 104" in header
    comment = header[header.rfind("/*", 0, proto.start()) : proto.start()]
    assert "(entry point added under SCALDPC_VERSION 104: nothing that existed changed)" in comment
    lib = C.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "scaldpc_bp_decode_batch_f64"), "libscaldpc.so does not export scaldpc_bp_decode_batch_f64"
    assert lib.scaldpc_version() == 104
    # the binding declares it (13 arguments, an int status)
    _lib._declare(lib)
    assert len(lib.scaldpc_bp_decode_batch_f64.argtypes) == 13 and lib.scaldpc_bp_decode_batch_f64.restype is C.c_int


def test_python_keywords_bind():
    inspect.signature(bp.BpDecoder.__init__).bind(None, [[1]], precision="float64")
    assert inspect.signature(bp.BpDecoder.__init__).parameters["precision"].default is None
    inspect.signature(bp.BpDecoder.decode_batch).bind(None, [[0]], precision="float64")
    inspect.signature(bp.BpDecoder.decode_batch_device).bind(None, 0, 0, 1, 0, precision="float64")
    inspect.signature(driver.hqc_decode_batch).bind(7, None, [], [], precision="float64")
    inspect.signature(driver.hqc_decode).bind(7, None, [], [], precision="float64")
    for f in (bp.BpDecoder.decode_batch, bp.BpDecoder.decode_batch_device, driver.hqc_decode_batch, driver.hqc_decode):
        assert inspect.signature(f).parameters["precision"].default is None


def test_precision_is_validated_before_any_library_call(monkeypatch):
    """"float64" with a min-sum method, or a precision that is none, raises ValueError with nothing loaded or built."""
    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    H = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.int8)
    with pytest.raises(ValueError, match="min-sum"):
        bp.bp_decoder(H, error_rate=0.1, bp_method="min_sum", precision="float64")
    with pytest.raises(ValueError, match="invalid"):
        bp.bp_decoder(H, error_rate=0.1, bp_method="product_sum", precision="float16")
    monkeypatch.setenv("SCALDPC_PRECISION", "float64")
    with pytest.raises(ValueError, match="SCALDPC_PRECISION"):
        bp.bp_decoder(H, error_rate=0.1, bp_method="ms")


@pytest.mark.parametrize("name, counts, converged", [("F", 7, 109), ("H1", 9, 101), ("H2", 9, 72)])
def test_mc_instances_are_hard_enough(name, counts, converged):
    """130 trials, 30 iterations, method 0 in float64: several iteration counts, converged and stuck codewords."""
    H, probs, x, kind = cases.mc_case(name)
    assert x.shape[0] == mc_ref.RUNS == 130 and kind == (0 if name == "F" else 1)
    # rows and columns of at most 16 edges: the 16-edge builds of the register-resident check and variable kernels
    assert np.diff(H.row_ptr).max() <= 16 and np.diff(H.col_ptr).max() <= 16
    ref = cases.mc_oracle(name, True)
    assert len(np.unique(ref["iters"])) == counts and int(ref["converged"].sum()) == converged
    if name == "F":  # its p = 0 / 1 / 2^-33 priors
        assert probs[0] == 0.0 and probs[1] == 1.0 and probs[2] == 2.0**-33 and probs[-1] == 0.0
    fixed = cases.mc_oracle(name, False)
    assert (fixed["iters"] == mc_ref.MAX_ITER).all() and 0 < fixed["converged"].sum() < 130


@pytest.mark.parametrize("colmax, counts, converged", [(64, 12, 67), (32, 2, 42)])
def test_staircase_instances(colmax, counts, converged):
    G, probs, synd = cases.staircase_case(colmax)
    rdeg, cdeg = np.diff(G.row_ptr), np.diff(G.col_ptr)
    assert set(rdeg) == set(range(1, 65)) and set(range(colmax + 1)) <= set(cdeg) and cdeg.max() == colmax
    assert synd.shape[0] == 150  # (rows up to 64: the widest register-resident check build; columns: the 32-edge variable
    # build, and at colmax 64 the any-degree column loop for 33 .. 64)
    ref = cases.staircase_oracle(colmax)
    assert len(np.unique(ref["iters"])) == counts and int(ref["converged"].sum()) == converged


def test_wide_toy_reaches_the_any_degree_loops():
    G, probs, synd = cases.wide_case()
    rdeg, cdeg = np.diff(G.row_ptr), np.diff(G.col_ptr)
    assert 65 <= rdeg.max() <= 200 and (rdeg > 64).sum() == 2 and cdeg.max() > 64
    assert (probs == 0.0).any() and (probs == 1.0).any()
    ref = cases.wide_oracle()
    conv = ref["converged"].astype(bool)
    assert len(np.unique(ref["iters"])) >= 2 and conv.any() and (~conv).any()
    assert np.isinf(ref["llr"]).any()  # the p = 0 / p = 1 priors show in the posteriors


def test_full_size_rows_hold_stuck_and_converged_codewords():
    H, _, _ = cases.full_size_case()
    # 51-edge rows: the 52-edge build of the register-resident check kernel; columns of up to 16 edges
    assert set(np.diff(H.row_ptr)) == {51} and np.diff(H.col_ptr).max() == 16
    ref = cases.full_size_oracle()
    assert set(ref["iters"]) == {3, 4, 50}
    assert ((ref["iters"] == 50) == (ref["converged"] == 0)).all()
    # the fp32 oracle in the kernels' order agrees on the iteration counts of all 16: the fp32 comparison of the GPU test has
    # codewords to compare
    assert np.array_equal(cases.full_size_oracle("f32")["iters"], ref["iters"])


def test_worst_ulp_measure():
    a = np.array([1.0, -2.0, np.inf, np.nan, 0.5])
    b = a.copy()
    assert cases.worst_ulp(a, b) == 0.0
    b[0] = np.nextafter(np.nextafter(1.0, 2.0), 2.0)
    assert cases.worst_ulp(b, a) == 2.0
    c = a.copy()
    c[2] = -np.inf
    with pytest.raises(AssertionError):
        cases.worst_ulp(c, a)
    d = a.copy()
    d[3] = 1.0
    with pytest.raises(AssertionError):
        cases.worst_ulp(d, a)
