"""The C-ABI library loads without a GPU and exports every symbol include/scaldpc.h declares."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "scaldpc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(scaldpc_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_boundary():
    fns = declared_functions()
    for must in ("scaldpc_bp_create", "scaldpc_bp_set_channel_probs", "scaldpc_bp_decode_batch", "scaldpc_bp_destroy",
                 "scaldpc_qary_create", "scaldpc_qary_min_sum_batch", "scaldpc_qary_special_create",
                 "scaldpc_qary_special_min_sum_batch", "scaldpc_qary_destroy", "scaldpc_last_error"):
        assert must in fns


def test_library_exports_every_declared_symbol():
    L = importlib.import_module("sca-ldpc_amd._lib")
    lib = L.load()  # raises if the HIP extension is missing: there is no fallback
    for fn in declared_functions():
        assert hasattr(lib, fn), f"{fn} declared in include/scaldpc.h but not exported"
    assert lib.scaldpc_version() == 104  # (round 4: scaldpc_measure_rmw_stream added, A/B knobs removed, fault injector opt-in)


def test_errors_cross_the_boundary_as_codes_not_exceptions():
    L = importlib.import_module("sca-ldpc_amd._lib")
    lib = L.load()
    h = ctypes.c_void_p()
    rc = lib.scaldpc_bp_create(0, 5, 0, None, None, ctypes.byref(h))
    assert rc == L.EINVAL and b"bad graph" in lib.scaldpc_last_error()
    import numpy as np
    H = np.array([[1, 2, 0]], dtype=np.int8)  # entry outside {-1,0,1}
    rc = lib.scaldpc_qary_create(1, 3, 1, H.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(h))
    assert rc == L.EINVAL


def test_fault_injector_is_opt_in():
    """scaldpc_debug_fail_alloc arms only in a process started with SCALDPC_DEBUG=1 (an always-compiled,
    process-wide injector any caller could arm).  Without the variable the export refuses with SCALDPC_EINVAL."""
    import subprocess
    import sys

    L = importlib.import_module("sca-ldpc_amd._lib")
    code = ("import ctypes,sys;l=ctypes.CDLL(sys.argv[1]);l.scaldpc_last_error.restype=ctypes.c_char_p;"
            "rc=l.scaldpc_debug_fail_alloc(3);print(rc, l.scaldpc_last_error().decode());print(l.scaldpc_debug_fail_alloc(0))")
    env = {k: v for k, v in os.environ.items() if k != "SCALDPC_DEBUG"}
    r = subprocess.run([sys.executable, "-c", code, L.SO_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    first, second = r.stdout.strip().splitlines()
    assert first.startswith(str(L.EINVAL)) and "SCALDPC_DEBUG=1" in first and second.strip() == "0"
    r = subprocess.run([sys.executable, "-c", code, L.SO_PATH], capture_output=True, text=True, env=dict(env, SCALDPC_DEBUG="1"), timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[0].startswith("0"), r.stdout + r.stderr


def test_no_product_module_touches_the_oracle():
    """The product path must never import, load or call anything under oracle/."""
    pkg = os.path.join(ROOT, "sca-ldpc_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                assert "pyoracle" not in txt and "liboracle" not in txt and "from oracle" not in txt, os.path.join(d, f)


def test_dropin_modules_import():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "sca-ldpc_amd", "dropin"))
    import ldpc
    import simulate_rs

    assert ldpc.bp_decoder.__name__ == "BpDecoder"
    assert ldpc.codes.rep_code(13).shape == (12, 13)
    assert simulate_rs.DecoderN450R150V3C7B1.Q == 3 and simulate_rs.DecoderN1280R512SW6.BSUM == 12
    # the import line of simulate/hqc.py:23 must work; constants yes, cryptography no
    from simulate_rs import Hqc128, Hqc192, Hqc256

    assert (Hqc128.params("N"), Hqc128.params("omega"), Hqc128.params("N1") * Hqc128.params("N2")) == (17669, 66, 17664)
    assert (Hqc192.params("N"), Hqc256.params("N"), Hqc256.params("DELTA")) == (35851, 57637, 29)
    assert Hqc128.name() == "Hqc128"
    import pytest

    with pytest.raises(NotImplementedError):
        Hqc128.keypair()
    with pytest.raises(ValueError):
        Hqc128.params("nope")
