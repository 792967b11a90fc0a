"""The kernel census ratchet (CPU suite): every kernel instantiation of the built library is on record with the GPU test
files that launch it.

More than half of the library's kernels are template instantiations picked at run time, and the suite is organised by
feature: twice an instantiation that no test reached was found by accident (tests/test_bp_gpu.py, "33- to 64-edge rows
of the first-pass kernels"; tests/test_isa_lint.py).  tests/golden/kernel_census.json lists every kernel of the library
by its key (`profiles/kernel_census.py`: demangled name with template arguments, no parameter list) with the GPU test
files whose profiler trace shows it, and this test holds the list against the built library: an instantiation that
appears or vanishes fails it until the census is taken again, and an entry that nothing launches needs a waiver that
says why.  What no tool sees is whether the launching test compares anything: `held_by` names, for the instantiations
the matrix tests were written for, the test that does."""
import importlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import isa_lint  # noqa: E402
import kernel_census  # noqa: E402

CENSUS = os.path.join(ROOT, "tests", "golden", "kernel_census.json")
REGENERATE = ("take the census again: profiles/kernel_census/README.md (one profiler kernel trace per GPU test file, "
              "`profiles/kernel_census.py reduce` on each, then `merge`)")
# `file:line` of the dispatch condition that makes an instantiation unreachable through the C ABI
_CONDITION = re.compile(r"\b[\w/.-]+\.(?:hip|h|py):\d+\b")

needs_tools = pytest.mark.skipif(
    not os.path.exists(os.path.join(isa_lint.LLVM_BIN, "llvm-objdump")) or kernel_census.demangler() is None,
    reason="llvm-objdump or a demangler not found")


def _census():
    with open(CENSUS) as fh:
        return json.load(fh)


def test_key_drops_prefix_return_type_and_parameters():
    k = kernel_census.key_of
    assert k("void (anonymous namespace)::k_check_tanh<16, true, false, (anonymous namespace)::SoftPrior>(int const*, float*, "
             "(anonymous namespace)::FusedTest)") == "k_check_tanh<16, true, false, SoftPrior>"
    assert k("(anonymous namespace)::k_finalize(int, int, unsigned long long*)") == "k_finalize"
    assert k("void (anonymous namespace)::k_q_check<unsigned __int128>(int, unsigned long long const*) [clone .kd]") == "k_q_check<unsigned __int128>"
    assert k("void k_var_rec<32, SharedPrior, true>(float*)") == "k_var_rec<32, SharedPrior, true>"
    assert k("k_mc_result.kd") == "k_mc_result"


@needs_tools
def test_census_lists_exactly_the_kernels_of_the_built_library():
    lib = importlib.import_module("sca-ldpc_amd._lib")
    keys = set(kernel_census.library_keys(lib.build(verbose=False)))
    assert len(keys) > 100, len(keys)
    listed = set(_census())
    new, gone = sorted(keys - listed), sorted(listed - keys)
    assert not new and not gone, (f"kernels of the library that the census does not list: {new}; listed kernels the library "
                                  f"no longer has: {gone}; {REGENERATE}")


def test_every_entry_is_launched_or_waived():
    census = _census()
    for key, e in census.items():
        assert set(e) == {"launched_by", "dispatches", "held_by", "waiver"}, key
        assert e["launched_by"] or e["waiver"], f"{key}: launched by no GPU test file and not waived; {REGENERATE}"
        if e["launched_by"]:
            assert e["dispatches"] > 0 and e["held_by"], key
            for f in e["launched_by"]:
                assert os.path.exists(os.path.join(ROOT, f)), (key, f)
            held = e["held_by"].split("::")[0]
            held = held if held.endswith(".py") else held.replace(".", "/") + ".py"
            assert os.path.exists(os.path.join(ROOT, held)), (key, e["held_by"])


def test_a_waiver_is_a_measurement_kernel_or_quotes_its_dispatch_condition():
    for key, e in _census().items():
        if e["waiver"] is None:
            continue
        assert not e["launched_by"], f"{key} is launched: drop its waiver"
        if key.startswith("k_rmw_stream"):  # the ten kernels of scaldpc_measure_rmw_stream: no decoder output
            continue
        m = _CONDITION.search(e["waiver"])
        assert m, f"{key}: the waiver must quote the dispatch condition (file:line) that makes it unreachable"
        path, line = m.group(0).rsplit(":", 1)
        found = [p for p in (os.path.join(ROOT, path), os.path.join(ROOT, "sca-ldpc_amd", "csrc", path)) if os.path.exists(p)]
        assert found, (key, path)
        with open(found[0]) as fh:
            assert int(line) <= sum(1 for _ in fh), (key, m.group(0))


def test_the_tile_row_parallel_and_lds_kernels_are_held_by_an_oracle_test():
    """For the template grid of the binary BP kernels, `held_by` names a test (not just a file), and the test exists."""
    families = ("k_check_tanh<", "k_check_minsum_x<", "k_check_minsum_rec<", "k_check_minsum<", "k_var<", "k_var_first<",
                "k_var_rec<", "k_el_check<", "k_el_var<", "k_bp_small<")
    census = _census()
    held = {k: e for k, e in census.items() if k.startswith(families)}
    assert len(held) >= 70, len(held)
    for key, e in held.items():
        if e["waiver"]:
            continue
        assert "::" in e["held_by"], f"{key}: held_by must name the test that compares it with the oracle"
        path, name = e["held_by"].split("::")[:2]
        with open(os.path.join(ROOT, path)) as fh:
            assert re.search(r"^def %s\(" % re.escape(name.split("[")[0]), fh.read(), re.M), (key, e["held_by"])
        assert path in e["launched_by"], f"{key}: {path} holds it but its trace does not show it"
