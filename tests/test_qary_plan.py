"""Which kernels a q-ary call runs is decided by one pure host function, qary_plan (csrc/scaldpc_qary_plan.h).  Here the
header is compiled for the HOST (tests/qary_plan_main.cc, with the address and undefined-behaviour sanitizers where the
toolchain has their runtimes) and held to a table written from the documented rules -- the knob comment of
include/scaldpc.h and DESIGN.md 4 -- not from the code.  tests/test_qary_gpu.py::test_the_plan_is_what_runs ties the plan
to the launches on the device."""
import os
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")  # the C++ driver of oracle/Makefile's gcc

# scaldpc_qary_last_timing's info[1] (include/scaldpc.h) = qary.CHECK_KERNELS
CHECK = ("k_q_check_unrolled<3,7>", "k_q_check_unrolled<5,5>", "k_q_special_check_tree<5,6>", "k_q_special_check_wave", "k_q_check_wave",
         "k_q_special_check", "k_q_check", "k_q_special_check_dp<5,6>", "k_q_check_dp<3,7>")
VAR = ("generic", "small", "small_special")
LLR = ("fused_both", "fused_each", "unfused")

# DecoderN450R150V3C7B1 and DecoderN1280R512SW6
GENERIC = dict(special=0, R=150, N=450, E=1050, Q=3, QS=3, W=3, maxdc=7, mindc=7, maxdv=3)
SPECIAL = dict(special=1, R=512, N=1280, E=3584, Q=5, QS=25, W=25, maxdc=7, mindc=7, maxdv=4)


def generic(Q=3, **kw):
    return dict(GENERIC, Q=Q, QS=Q, W=Q, **kw)


def special(QS=25, **kw):
    return dict(SPECIAL, QS=QS, W=max(5, QS), **kw)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qary_plan") / "qary_plan_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "qary_plan_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: qary_plan_main is built without them")
        subprocess.check_call(cmd)

    def run(shape, batch, **knobs):
        args = [str(shape[k]) for k in ("special", "R", "N", "E", "Q", "QS", "W", "maxdc", "mindc", "maxdv")] + [str(batch)]
        out = subprocess.run([exe] + args + [f"{k}={v}" for k, v in knobs.items()], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        p = {k: int(v) for k, v in (kv.split("=") for kv in out.stdout.split())}
        if not p["refused"]:
            p["check_name"] = CHECK[p["check"]] if p["check"] >= 0 else None
            p["var_name"], p["llr_name"] = VAR[p["var"]], LLR[p["llr"]]
        return p

    return run


def test_the_program_takes_only_the_plan_header():
    src = open(os.path.join(ROOT, "tests", "qary_plan_main.cc")).read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include \"")] == ['"../sca-ldpc_amd/csrc/scaldpc_qary_plan.h"']
    hdr = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_qary_plan.h")).read()
    assert "hip" not in [ln.split("<")[1].split("/")[0] for ln in hdr.splitlines() if ln.startswith("#include <")]
    assert '#include "' not in hdr


# ------------------------------------------------------------------------------------------ generic decoder, config 4's shape
@pytest.mark.parametrize("batch", [1, 20, 1024])
def test_generic_defaults(plan, batch):
    p = plan(generic(), batch)
    assert p["check_name"] == "k_q_check_dp<3,7>" and p["var_name"] == "small"
    assert p["llr_name"] == "fused_each" and p["init"] == 0  # tiled + fused: k_q_init is not launched


@pytest.mark.parametrize("knobs, batch, want", [
    (dict(dp=0), 1, "k_q_check_unrolled<3,7>"),
    (dict(dp=0), 1024, "k_q_check_unrolled<3,7>"),
    (dict(unroll=0), 256, "k_q_check_wave"),
    (dict(unroll=0), 257, "k_q_check"),
    (dict(unroll=0, wave=0), 1, "k_q_check"),
    (dict(unroll=0, wave=1), 1024, "k_q_check_wave"),
])  # fmt: skip
def test_generic_check_knobs(plan, knobs, batch, want):
    p = plan(generic(), batch, **knobs)
    assert p["check_name"] == want
    if want == "k_q_check":
        assert p["check_words128"] == 0 and p["T"] == 64  # 64-bit digit words
        assert p["check_lds"] == 7 * 3 * 9 * 64  # A, Bt floats + fin bytes per (edge, symbol, thread)


def test_generic_variable_and_conversion_knobs(plan):
    assert plan(generic(), 20, var_small=0)["var_name"] == "generic"
    p = plan(generic(), 20, llr_tiled=0)
    assert (p["llr_name"], p["llr_tiled_b"], p["init"]) == ("unfused", 0, 1)  # plain conversion, then k_q_init
    assert plan(generic(), 20, var_small=0)["var_lds"] == 2 * 3 * 64 * 4


# ------------------------------------------------------------------------------------------------ generic decoder, other shapes
@pytest.mark.parametrize("dp", [0, 1])
def test_q5_dc5_is_unrolled_whatever_dp_is(plan, dp):
    assert plan(generic(Q=5, maxdc=5, mindc=5), 20, dp=dp)["check_name"] == "k_q_check_unrolled<5,5>"


def test_q5_dc6_takes_the_wave_kernel(plan):
    assert plan(generic(Q=5, maxdc=6, mindc=6), 4)["check_name"] == "k_q_check_wave"


@pytest.mark.parametrize("batch", [1, 256, 1024])
def test_degree_9_takes_the_lane_kernel_with_128_bit_words(plan, batch):
    p = plan(generic(maxdc=9, mindc=9), batch, wave=1, unroll=1)
    assert p["check_name"] == "k_q_check" and p["check_words128"] == 1


@pytest.mark.parametrize("Q, maxdc, T", [(15, 7, 64), (31, 7, 32), (255, 3, 8)])
def test_lane_form_block_size_fits_64_kb(plan, Q, maxdc, T):
    p = plan(generic(Q=Q, maxdc=maxdc, mindc=maxdc), 1024, wave=0, unroll=0)
    assert p["check_name"] == "k_q_check" and p["T"] == T and p["check_lds"] == maxdc * Q * 9 * T <= 64 * 1024


def test_the_plan_refuses_what_does_not_fit(plan):
    for knobs in (dict(), dict(wave=1), dict(wave=0, unroll=0)):  # whatever check kernel would be chosen
        assert plan(generic(Q=255, maxdc=4, mindc=4, maxdv=1), 1, **knobs)["refused"] == 1
    assert plan(generic(Q=255, maxdc=3, mindc=3, maxdv=1), 1)["refused"] == 0


def test_columns_of_five_checks_take_the_generic_variable_form(plan):
    assert plan(generic(maxdv=5), 20)["var_name"] == "generic"
    assert plan(generic(maxdv=4), 20)["var_name"] == "small"


# ------------------------------------------------------------------------------------------------- special decoder, Kyber SW6
@pytest.mark.parametrize("knobs, batch, want, parts", [
    (dict(), 1, "k_q_special_check_tree<5,6>", None),
    (dict(), 4, "k_q_special_check_tree<5,6>", None),
    (dict(), 5, "k_q_special_check_dp<5,6>", 4),
    (dict(), 64, "k_q_special_check_dp<5,6>", 4),
    (dict(), 65, "k_q_special_check_dp<5,6>", 2),
    (dict(), 192, "k_q_special_check_dp<5,6>", 2),
    (dict(), 193, "k_q_special_check_dp<5,6>", 1),
    (dict(dp=0), 256, "k_q_special_check_tree<5,6>", None),
    (dict(tree=0, dp=0), 1, "k_q_special_check_wave", None),
    (dict(tree=0, dp=0), 1024, "k_q_special_check_wave", None),
    (dict(tree=0), 4, "k_q_special_check_wave", None),
    (dict(tree=0), 5, "k_q_special_check_dp<5,6>", 4),
    (dict(wave=0), 1, "k_q_special_check", None),
    (dict(wave=0), 256, "k_q_special_check", None),
    (dict(dp_min=1, dp_split=0, dp_split2=0), 1, "k_q_special_check_dp<5,6>", 1),
])  # fmt: skip
def test_special_check_kernels(plan, knobs, batch, want, parts):
    p = plan(special(), batch, **knobs)
    assert p["check_name"] == want
    if parts is not None:
        assert p["check_parts"] == parts
    assert p["wave_fallback_nb"] == -1  # every row has six coefficient edges: no follow-up launch
    assert p["var_name"] == "small_special"
    assert p["llr_name"] == "fused_both" and p["init"] == 0  # one fused launch for both alphabets


@pytest.mark.parametrize("batch, want", [(1, "k_q_special_check_tree<5,6>"), (70, "k_q_special_check_dp<5,6>")])
def test_mixed_row_degrees_get_the_follow_up_wave_launch(plan, batch, want):
    p = plan(special(mindc=4), batch)
    assert p["check_name"] == want and p["wave_fallback_nb"] == 6  # the wave kernel skips the six-edge rows
    assert p["wave_lds"] == (6 * 5 + 25) * 65 * 4
    p = plan(special(mindc=4), batch, tree=0, dp=0)
    assert p["check_name"] == "k_q_special_check_wave" and p["wave_fallback_nb"] == -1  # the form itself: nothing follows


# ------------------------------------------------------------------------------------------------ special decoder, other shapes
def test_special_other_shapes(plan):
    sw4 = special(QS=17, maxdc=5, mindc=5)
    p = plan(sw4, 20)
    assert p["check_name"] == "k_q_special_check_wave" and p["var_name"] == "generic"
    assert plan(sw4, 20, wave=0)["check_name"] == "k_q_special_check"
    p = plan(special(QS=29), 20)
    assert p["var_name"] == "generic" and p["llr_name"] == "fused_both"
    p = plan(special(QS=33, maxdc=5, mindc=5), 20)  # Q = 5 with QS > 32
    assert (p["llr_name"], p["llr_tiled_b"], p["llr_tiled_s"], p["init"]) == ("unfused", 1, 0, 1)


def test_a_graph_without_edges(plan):
    p = plan(generic(E=0, maxdc=0, mindc=0, maxdv=0), 20)
    assert p["check"] == -1 and p["init"] == 0 and p["llr_name"] == "unfused"


def test_knob_clamps(plan):
    p = plan(generic(), 1, wave=-7, dp_min=0, dp_split=-3, dp_split2=-1, unroll=5)
    assert (p["wave"], p["dp_min"], p["dp_split"], p["dp_split2"], p["unroll"]) == (-1, 1, 0, 0, 1)
    p = plan(generic(), 1)
    assert [p[k] for k in ("wave", "unroll", "tree", "dp", "dp_min", "dp_split", "dp_split2", "llr_tiled", "var_small", "timing")] == [
        -1, 1, 1, 1, 5, 64, 192, 1, 1, 0]
