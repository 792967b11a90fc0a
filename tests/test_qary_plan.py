"""Which kernels a q-ary call runs is decided by one pure host function, qary_plan (csrc/scaldpc_qary_plan.h).  Here the
header is compiled for the HOST (tests/qary_plan_main.cc, with the address and undefined-behaviour sanitizers where the
toolchain has their runtimes) and held to a table written from the documented rules -- the knob comment of
include/scaldpc.h and DESIGN.md 4 -- not from the code.  tests/test_qary_gpu.py::test_the_plan_is_what_runs ties the plan
to the launches on the device."""
import os
import subprocess
import warnings

import pytest

import qary_shape_cases as shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")  # the C++ driver of oracle/Makefile's gcc

# scaldpc_qary_last_timing's info[1] (include/scaldpc.h) = qary.CHECK_KERNELS
CHECK = ("k_q_check_unrolled<3,7>", "k_q_check_unrolled<5,5>", "k_q_special_check_tree<5,6>", "k_q_special_check_wave", "k_q_check_wave",
         "k_q_special_check", "k_q_check", "k_q_special_check_dp<5,6>", "k_q_check_dp<3,7>", "k_q_special_check_dp_any")
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

    def words(shape, batch, knobs):
        return [str(shape[k]) for k in ("special", "R", "N", "E", "Q", "QS", "W", "maxdc", "mindc", "maxdv")] + [str(batch)] + [
            f"{k}={v}" for k, v in knobs.items()]

    def parse(line):
        p = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        if not p["refused"]:
            p["check_name"] = CHECK[p["check"]] if p["check"] >= 0 else None
            p["var_name"], p["llr_name"] = VAR[p["var"]], LLR[p["llr"]]
        return p

    def run(shape, batch, **knobs):
        out = subprocess.run([exe] + words(shape, batch, knobs), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return parse(out.stdout)

    def many(calls):
        """The plans of a list of (shape, batch, knobs) out of ONE process (the program's `-` form)."""
        text = "".join(" ".join(words(*c)) + "\n" for c in calls)
        out = subprocess.run([exe, "-"], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and not out.stderr, out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(calls)
        return [parse(ln) for ln in lines]

    run.many = many
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
    p = plan(generic(), 20, var_small=0)
    assert p["var_T"] == 64 and p["var_lds"] == 2 * 3 * 64 * 4


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


# ------------------------------------------------------------------------------------------- every launch within 64 KB of LDS
@pytest.mark.parametrize("W, var_T", [(3, 64), (127, 64), (129, 32), (255, 32)])
def test_the_variable_kernel_block_size_fits_64_kb(plan, W, var_T):
    """k_q_var stages two rows of W floats per codeword: 64 codewords per block while that fits 64 KB (W <= 128), halved
    beyond.  Written from the rule (include/scaldpc.h): 2 * 4 * 128 * 64 = 65 536."""
    want_lds = {3: 1536, 127: 65024, 129: 33024, 255: 65280}[W]
    assert want_lds == 2 * W * var_T * 4 <= 64 * 1024 and (var_T == 64 or 2 * W * (2 * var_T) * 4 > 64 * 1024)
    p = plan(generic(Q=W, maxdc=2, mindc=2), 20, var_small=0)
    assert (p["var_name"], p["var_T"], p["var_lds"]) == ("generic", var_T, want_lds)
    p = plan(dict(SPECIAL, Q=3, QS=W, W=W, maxdc=2, mindc=2), 20)  # DecoderSpecial: the row-sum alphabet sets the width
    assert (p["var_name"], p["var_T"], p["var_lds"]) == ("generic", var_T, want_lds)


def launched_lds(p):
    """name -> dynamic LDS bytes of every kernel an accepted plan launches (csrc/scaldpc_qary.hip: launch_check, launch_var)."""
    by_form = {"k_q_check_unrolled<3,7>": 0, "k_q_check_unrolled<5,5>": 0, "k_q_check_dp<3,7>": 0, "k_q_special_check_dp<5,6>": 0,
               "k_q_special_check_tree<5,6>": p["tree_lds"], "k_q_special_check_wave": p["wave_lds"], "k_q_check_wave": p["wave_lds"],
               "k_q_special_check": p["check_lds"], "k_q_check": p["check_lds"], "k_q_special_check_dp_any": p["dp_any_lds"]}
    out = {}
    if p["check_name"] is not None:
        out[p["check_name"]] = by_form[p["check_name"]]
    if p["wave_fallback_nb"] >= 0:
        out["k_q_special_check_wave (fallback)"] = p["wave_lds"]
    if p["var_name"] == "generic":
        out["k_q_var"] = p["var_lds"]
    return out


def test_no_accepted_plan_asks_for_more_than_64_kb(plan):
    """Odd Q from 3 to 255, rows of 1 .. 16 edges (with and without a shorter row), both decoder kinds (DecoderSpecial with
    QS = Q, 2 Q + 1, 253, 255), columns of 1 and 5 checks, batches 1 and 300, default knobs and the lane form on demand: whatever
    the plan accepts, no launch of it -- the check form, the wave kernel behind the tree walk or the recursion, k_q_var --
    asks for more than 65 536 B of dynamic LDS.  Every form must have been seen, and refusals too."""
    calls = []
    for Q in range(3, 256, 2):
        kinds = [(0, Q)] + [(1, QS) for QS in sorted({Q, 2 * Q + 1, 253, 255})]
        for special_, QS in kinds:
            for maxdc in range(1, 17):
                for mindc in sorted({maxdc, max(1, maxdc - 1)} if special_ and Q == 5 else {maxdc}):  # (a shorter row: the fallback launch)
                    g = dict(special=special_, R=12, N=40, E=12 * maxdc, Q=Q, QS=QS, W=max(Q, QS), maxdc=maxdc, mindc=mindc, maxdv=1)
                    for maxdv in (1, 5):
                        for batch in (1, 300):
                            for knobs in (dict(), dict(wave=0, unroll=0, tree=0, dp=0)):
                                calls.append((dict(g, maxdv=maxdv), batch, knobs))
    plans = plan.many(calls)
    seen, refused, worst = set(), 0, {}
    for (g, batch, knobs), p in zip(calls, plans):
        if p["refused"]:
            refused += 1
            continue
        assert p["T"] in (8, 16, 32, 64) and p["var_T"] in (8, 16, 32, 64)
        for name, lds in launched_lds(p).items():
            assert lds <= 64 * 1024, (name, lds, g, batch, knobs)
            seen.add(name)
            worst[name] = max(worst.get(name, 0), lds)
    print(f"{len(calls)} shapes, {refused} refused; largest dynamic LDS per launch: {worst}")
    assert refused > 1000 and seen == set(CHECK) - {"k_q_check_unrolled<3,7>"} | {"k_q_special_check_wave (fallback)", "k_q_var"}


@pytest.mark.parametrize("name", list(shapes.PLAIN) + list(shapes.SPECIAL))
def test_the_shape_cases_take_the_branches_they_are_named_for(plan, name):
    """tests/test_qary_shapes_gpu.py's cases (tests/qary_shape_cases.py), on the shapes qary_build works out of their graphs: at
    every batch they run, each form is the named check kernel, with the block sizes, the conversion and the variable form of the
    case's table row; the lane form's block size is the one the batches are ragged against."""
    c = shapes.PLAIN.get(name) or shapes.SPECIAL[name]
    g = shapes.shape_of(name)
    per_codeword = 2 * ((g["maxdc"] - 1) * g["Q"] + g["QS"]) * 4 if g["special"] else g["maxdc"] * g["Q"] * 9
    assert shapes.block_size(per_codeword) == c["T"]
    for knobs, kernel in c["forms"]:
        for batch in shapes.batches(c["T"]):
            p = plan(g, batch, **knobs)
            assert (p["check_name"], p["T"], p["llr_name"], p["var_name"]) == (kernel, c["T"], c["llr"], c.get("var", "generic")), (knobs, batch)
            assert p["var_T"] == (64 if g["W"] <= 128 else 32) and p["init"] == (c["llr"] == "unfused")
            assert p["check_words128"] == (kernel == "k_q_check" and g["maxdc"] > 8)
    if name in shapes.FAMILY:
        assert (plan(g, shapes.BATCH)["check_name"], plan(g, shapes.BIG)["check_name"]) == shapes.FAMILY[name]
    # what the case is there for
    want = {"q31": dict(llr_tiled_b=0), "q33": dict(llr_tiled_b=0, init=1), "SW3B7": dict(llr_tiled_b=1, llr_tiled_s=0, init=1),
            "q63": dict(wave_lds=65792), "q63_wave": dict(wave_lds=49348), "q83": dict(wave_lds=65008), "q255": dict(var_lds=65280),
            "SW2B63": dict(check_lds=64896, var_lds=2 * 253 * 32 * 4), "q15_dc8": dict(check_lds=8 * 15 * 9 * 32)}.get(name, {})
    p = plan(g, shapes.BATCH, **c["forms"][-1][0])
    assert {k: p[k] for k in want} == want
    assert g["maxdv"] == {"q15_dc8_dv5": 5, "dv9_q3": 9, "dv9_q15": 9}.get(name, g["maxdv"]) and (c.get("var") != "small" or g["maxdv"] <= 4)


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
