"""DecoderSpecial for checks of any length (k_q_special_check_dp_any, csrc/scaldpc_qary_special.h), the parts that need no GPU:
the launch plan's rules for the new kernel (include/scaldpc.h), the three-field decoder name
DecoderN{N}R{R}SW{SW}B{B}, and the identity the kernel rests on at the row lengths it exists for.  The kernel itself is held
to the oracle, to exact inference and to a plain enumeration in tests/test_qary_special_any_gpu.py."""
import importlib
import os
import subprocess
import warnings

import numpy as np
import pytest

from test_min_marginal_identity import _draw, special_check_enumerated, special_check_minplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")
qary = importlib.import_module("sca-ldpc_amd.qary")

DP_ANY = 9  # QCheck::SPECIAL_DP_ANY = scaldpc_qary_last_timing's info[1]
# DecoderN1280R512SW6 (tests/test_qary_plan.py) and DecoderN1024R256SW9B2
SW6 = dict(special=1, R=512, N=1280, E=3584, Q=5, QS=25, W=25, maxdc=7, mindc=7, maxdv=4)
SW9 = dict(special=1, R=256, N=1024, E=2560, Q=5, QS=37, W=37, maxdc=10, mindc=4, maxdv=3)


def shape(base, Q=None, maxdc=None, **kw):
    g = dict(base, **kw)
    if Q is not None:
        g["Q"] = Q
    if maxdc is not None:
        g["maxdc"] = maxdc
    B = (g["Q"] - 1) // 2
    g["QS"] = 2 * B * (g["maxdc"] - 1) + 1  # BSUM = SW B
    g["W"] = max(g["Q"], g["QS"])
    return g


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """tests/qary_plan_main.cc, built as tests/test_qary_plan.py builds it."""
    exe = str(tmp_path_factory.mktemp("qary_plan_any") / "qary_plan_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "qary_plan_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: qary_plan_main is built without them")
        subprocess.check_call(cmd)

    def run(g, batch, **knobs):
        args = [str(g[k]) for k in ("special", "R", "N", "E", "Q", "QS", "W", "maxdc", "mindc", "maxdv")] + [str(batch)]
        out = subprocess.run([exe] + args + [f"{k}={v}" for k, v in knobs.items()], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr
        return {k: int(v) for k, v in (kv.split("=") for kv in out.stdout.split())}

    return run


# ------------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("batch", [1, 70, 1024])
@pytest.mark.parametrize("knobs", [dict(), dict(wave=0), dict(wave=1), dict(tree=0), dict(dp=0), dict(wave=0, tree=0, dp=0), dict(dp_any=1)])
def test_checks_of_ten_edges_take_the_new_kernel_whatever_the_other_knobs_say(plan, batch, knobs):
    p = plan(SW9, batch, **knobs)
    assert p["refused"] == 0 and p["check"] == DP_ANY
    assert p["wave_fallback_nb"] == -1 and p["check_parts"] == 1  # every row, one wave per (check, 64 codewords): nothing follows
    # 37 > 32 row-sum symbols: the conversion takes the unfused path, the variable pass k_q_var
    assert (p["llr"], p["llr_tiled_b"], p["llr_tiled_s"], p["init"], p["var"]) == (2, 1, 0, 1, 0)


@pytest.mark.parametrize("batch", [1, 4, 5, 64, 70, 256, 1024])
def test_the_kyber_shape_takes_it_on_demand_only(plan, batch):
    default = plan(SW6, batch)
    assert default["check"] in (2, 7) and default == plan(SW6, batch, dp_any=-1)  # tree walk / k_q_special_check_dp<5,6>, as before
    forced = plan(SW6, batch, dp_any=1)
    assert forced["check"] == DP_ANY and forced["wave_fallback_nb"] == -1 and forced["check_parts"] == 1
    assert plan(dict(SW6, mindc=4), batch, dp_any=1)["wave_fallback_nb"] == -1  # mixed rows: still nothing follows
    off = plan(SW6, batch, dp_any=0)
    assert {k: v for k, v in off.items()} == {k: v for k, v in default.items()}  # (the plan prints no dp_any knob)


def test_every_other_shape_keeps_its_plan(plan):
    generic = dict(special=0, R=150, N=450, E=1050, Q=3, QS=3, W=3, maxdc=7, mindc=7, maxdv=3)
    for g in (generic, dict(generic, maxdc=9, mindc=9), dict(generic, Q=5, QS=5, W=5, maxdc=6, mindc=6)):
        for dp_any in (0, 1):
            assert plan(g, 20, dp_any=dp_any) == plan(g, 20)  # the plain decoder never takes it
    sw4 = shape(SW6, maxdc=5, mindc=5)
    assert plan(sw4, 20)["check"] == 3 and plan(sw4, 20, dp_any=1)["check"] == DP_ANY
    # dp_any = 1 on another alphabet falls back to what runs today
    for Q in (9, 15):
        g = shape(SW6, Q=Q, maxdc=4, mindc=4)
        assert plan(g, 20, dp_any=1) == plan(g, 20) and plan(g, 20)["check"] == 3


def test_what_the_plan_refuses(plan):
    assert plan(SW9, 20, dp_any=0)["refused"] == 1  # nothing else runs ten edges
    assert plan(shape(SW9, Q=9), 20)["refused"] == 1 and plan(shape(SW9, Q=9), 20, dp_any=1)["refused"] == 1  # B = 4
    assert plan(shape(SW9, Q=7, maxdc=15), 20)["check"] == DP_ANY  # 6 * 14 + 1 = 85 entries: 3 * 85 * 256 = 65 280 bytes
    assert plan(shape(SW9, Q=7, maxdc=16), 20)["refused"] == 1  # 91 entries
    assert plan(shape(SW9, Q=3, maxdc=43), 20)["check"] == DP_ANY and plan(shape(SW9, Q=3, maxdc=44), 20)["refused"] == 1
    assert plan(shape(SW9, Q=5, maxdc=22), 20)["check"] == DP_ANY and plan(shape(SW9, Q=5, maxdc=23), 20)["refused"] == 1


def test_knob_values(plan):
    assert plan(SW9, 1, dp_any=-5)["check"] == DP_ANY and plan(SW9, 1, dp_any=7)["check"] == DP_ANY  # < 0: auto, != 0: on


# ----------------------------------------------------------------------------------------------------------------- names
def test_three_field_names():
    cls = qary.decoder_class("DecoderN33R5SW9B2")
    assert issubclass(cls, qary.QarySpecialDecoder)
    assert (cls.N, cls.R, cls.B, cls.BSUM, cls.Q, cls.QS, cls.DC) == (33, 5, 2, 18, 5, 37, 10)
    c3 = qary.decoder_class("DecoderN9R2SW12B3")
    assert (c3.B, c3.BSUM, c3.Q, c3.QS, c3.DC) == (3, 36, 7, 73, 13)
    c7 = qary.decoder_class("DecoderN40R6SW7B5")  # up to seven coefficient edges any B resolves: the enumeration kernels
    assert (c7.B, c7.BSUM, c7.DC) == (5, 35, 8)
    assert qary.decoder_class("DecoderN1024R256SW6B2").BSUM == qary.decoder_class("DecoderN1024R256SW6").BSUM == 12
    with pytest.raises(AttributeError, match="91 entries"):
        qary.decoder_class("DecoderN9R2SW15B3")
    with pytest.raises(AttributeError, match="B = 4"):
        qary.decoder_class("DecoderN9R2SW9B4")
    with pytest.raises(AttributeError, match="check degree 9"):  # the reference's two-field names keep their limit
        qary.decoder_class("DecoderN40R6SW8")
    with pytest.raises(AttributeError):
        qary.decoder_class("DecoderN40R6SW8B")
    assert qary.MAX_SPECIAL_CHECK_DEGREE == 8
    assert qary._QaryBase.CHECK_KERNELS[DP_ANY] == "k_q_special_check_dp_any" and len(qary._QaryBase.CHECK_KERNELS) == 10


def test_the_drop_in_resolves_the_three_field_name():
    import sys

    drop = os.path.join(ROOT, "sca-ldpc_amd", "dropin")
    if drop not in sys.path:
        sys.path.insert(0, drop)
    import simulate_rs

    assert getattr(simulate_rs, "DecoderN33R5SW9B2") is qary.decoder_class("DecoderN33R5SW9B2")
    with pytest.raises(AttributeError):
        getattr(simulate_rs, "DecoderN9R2SW9B4")


# -------------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("B, nb", [(1, 9), (1, 10), (2, 7), (2, 8), (3, 5)])
def test_minplus_recursion_equals_the_enumeration_at_the_new_row_lengths(B, nb):
    """special_check_minplus is the kernel's specification; special_check_enumerated the reference's form
    (tests/test_min_marginal_identity.py, which holds them together at 2 - 4 edges)."""
    rng = np.random.RandomState(100 * B + nb)
    for kind in range(6):
        BSUM = nb * B + 2 * (kind % 2)  # (with and without row-sum symbols no assignment reaches)
        a = _draw(rng, (nb, 2 * B + 1), kind)
        a_sum = _draw(rng, (2 * BSUM + 1,), kind)
        want, want_s = special_check_enumerated(a, a_sum, B, BSUM)
        got, got_s = special_check_minplus(a, a_sum, B, BSUM)
        assert want.tobytes() == got.tobytes(), (kind, a, a_sum, want, got)
        assert want_s.tobytes() == got_s.tobytes(), (kind, a, a_sum, want_s, got_s)
