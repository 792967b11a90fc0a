"""The lane-offset rule (csrc/scaldpc_bp_sched.h, phase_reestablished): does a tile group (re-)establish the one-kernel offset
between neighbouring lanes when it starts?  The rule in force is "always", whatever the chain bits, the settle horizon and
the iteration count (profiles/minsum_settle_passes/README.md has the measurement).  Here the header -- compiled for the HOST
with the address and undefined-behaviour sanitizers (tests/phase_sched_main.cc) -- is held to a restatement in Python, over
the whole grid of inputs and over fixed-iteration levels whose chain bits come from chain_bits itself."""
import itertools
import os
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("phase_sched") / "phase_sched_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "phase_sched_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: phase_sched_main is built without them")
        subprocess.check_call(cmd)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return [[w if i == 0 else int(w) for i, w in enumerate(ln.split())] for ln in out.stdout.splitlines()]

    return run


# ---- the rule, restated ---------------------------------------------------------------------------------------------
def model_phase(chain, horizon, max_iter):
    """Every group re-establishes the offset: a group that continues nobody's lanes must (its lanes start together), and for
    a chained one carrying the offset over measured inside the run-to-run spread, with and without a horizon."""
    return 1


def model_chain(groups, full_last):
    """chain_bits of a fixed-iteration level on two lanes: a full group continues a full predecessor (bit 0) and leaves its
    lanes to a full successor (bit 1); a partial last group does neither."""
    full = [True] * (groups - 1) + [bool(full_last)]
    out = []
    for g in range(groups):
        c = 0
        if full[g]:
            c |= 1 if g > 0 else 0
            c |= 2 if g + 1 < groups and full[g + 1] else 0
        out.append(c)
    return out


def test_rule_over_the_grid(tool):
    grid = list(itertools.product(range(4), (0, 3, 8, 12, 49, 50), (1, 2, 13, 50, 1000)))
    got = tool([f"phase {c} {k} {m}" for c, k, m in grid])
    assert got == [["phase", model_phase(c, k, m)] for c, k, m in grid]


@pytest.mark.parametrize("groups,full_last", [(1, 1), (1, 0), (2, 1), (2, 0), (3, 0), (16, 1), (17, 0)])
@pytest.mark.parametrize("horizon,max_iter", [(0, 50), (12, 50)])
def test_levels(tool, groups, full_last, horizon, max_iter):
    """The flagship's level is (16, 1): one unchained start, fifteen chained groups."""
    got = tool([f"level {groups} {full_last} {horizon} {max_iter}"])
    chain = model_chain(groups, full_last)
    assert got == [["group", c, model_phase(c, horizon, max_iter)] for c in chain]
    assert chain[0] & 1 == 0 and got[0][2] == 1  # a level's first group continues nobody: it must set the offset
