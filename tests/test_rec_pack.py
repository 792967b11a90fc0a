"""The variable pass of the min-sum record form reads one word per edge that holds the edge's row AND its index in that
row (csrc/scaldpc_rec_pack.h).  The header is compiled for the HOST (tests/rec_pack_main.cc, with the address and
undefined-behaviour sanitizers where the toolchain has their runtimes): every (row, index) the record form can meet
survives the round trip, and a graph with more rows than the word holds is REFUSED by rec_rows_fit -- the predicate
rec_form() ends with -- so it runs in the message form instead of overflowing into the index bits."""
import os
import re
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_pack") / "rec_pack_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "rec_pack_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: rec_pack_main is built without them")
        subprocess.check_call(cmd)

    def run(*words):
        out = subprocess.run([exe] + [str(w) for w in words], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return {k: int(v) for k, v in (kv.split("=") for kv in out.stdout.split())}

    return run


def test_limits_hold_what_the_record_form_needs(tool):
    lim = tool("limits")
    assert lim["max_row_deg"] >= 64  # rows of the record form have at most 64 edges
    assert lim["max_rows"] < 1 << lim["row_bits"]  # every row index fits the row bits
    assert lim["rec2_bytes_max"] < 1 << 32  # the byte distance to the second magnitudes fits the 32-bit lane offset
    assert lim["max_rows"] >= 1 << 20  # (and no graph of a size anybody decodes is turned away)


def test_round_trip(tool):
    lim = tool("limits")
    for row in (0, 1, 12345, lim["max_rows"] - 1):
        for k in (0, 1, 31, 32, 63):
            got = tool("pack", row, k)
            assert (got["row"], got["index"]) == (row, k), (row, k, got)
            assert got["word"] == row | (k << lim["row_bits"])


def test_too_many_rows_fall_back(tool):
    lim = tool("limits")
    assert tool("fit", 1, 1)["fit"] == 1
    assert tool("fit", lim["max_rows"], 64)["fit"] == 1
    assert tool("fit", lim["max_rows"] + 1, 64)["fit"] == 0  # one row too many: message form
    assert tool("fit", 1 << 31, 8)["fit"] == 0
    assert tool("fit", 1000, lim["max_row_deg"] + 1)["fit"] == 0
    # ... and rec_form() asks: the predicate is part of its condition
    src = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_bp.hip")).read()
    body = re.search(r"bool rec_form\(const scaldpc_bp \*h, int method\)\s*\{(.*?)\n\}", src, re.S).group(1)
    assert "rec_rows_fit(h->m, h->max_row_deg)" in body
