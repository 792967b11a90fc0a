"""Which rows the record check pass may trim (csrc/scaldpc_rec_trim.h): a row is marked exactly when its LAST edge goes into a
column of degree 1.  The header is compiled for the HOST (tests/rec_trim_main.cc, with the address and undefined-behaviour
sanitizers where the toolchain has their runtimes) and held to a plain numpy statement of the rule on hand-made corner
cases and on random graphs; the mark must not disturb what the other check kernels read in the descriptor word."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_trim") / "rec_trim_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "rec_trim_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: rec_trim_main is built without them")
        subprocess.check_call(cmd)

    def run(*words):
        out = subprocess.run([exe] + [str(w) for w in words], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return dict(kv.split("=") for kv in out.stdout.split())

    return run


def marks(tool, rows, n):
    """rows: list of column lists (ascending).  Returns the tool's marks as a list of 0 / 1."""
    got = tool("mark", len(rows), n, *[len(r) for r in rows], "--", *[c for r in rows for c in r])
    mk = [] if got["mark"] == "-" else [int(ch) for ch in got["mark"]]
    assert len(mk) == len(rows) and int(got["marked"]) == sum(mk)
    cols = [] if got["cols"] == "-" else [int(c) for c in got["cols"].rstrip(",").split(",")]
    assert cols == [r[-1] if k else -1 for r, k in zip(rows, mk)]  # a marked row comes with the column of its last edge
    return mk


def expected(rows, n):
    cdeg = np.bincount(np.array([c for r in rows for c in r], dtype=np.int64), minlength=n)
    return [int(bool(r) and cdeg[r[-1]] == 1) for r in rows]


def test_corner_cases(tool):
    # [Hin | I]: every row ends in its own column
    rows = [[0, 1, 3], [1, 2, 4], [0, 2, 5]]
    assert marks(tool, rows, 6) == [1, 1, 1]
    # [I | Hin]: the constant edge comes first -- not marked
    rows = [[0, 3, 4], [1, 4, 5], [2, 3, 5]]
    assert marks(tool, rows, 6) == [0, 0, 0]
    # a row whose only edge is constant; a row whose last TWO edges are; a row that ends in a column of degree 2
    rows = [[5], [0, 1, 3, 4], [0, 1, 2], [2]]
    assert marks(tool, rows, 6) == [1, 1, 0, 0]
    # empty rows before, between and behind (they share their start with the next row), and an empty graph
    rows = [[], [0, 1], [], [], [0, 2], []]
    assert marks(tool, rows, 3) == [0, 1, 0, 0, 1, 0]
    assert marks(tool, [], 0) == [] and marks(tool, [[], []], 4) == [0, 0]
    # a column of degree 1 gets a second edge (what append_rows can do): its row loses the mark
    rows = [[0, 2], [1, 3]]
    assert marks(tool, rows, 4) == [1, 1]
    assert marks(tool, rows + [[0, 2, 4]], 5) == [0, 1, 1]


def test_random_graphs(tool):
    rng = np.random.RandomState(811)
    seen = set()
    for _ in range(40):
        m, n = rng.randint(1, 12), rng.randint(1, 14)
        H = rng.rand(m, n) < rng.choice([0.1, 0.25, 0.5])
        rows = [list(np.flatnonzero(r)) for r in H]
        got = marks(tool, rows, n)
        assert got == expected(rows, n), rows
        seen.update(got)
    assert seen == {0, 1}


def test_descriptor_word(tool):
    max_col = (1 << 23) - 1  # the word's column field
    for bound in (2, 4, 8, 16, 32, 64):
        for col in (0, 1, 21668, max_col):
            w = tool("word", bound, 1 + col)
            assert (int(w["flag"]), int(w["bound"]), int(w["col"])) == (1, bound, col) and int(w["word"]) > 0
        w = tool("word", bound, 0)
        assert (int(w["flag"]), int(w["bound"]), int(w["word"])) == (0, bound, bound)
        # a column the field cannot hold: the row stays unmarked (all loads, as before)
        assert int(tool("word", bound, 2 + max_col)["word"]) == bound
    # an any-degree row (bound 0) is never marked: k_check_tanh reads "word == 0" as "the any-degree fallback"
    assert int(tool("word", 0, 1)["word"]) == 0
    src = open(os.path.join(ROOT, "sca-ldpc_amd", "csrc", "scaldpc_bp.hip")).read()
    body = re.search(r"int ensure_tile_tables\(scaldpc_bp \*h\)\s*\{(.*?)\n\}", src, re.S).group(1)
    assert "rec_mark_const_last(" in body and "rec_desc_word(" in body  # ... and the table builder asks
