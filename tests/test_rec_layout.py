"""A tile's block of the min-sum record form (csrc/scaldpc_rec_pack.h): the plane of first magnitudes, 64 floats a row,
the plane of second magnitudes m rows behind it, and behind both the arg-min plane, 64 bytes a row.  The helpers that
place them are plain C++; tests/rec_layout_main.cc is built with the host compiler (with the address and
undefined-behaviour sanitizers where the toolchain has their runtimes) and asked for every size at which the rounding to
whole lines can go wrong: the planes of a block do not overlap, a block is a whole number of 256-B lines, magnitude rows
are 8-byte aligned, the arg-min plane starts where it is said to, and the byte distance between the two magnitude
planes fits the 32-bit lane offset the variable pass adds it to."""
import os
import subprocess
import warnings

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_layout") / "rec_layout_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "rec_layout_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: rec_layout_main is built without them")
        subprocess.check_call(cmd)

    def run(*words):
        out = subprocess.run([exe] + [str(w) for w in words], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return {k: int(v) for k, v in (kv.split("=") for kv in out.stdout.split())}

    return run


def sizes(tool):
    return [1, 2, 63, 64, 65, 4000, tool("limits")["max_rows"]]


def planes(lay, m):
    """[begin, end) in bytes of the three planes of a block of m rows"""
    row = 4 * lay["row_floats"]
    m1 = (0, 4 * lay["row_last"] + row)
    m2 = (4 * lay["m2_off"], 4 * (lay["m2_off"] + lay["row_last"]) + row)
    arg = (4 * lay["arg_off"], 4 * lay["arg_off"] + m * lay["arg_row_bytes"])
    return m1, m2, arg


def test_planes_do_not_overlap(tool):
    for m in sizes(tool):
        lay = tool("layout", m)
        assert lay["tw"] == 64 and lay["row_floats"] == lay["tw"] and lay["arg_row_bytes"] == lay["tw"]
        assert lay["row_last"] == (m - 1) * lay["row_floats"]
        m1, m2, arg = planes(lay, m)
        assert m1[0] < m1[1] <= m2[0] < m2[1] <= arg[0] < arg[1] <= 4 * lay["tile_floats"], (m, lay)


def test_blocks_are_whole_lines(tool):
    for m in sizes(tool):
        lay = tool("layout", m)
        assert (4 * lay["tile_floats"]) % 256 == 0, m
        # ... and no larger than they have to be: less than a line of padding
        used = planes(lay, m)[2][1]
        assert 0 <= 4 * lay["tile_floats"] - used < 256, m


def test_alignment_and_stated_offsets(tool):
    for m in sizes(tool):
        lay = tool("layout", m)
        assert (4 * lay["row_floats"]) % 8 == 0 and (4 * lay["row_last"]) % 8 == 0 and (4 * lay["m2_off"]) % 8 == 0  # 8-byte aligned rows
        assert lay["m2_off"] == m * lay["tw"]  # the second magnitudes lie m rows behind the first
        assert lay["arg_off"] == 2 * m * lay["tw"]  # the arg-min plane follows both magnitude planes
        assert (4 * lay["arg_off"]) % 64 == 0  # (its 64-byte rows are aligned to themselves)
        assert 4 * lay["m2_off"] + 4 * (lay["tw"] - 1) < 1 << 32  # the lane's byte offset into the second plane: 32 bits
