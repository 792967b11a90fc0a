"""Which blocks of the column records a record-form variable pass launches is a pure function of integers
(rec_var_slices, csrc/scaldpc_bp_sched.h): the slim pass that leaves the degree-1 bucket out, the wide (32, 64] bucket with a
launch of its own, records laid out heaviest first, and grid.x rounded up to 8 under the XCD map.  A wrong slice is a silent
skip of columns.  Here the header -- compiled for the HOST with the address and undefined-behaviour sanitizers
(tests/rec_slices_main.cc) -- is held to a restatement of the rules in Python: on hand-worked cases whose expected lines are
written out below, on the bucket tables of the graphs tests/rec_wide_cases.py builds, and on seeded random tables."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import kernel_matrix_cases as K
import rec_wide_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rec_slices") / "rec_slices_main")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "rec_slices_main.cc"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the host toolchain lacks the sanitizer runtimes: rec_slices_main is built without them")
        subprocess.check_call(cmd)

    def run(cases):
        lines = [case_line(*c) for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands here)
        return [[int(w) for w in ln.split()[1:]] for ln in out.stdout.splitlines()]

    return run


def case_line(maxd, blk, rev, light, wo, G, maxcol):
    assert len(blk) == len(maxd) + 1
    return " ".join(map(str, ["slices", len(maxd), *maxd, *blk, int(rev), int(light), int(wo), G, maxcol]))


# ---- the rules, restated: block by block -----------------------------------------------------------------------------
# A table is (maxd, blk): bucket b = blocks [blk[b], blk[b + 1]) of columns with at most maxd[b] edges, ascending, no
# bucket empty; reversed, the records run the other way.  Every block belongs to exactly one of: the wide launch (bound
# above 32), the blocks left out (bound 1, in a pass after iteration 1 without output, unless that bucket is all there is),
# the narrow launch.
def bounds_in_order(maxd, blk, rev):
    order = [maxd[b] for b in range(len(maxd)) for _ in range(blk[b + 1] - blk[b])]
    return order[::-1] if rev else order


def left_out(maxd, blk, rev, light, wo):
    if not (light and not wo and maxd and maxd[0] == 1 and len(maxd) > 1):
        return []
    return [i for i, d in enumerate(bounds_in_order(maxd, blk, rev)) if d == 1]


def model(maxd, blk, rev, light, wo, G, maxcol):
    """[narrow0, narrow_n, narrow_deg, narrow_grid, wide0, wide_n, wide_grid, xmap]; the first block of an empty slice is None."""
    order = bounds_in_order(maxd, blk, rev)
    skipped = set(left_out(maxd, blk, rev, light, wo))
    wide = [i for i, d in enumerate(order) if d > 32]
    narrow = [i for i, d in enumerate(order) if d <= 32 and i not in skipped]
    for run in (wide, narrow):  # a slice is contiguous
        assert run == list(range(run[0], run[0] + len(run))) if run else True
    xmap = G in (2, 4, 8)

    def grid(count):
        return -(-count // 8) * 8 if xmap else count

    # the narrow launch is compiled for the widest bucket it may meet: with a wide bucket, the widest of the others
    narrow_deg = max([d for d in maxd if d <= 32], default=0) if wide else maxcol
    return [narrow[0] if narrow else None, len(narrow), narrow_deg, grid(len(narrow)),
            wide[0] if wide else None, len(wide), grid(len(wide)), int(xmap)]  # fmt: skip


def same(got, want):
    return all(g == w or (w is None and i in (0, 4)) for i, (g, w) in enumerate(zip(got, want))) and len(got) == len(want)


# ---- hand-worked cases -----------------------------------------------------------------------------------------------
HQC = ([1, 16], [0, 1000, 1500])  # 4000 identity columns in 1000 blocks, then 500 blocks of columns of up to 16 edges
WIDE16 = ([1, 16, 64], [0, 10, 25, 27])
WIDE32 = ([1, 16, 32, 64], [0, 10, 25, 30, 32])


def test_hqc_like_table(tool):
    cases = [(*HQC, False, True, False, 1, 16),  # light, no output: blocks [0, 1000) are left out
             (*HQC, False, True, True, 1, 16),   # with output: nothing is left out
             (*HQC, False, False, False, 1, 16), # iteration 1 (not light): nothing is left out
             (*HQC, True, True, False, 1, 16),   # heaviest first: the degree-1 bucket ends the records, [500, 1500) left out
             (*HQC, True, True, True, 1, 16)]  # fmt: skip
    got = tool(cases)
    assert got == [[1000, 500, 16, 500, 1500, 0, 0, 0],
                   [0, 1500, 16, 1500, 1500, 0, 0, 0],
                   [0, 1500, 16, 1500, 1500, 0, 0, 0],
                   [0, 500, 16, 500, 0, 0, 0, 0],
                   [0, 1500, 16, 1500, 0, 0, 0, 0]]  # fmt: skip
    assert all(same(g, model(*c)) for g, c in zip(got, cases))
    assert left_out(*HQC, False, True, False) == list(range(1000)) and left_out(*HQC, True, True, False) == list(range(500, 1500))


def test_only_degree_one(tool):
    # the degree-1 bucket is all there is: the slim pass is off and all blocks are launched
    cases = [(([1]), [0, 7], rev, True, False, 1, 1) for rev in (False, True)]
    got = tool(cases)
    assert got == [[0, 7, 1, 7, 7, 0, 0, 0], [0, 7, 1, 7, 0, 0, 0, 0]]
    assert all(same(g, model(*c)) for g, c in zip(got, cases))


def test_wide_bucket(tool):
    # a (32, 64] last bucket of 2 blocks: its own slice; the narrow cap follows the widest NARROW bucket, whatever the
    # widest column (40 here); reversed, the wide blocks lead the records
    cases = [(*WIDE16, False, True, False, 1, 40), (*WIDE16, True, True, False, 1, 40), (*WIDE16, False, True, True, 1, 40),
             (*WIDE32, False, True, False, 1, 40), (*WIDE32, True, True, False, 1, 40), (*WIDE32, True, False, True, 1, 40)]  # fmt: skip
    got = tool(cases)
    assert got == [[10, 15, 16, 15, 25, 2, 2, 0],
                   [2, 15, 16, 15, 0, 2, 2, 0],
                   [0, 25, 16, 25, 25, 2, 2, 0],
                   [10, 20, 32, 20, 30, 2, 2, 0],
                   [2, 20, 32, 20, 0, 2, 2, 0],
                   [2, 30, 32, 30, 0, 2, 2, 0]]  # fmt: skip
    assert all(same(g, model(*c)) for g, c in zip(got, cases))


def test_only_the_wide_bucket(tool):
    cases = [([64], [0, 3], rev, True, wo, 1, 50) for rev in (False, True) for wo in (False, True)]
    got = tool(cases)
    # narrow count 0: no narrow launch (reversed, its empty slice starts behind the wide blocks)
    assert got == [[0, 0, 0, 0, 0, 3, 3, 0]] * 2 + [[3, 0, 0, 0, 0, 3, 3, 0]] * 2
    assert all(same(g, model(*c)) for g, c in zip(got, cases))
    # ... and a degree-1 bucket beside it, left out: still no narrow launch
    assert tool([([1, 64], [0, 5, 8], False, True, False, 1, 50)]) == [[5, 0, 1, 0, 5, 3, 3, 0]]


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16])
def test_grid_rounds_up_under_the_xcd_map(tool, G):
    # 15 narrow blocks and 2 wide ones: grid.x = 16 and 8 exactly where the launch's tiles divide the 8 XCDs
    (got,) = tool([(*WIDE16, False, True, False, G, 40)])
    xmap = G in (2, 4, 8)
    assert got == ([10, 15, 16, 16, 25, 2, 8, 1] if xmap else [10, 15, 16, 15, 25, 2, 2, 0])
    # a count that is a multiple of 8 already stays
    assert tool([([16], [0, 24], False, True, False, G, 16)]) == [[0, 24, 16, 24, 24, 0, 0, int(xmap)]]


# ---- the bucket tables of real graphs --------------------------------------------------------------------------------
BOUNDS = [1, 2, 4, 8, 16, 32, 64]  # (finish_graph: bucket b holds the columns with BOUNDS[b-1] < degree <= BOUNDS[b])


def bucket_table(cdeg):
    """(maxd, blk) of a graph's columns: isolated columns go with degree 1, empty buckets are left out, 4 columns a block."""
    assert cdeg.max() <= BOUNDS[-1]
    maxd, blk, lo = [], [0], -1
    for hi in BOUNDS:
        cnt = int(((cdeg > lo) & (cdeg <= hi)).sum())
        if cnt:
            maxd.append(hi)
            blk.append(blk[-1] + (cnt + 3) // 4)
        lo = hi
    return maxd, blk


def graph_tables():
    out = {}
    for R_, C in W.WIDE:  # one wide column in 72 x 200
        G, _ = K.graph(R_, C, False, W.SEEDS[(R_, C, False)])
        out[f"matrix-{R_}-{C}"] = G.col_degrees()
    out["staircase"] = W.staircase()[0].col_degrees()  # 192 x 665, one column of every degree 0 .. 64
    return out


def test_graph_tables(tool):
    for name, cdeg in graph_tables().items():
        maxd, blk = bucket_table(np.asarray(cdeg))
        nblk, maxcol = blk[-1], int(np.max(cdeg))
        assert maxd[0] == 1 and maxd[-1] == 64, name
        cases = [(maxd, blk, rev, light, wo, G, maxcol) for rev in (False, True) for light in (False, True) for wo in (False, True)
                 for G in (1, 2, 3)]  # fmt: skip
        got = tool(cases)
        for g, c in zip(got, cases):
            assert same(g, model(*c)), (name, c, g)
            covered = sorted(list(range(g[0], g[0] + g[1])) + list(range(g[4], g[4] + g[5])) + left_out(*c[:5]))
            assert covered == list(range(nblk)), (name, c, g)
        if name == "staircase":  # 32 columns of 33 .. 64 edges = 8 blocks; the narrow launch is the 32-edge build
            assert all(g[5] == 8 and g[2] == 32 for g in got)
        else:  # ONE wide column = one block; the columns beside it have at most 6 edges: the 16-edge build
            assert all(g[5] == 1 and g[2] == 8 for g in got)


# ---- seeded random tables --------------------------------------------------------------------------------------------
def test_random_tables(tool):
    rng = np.random.default_rng(20261)
    cases = []
    for _ in range(1500):
        nb = int(rng.integers(1, len(BOUNDS) + 1))
        maxd = sorted(int(x) for x in rng.choice(BOUNDS, size=nb, replace=False))
        blk = [0] + [int(x) for x in np.cumsum(rng.integers(1, 40, nb))]
        lo = BOUNDS[BOUNDS.index(maxd[-1]) - 1] if maxd[-1] > 1 else 0
        maxcol = int(rng.integers(lo + 1, maxd[-1] + 1))  # the widest column lies in the last bucket
        cases.append((maxd, blk, bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2)), int(rng.integers(1, 10)), maxcol))
    got = tool(cases)
    assert len(got) == len(cases)
    for g, c in zip(got, cases):
        assert same(g, model(*c)), (c, g)
        # the narrow and the wide slice are disjoint, and with the blocks left out they cover [0, nblk) exactly once
        narrow, wide = list(range(g[0], g[0] + g[1])), list(range(g[4], g[4] + g[5]))
        assert sorted(narrow + wide + left_out(*c[:5])) == list(range(c[1][-1])), (c, g)
        assert g[3] >= g[1] and g[6] >= g[5] and g[3] - g[1] < 8 and g[6] - g[5] < 8
        assert (g[3] % 8 == 0 and g[6] % 8 == 0) if c[5] in (2, 4, 8) else (g[3] == g[1] and g[6] == g[5])
