"""TEST INFRASTRUCTURE shared by tests/test_mc_trial_list.py (CPU) and tests/test_mc_trial_list_gpu.py: the trial lists the
entries that decode chosen trials (scaldpc_mc_*_at) are held on.  Positions are offsets into the window
[FIRST, FIRST + RUNS) of tests/mc_ref.py, which crosses 2^32."""
import numpy as np

from mc_ref import FIRST, RUNS

PERM_SEED = 7
# 100 distinct trials of the window in a shuffled order, then a duplicate pair, both ends of the window and both sides of a tile
# boundary: 106 slots = one full tile and a ragged one
OFFSETS = np.concatenate([np.random.RandomState(PERM_SEED).permutation(RUNS)[:100], [7, 7, 129, 0, 64, 63]]).astype(np.int64)
IDS = FIRST + OFFSETS
PREFIXES = (1, 64, 65)
FAR = np.array([0, 2**40 + 5, 2**62], dtype=np.int64)  # held to contiguous batch-1 calls with first_trial = the index

assert IDS.size == 106 and IDS.min() == FIRST < 2**32 <= IDS.max() == FIRST + RUNS - 1


def rows(res, at=OFFSETS):
    """The rows `at` of a contiguous call's result dict (None entries stay None)."""
    return {k: None if v is None else np.asarray(v)[at] for k, v in res.items()}


def same(got, want, what=""):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
