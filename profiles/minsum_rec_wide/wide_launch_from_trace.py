#!/usr/bin/env python3
"""The narrow and the wide variable launch of the record form, from a kernel trace (rocprofv3 --kernel-trace, CSV).

    python profiles/minsum_rec_wide/wide_launch_from_trace.py TRACE_DIR

The wide launch is k_var<64, P> in its record mode, the same kernel name as the message form's variable pass, so the two
are told apart by the GRID: the wide launch runs over the blocks of the (32, 64] bucket alone (a handful), the message form
over every column record.  Prints, per kernel name and grid, calls and the mean / median / min / max duration in us, for
the variable and check kernels of the tile path."""
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kernel_census  # noqa: E402


def main():
    rows = {}
    for root, _, files in os.walk(sys.argv[1]):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                with open(os.path.join(root, f), newline="") as fh:
                    for r in csv.DictReader(fh):
                        grid = "x".join(str(int(r[k]) // max(int(r.get(w, 1) or 1), 1)) for k, w in
                                        (("Grid_Size_X", "Workgroup_Size_X"), ("Grid_Size_Y", "Workgroup_Size_Y")))
                        rows.setdefault((r["Kernel_Name"], grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    names = sorted({n for n, _ in rows})
    key = dict(zip(names, kernel_census.keys_of(names)))
    print("kernel | grid (blocks x tiles) | calls | mean us | median us | min us | max us")
    for (n, grid), d in sorted(rows.items(), key=lambda kv: (key[kv[0][0]], kv[0][1])):
        if key[n].startswith(("k_var", "k_check_minsum")):
            print(f"{key[n]} | {grid} | {len(d)} | {statistics.mean(d):.2f} | {statistics.median(d):.2f} | {min(d):.2f} | {max(d):.2f}")


if __name__ == "__main__":
    main()
