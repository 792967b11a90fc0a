"""Mean kernel time per PASS of a tile group from a rocprofv3 kernel trace of bench.py: a group of a stream is what lies between
two k_var_first launches; its n-th steady k_check_minsum_rec is check pass 3 + n, its n-th k_var_rec (not <last>) variable
pass 2 + n.  The last step of the trace (from its k_pack_bits on) is taken."""
import collections
import csv
import re
import sys


def kind(name):
    m = re.search(r"(k_\w+)(<[^>]*>)?", name)
    if not m:
        return name
    k, t = m.group(1), m.group(2) or ""
    if k == "k_var_rec":
        return "var_last" if t.rstrip(">").endswith("true") else "var"
    if k == "k_check_minsum_rec":
        return "boot" if t.split(",")[1].strip() == "true" else "check"
    return k


rows = list(csv.DictReader(open(sys.argv[1])))
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Stream_Id"], kind(r["Kernel_Name"])) for r in rows)
first = max(i for i, e in enumerate(ev) if e[3] == "k_pack_bits")
ev = ev[first:]
per = collections.defaultdict(list)
count = {}
for s, e, stream, k in ev:
    if k == "k_var_first":
        count[stream] = {"check": 0, "var": 0}
    elif k in ("check", "var") and stream in count:
        p = count[stream][k] + (3 if k == "check" else 2)
        count[stream][k] += 1
        per[(k, p)].append((e - s) / 1e3)
print(sys.argv[1])
for (k, p), v in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0] == "var")):
    print(f"  {k:5s} pass {p:2d}: {len(v):4d} launches, mean {sum(v) / len(v):6.2f} us, min {min(v):6.2f}, max {max(v):6.2f}")
