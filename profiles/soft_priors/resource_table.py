#!/usr/bin/env python3
"""Kernel resource usage of a build as a table, and the difference between two builds.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> -Rpass-analysis=kernel-resource-usage \
          -c -o /dev/null scaldpc_bp.hip 2> remarks.txt            (no GPU needed)
    resource_table.py remarks.txt > table.tsv
    resource_table.py parent_remarks.txt new_remarks.txt > diff.txt

The table has one line per kernel (demangled name), sorted by name: SGPRs, VGPRs, AGPRs, scratch bytes per lane,
occupancy, SGPR spills, VGPR spills, LDS bytes.  The difference lists kernels that changed, left and came.
"""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        line = re.sub(r"^remark: \S+:\d+:\d+:", "remark:", line)  # (a compiler that prefixes the remark with file:line:col)
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    table = {}
    for mangled, name in zip(names, dem):
        name = name.replace("(anonymous namespace)::", "")
        name = re.sub(r"\(.*$", "", name)  # arguments: the template arguments identify the instantiation
        table[name] = tuple(out[mangled].get(f, "?") for f in FIELDS)
    return table


def main():
    if len(sys.argv) == 2:
        print("kernel\t" + "\t".join(FIELDS))
        for k, v in sorted(parse(sys.argv[1]).items()):
            print(k + "\t" + "\t".join(v))
        return 0
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    changed = [k for k in sorted(a) if k in b and a[k] != b[k]]
    print(f"kernels: {len(a)} before, {len(b)} after; {len(changed)} changed, {len(set(a) - set(b))} gone, {len(set(b) - set(a))} new")
    print("columns: " + ", ".join(FIELDS))
    for k in changed:
        print(f"CHANGED {k}\n    before {a[k]}\n    after  {b[k]}")
    for k in sorted(set(a) - set(b)):
        print(f"GONE    {k}  {a[k]}")
    for k in sorted(set(b) - set(a)):
        print(f"NEW     {k}  {' '.join(b[k])}")
    return 1 if changed or set(a) - set(b) else 0


if __name__ == "__main__":
    sys.exit(main())
