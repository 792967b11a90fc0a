#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds of scaldpc_bp.hip from their device assembly.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --save-temps -c -o scaldpc_bp.o scaldpc_bp.hip     (no GPU needed)
    compare_asm.py parent/scaldpc_bp-hip-amdgcn-amd-amdhsa-gfx950.s new/scaldpc_bp-hip-amdgcn-amd-amdhsa-gfx950.s

Kernels of the parent are matched to this commit's by name: a plain prior-consuming kernel gains `SharedPrior` as its
last template argument, a `_soft` twin becomes the same base name with `SoftPrior` (and the FIRST / PAR / PLANES values
its wrapper used to hard-wire).  For each pair the instruction streams are compared with block labels renumbered in
order of appearance (`.LBBn_m` and the `.Lpost_getpcN` of long branches):
    identical   every instruction and operand equal
    operands    same number of instructions, same opcode at every position; operands differ (kernarg offsets, registers)
    DIFFERENT   anything else

    compare_asm.py --tables resource_usage_parent.tsv resource_usage_new.tsv
the same matching applied to two tables of profiles/soft_priors/resource_table.py: kernels whose figures changed, left, came.
"""
import re
import subprocess
import sys

PRIOR_KERNELS = ("k_init_msg", "k_check_minsum", "k_check_minsum_x", "k_check_tanh", "k_bp_small", "k_var", "k_var_rec",
                 "k_el_check", "k_el_var")
SOFT_FILL = {  # template arguments the parent's `_soft` wrapper fixed, in the merged kernel's order: {} = the wrapper's own
    "k_init_msg": "", "k_check_minsum": "true", "k_check_minsum_x": "{}, true, false", "k_check_tanh": "{}, true, false",
    "k_bp_small": "{}, false", "k_var": "{}", "k_var_rec": "{}", "k_el_check": "{}, true", "k_el_var": "",
}


def kernels(path):
    """{demangled name: [instruction lines]} of the .amdhsa_kernel symbols of an assembly file."""
    text = open(path, errors="replace").read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(names, dem):
        name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
        body = text.split("\n" + mangled + ":", 1)[1].split(".Lfunc_end", 1)[0]
        ins, labels = [], {}
        for line in body.split("\n"):
            line = line.split(";", 1)[0].strip()
            if not line or line.startswith(".") and not line.startswith(".LBB"):
                continue
            ins.append(line)
        def canon(m):
            return labels.setdefault(m.group(0), "L%d" % len(labels))
        out[name] = [re.sub(r"\.LBB\d+_\d+|\.Lpost_getpc\d+", canon, i) for i in ins]
    return out


def new_name(old):
    m = re.match(r"(\w+?)(_soft)?(?:<(.*)>)?$", old)
    base, soft, args = m.group(1), m.group(2), m.group(3)
    if base not in PRIOR_KERNELS:
        return old
    if soft:
        args = SOFT_FILL[base].format(args)
    return "%s<%s>" % (base, ", ".join(x for x in (args, "SoftPrior" if soft else "SharedPrior") if x))


def tables(pa, pb):
    def load(path):
        rows = [line.rstrip("\n").split("\t") for line in open(path)][1:]
        return {r[0].replace("void ", ""): tuple(r[1:]) for r in rows}
    a, b = load(pa), load(pb)
    renamed = {new_name(k): (k, v) for k, v in a.items()}
    changed = [(k, renamed[k]) for k in sorted(b) if k in renamed and renamed[k][1] != b[k]]
    gone = sorted(old for new, (old, _) in renamed.items() if new not in b)
    came = sorted(set(b) - set(renamed))
    print("kernels: %d before, %d after; %d changed, %d gone, %d new" % (len(a), len(b), len(changed), len(gone), len(came)))
    for k, (old, v) in changed:
        print("CHANGED %s (was %s)\n    before %s\n    after  %s" % (k, old, v, b[k]))
    for k in gone:
        print("GONE    %s  %s" % (k, " ".join(a[k])))
    for k in came:
        print("NEW     %s  %s" % (k, " ".join(b[k])))


def main():
    if sys.argv[1] == "--tables":
        return tables(sys.argv[2], sys.argv[3])
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    seen, counts = set(), {}
    for old in sorted(a):
        new = new_name(old)
        if new not in b:
            print("GONE       %s" % old)
            continue
        seen.add(new)
        x, y = a[old], b[new]
        if x == y:
            verdict = "identical"
        elif len(x) == len(y) and all(p.split()[0] == q.split()[0] for p, q in zip(x, y)):
            verdict = "operands "
        else:
            verdict = "DIFFERENT"
        counts[verdict] = counts.get(verdict, 0) + 1
        note = ""
        if verdict == "operands ":
            d = [(p, q) for p, q in zip(x, y) if p != q]
            loads = sum(p.split()[0].startswith("s_load") for p, _ in d)
            note = "  (%d of %d lines differ, %d of them kernarg / scalar loads)" % (len(d), len(x), loads)
        elif verdict == "DIFFERENT":
            note = "  (%d -> %d instructions)" % (len(x), len(y))
        print("%s  %s%s%s" % (verdict, old, "" if old == new else "  ->  " + new, note))
    for new in sorted(set(b) - seen):
        print("NEW        %s" % new)
    print("summary: %d kernels before, %d after; %s" % (len(a), len(b), ", ".join("%d %s" % (v, k.strip()) for k, v in sorted(counts.items()))))


if __name__ == "__main__":
    main()
