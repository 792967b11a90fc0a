"""Compare the -Rpass-analysis=kernel-resource-usage remarks of two builds of libscaldpc.so.

    make -C sca-ldpc_amd/csrc ../libscaldpc.so CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" 2> build.log

on the parent commit and on the change, then

    python profiles/mc_trial_list/resource_usage.py parent.log change.log > profiles/mc_trial_list/resource_usage_diff.txt

Every kernel of the library is compared (so a generator whose registers moved cannot hide behind a name); the seven trial
generators, whose bodies became templates over the source of the trial index, are printed in full, with their list forms.
Columns: SGPRs VGPRs AGPRs scratch[B/lane] occupancy[waves/SIMD] SGPR-spill VGPR-spill LDS[B/block].
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")
GENERATORS = ("k_mc_bernoulli", "k_mc_hqc_secret", "k_mc_hqc_outcome", "k_mc_hqc_outcome64", "k_q_mc_draw", "k_q_mc_secret_draw",
              "k_q_mc_secret_sums")


def parse(path):
    names, out, cur = [], {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            names.append(cur)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur and m.group(1) in FIELDS:
            out[cur][m.group(1)] = m.group(2)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", d)
        key = re.sub(r"\(.*$", "", d) if "<" not in d else re.sub(r">\(.*$", ">", d)
        res[key] = " ".join(out[n].get(f, "?") for f in FIELDS)
    return res


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    changed = sorted(k for k in a if k in b and a[k] != b[k])
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print(f"kernels: {len(a)} before, {len(b)} after; {len(changed)} changed, {len(gone)} gone, {len(new)} new")
    for k in changed:
        print(f"CHANGED {k}  {a[k]}  ->  {b[k]}")
    for k in gone:
        print(f"GONE    {k}  {a[k]}")
    for k in new:
        print(f"NEW     {k}  {b[k]}")
    print()
    print("the trial generators (SGPRs VGPRs AGPRs scratch occupancy SGPR-spill VGPR-spill LDS): parent | change | list form")
    for g in GENERATORS:
        for k in sorted(a):
            if re.fullmatch(re.escape(g) + r"(<.*>)?", k):
                at = re.sub(r"^" + re.escape(g), g + "_at", k)
                same = "same" if a[k] == b.get(k) else "DIFFERENT"
                print(f"{k:28s} {a[k]} | {b.get(k, 'missing')} ({same}) | {b.get(at, 'missing')}")


if __name__ == "__main__":
    main()
