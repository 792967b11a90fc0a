#!/usr/bin/env python3
"""Kernel census: which kernel instantiations of the built libscaldpc.so does the GPU suite launch?

More than half of the library's kernels are template instantiations picked at run time (row / column cap, first pass,
fused test, prior source, ...), and the suite is organised by feature, not by instantiation.  This tool makes "has this
instantiation ever produced a number that was compared with anything?" answerable as far as a tool can: it lists the
kernels of the library, reduces profiler kernel traces of the GPU test files to the same names, and merges both into
tests/golden/kernel_census.json, which tests/test_kernel_census.py holds against the built library.

A kernel is named by its KEY: the demangled name with its template arguments, without the anonymous-namespace prefix and
without the parameter list, e.g. `k_check_tanh<16, true, false, SoftPrior>` -- so a change to a kernel's parameter list
does not invalidate the census.

  symbols [LIB]                         the keys of the library, one per line (no GPU needed)
  reduce DIR --test-file NAME [-o OUT]  read EVERY kernel-trace / stats CSV under DIR (child processes that tests start
                                        write files of their own) -> {"test_file": NAME, "kernels": {key: dispatches}}
  merge PART.json ... [-o OUT] [--lib LIB] [--keep OLD.json]
                                        the per-file sets -> the census: every key of the library with the files that
                                        launched it and its dispatch count; `held_by` and `waiver` entries written by
                                        hand are kept from OLD (default: the output file, if it exists)

What the tool cannot see: whether the test file that launched a kernel compares its output with anything.  `held_by` is
therefore written by hand where a test was added for an instantiation, and is otherwise just the first file of
`launched_by`.  How the traces are taken: profiles/kernel_census/README.md.
"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_lint  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "..", "sca-ldpc_amd", "libscaldpc.so")
DEFAULT_CENSUS = os.path.join(HERE, "..", "tests", "golden", "kernel_census.json")
ANON = "(anonymous namespace)::"


def demangler():
    """Path of c++filt or llvm-cxxfilt, or None."""
    for name in ("c++filt", "llvm-cxxfilt"):
        path = shutil.which(name) or (os.path.join(isa_lint.LLVM_BIN, name) if os.path.exists(os.path.join(isa_lint.LLVM_BIN, name)) else None)
        if path:
            return path
    return None


def demangle(names):
    """Mangled names -> demangled ones (names that are not mangled come back as they are)."""
    names = list(names)
    if not names:
        return []
    filt = demangler()
    if filt is None:
        raise RuntimeError("neither c++filt nor llvm-cxxfilt found")
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    lines = out.split("\n")[: len(names)]
    assert len(lines) == len(names)
    return lines


def key_of(demangled):
    """`void (anonymous namespace)::k_var<16, (anonymous namespace)::SoftPrior>(float*, ...)` -> `k_var<16, SoftPrior>`."""
    s = demangled.strip().replace(ANON, "")
    if s.endswith(".kd"):
        s = s[:-3]
    depth = 0
    for i, ch in enumerate(s):  # the parameter list: the first parenthesis outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            s = s[:i]
            break
    s = s.strip()
    # a function template's demangled name leads with its return type
    depth = 0
    for i in range(len(s) - 1, -1, -1):
        ch = s[i]
        if ch == ">":
            depth += 1
        elif ch == "<":
            depth -= 1
        elif ch == " " and depth == 0:
            s = s[i + 1:]
            break
    return s


def keys_of(names):
    """Kernel names as a symbol table or a profiler gives them (mangled or not, with or without `.kd`) -> keys."""
    stripped = [n[:-3] if n.endswith(".kd") else n for n in names]
    return [key_of(d) for d in demangle(stripped)]


def library_keys(so_path):
    """The keys of every kernel in the gfx950 code objects of the library (sorted, unique)."""
    readelf = os.path.join(isa_lint.LLVM_BIN, "llvm-readelf")
    mangled = set()
    with tempfile.TemporaryDirectory() as wd:
        for s in isa_lint.extract_code_objects(so_path, wd):
            co = s[:-2]  # (the code object beside its disassembly)
            text = subprocess.run([readelf, "--symbols", "--wide", co], check=True, capture_output=True, text=True).stdout
            for line in text.splitlines():
                parts = line.split()
                if parts and parts[-1].endswith(".kd"):
                    mangled.add(parts[-1])
    return sorted(set(keys_of(sorted(mangled))))


def reduce_dir(directory):
    """{key: dispatches} over every kernel-trace CSV under `directory` (stats CSVs where a run left no trace)."""
    traces, stats = [], []
    for root, _, files in os.walk(directory):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                traces.append(os.path.join(root, f))
            elif f.endswith("kernel_stats.csv"):
                stats.append(os.path.join(root, f))
    counts = {}
    traced_dirs = {os.path.dirname(p) for p in traces}
    for path in traces:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name")
                if name:
                    counts[name] = counts.get(name, 0) + 1
    for path in stats:
        if os.path.dirname(path) in traced_dirs:
            continue  # (the same dispatches, already counted one by one)
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name")
                if name:
                    counts[name] = counts.get(name, 0) + int(row.get("Calls") or 0)
    names = sorted(counts)
    out = {}
    for name, key in zip(names, keys_of(names)):
        out[key] = out.get(key, 0) + counts[name]
    return out, len(traces), len(stats)


def merge(parts, lib_keys, old):
    """parts: [{"test_file", "kernels"}] -> the census over `lib_keys` (kernels of other libraries in a trace -- torch's
    own -- are left out)."""
    census = {}
    for key in lib_keys:
        files = sorted(p["test_file"] for p in parts if key in p["kernels"])
        total = sum(p["kernels"].get(key, 0) for p in parts)
        was = old.get(key, {})
        held = was.get("held_by") if "::" in (was.get("held_by") or "") else None  # a test id: written by hand
        census[key] = {"launched_by": files, "dispatches": total, "held_by": held or (files[0] if files else None),
                       "waiver": was.get("waiver")}
    return census


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("symbols")
    a.add_argument("lib", nargs="?", default=DEFAULT_LIB)
    a = sub.add_parser("reduce")
    a.add_argument("dir")
    a.add_argument("--test-file", required=True)
    a.add_argument("-o", "--output")
    a = sub.add_parser("merge")
    a.add_argument("parts", nargs="+")
    a.add_argument("-o", "--output", default=DEFAULT_CENSUS)
    a.add_argument("--lib", default=DEFAULT_LIB)
    a.add_argument("--keep")
    args = ap.parse_args(argv)
    if args.cmd == "symbols":
        keys = library_keys(args.lib)
        print("\n".join(keys))
        print(f"{len(keys)} keys", file=sys.stderr)
        return 0
    if args.cmd == "reduce":
        kernels, ntrace, nstats = reduce_dir(args.dir)
        text = json.dumps({"test_file": args.test_file, "kernels": kernels}, indent=1, sort_keys=True)
        if args.output:
            with open(args.output, "w") as fh:
                fh.write(text + "\n")
        else:
            print(text)
        print(f"{args.test_file}: {len(kernels)} kernels, {sum(kernels.values())} dispatches from {ntrace} trace and "
              f"{nstats} stats files", file=sys.stderr)
        return 0
    parts = []
    for p in args.parts:
        with open(p) as fh:
            parts.append(json.load(fh))
    keep = args.keep or args.output
    old = {}
    if os.path.exists(keep):
        with open(keep) as fh:
            old = json.load(fh)
    census = merge(parts, library_keys(args.lib), old)
    with open(args.output, "w") as fh:
        fh.write(json.dumps(census, indent=1, sort_keys=True) + "\n")
    unreached = [k for k, v in census.items() if not v["launched_by"] and not v["waiver"]]
    print(f"{len(census)} keys, {len(unreached)} launched by no file and not waived", file=sys.stderr)
    for k in unreached:
        print("UNREACHED", k, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
