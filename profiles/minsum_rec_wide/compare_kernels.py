#!/usr/bin/env python3
"""Kernel by kernel: is the gfx950 disassembly of two builds of libscaldpc.so the same?  (no GPU needed)

    python3 profiles/minsum_rec_wide/compare_kernels.py PARENT/libscaldpc.so CHANGE/libscaldpc.so

profiles/mc_entries/compare_code_objects.py compares whole code objects, and a code object that gains a kernel is other
bytes whatever happened to the kernels it already had.  This one unbundles and disassembles both libraries
(profiles/isa_lint: extract_code_objects, parse) and compares, for every kernel of the parent, the instruction stream --
mnemonics and operands in order, branch targets as the relative offsets the encoding holds, no addresses; the literal of
a PC-relative address (s_getpc_b64 + s_add_u32) is left out, since it is a distance across .text.  Prints one
line per kernel that differs, left or came, the verdict for the families named on the command line after the two
libraries (default: k_var_rec< and k_check_minsum_rec<) in full, and exits 1 if a kernel of the parent differs or left."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import isa_lint  # noqa: E402
import kernel_census  # noqa: E402


def kernels(so_path):
    """{key: [instruction text]} over all gfx950 code objects of a library."""
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        raw = {}
        for s in isa_lint.extract_code_objects(so_path, wd):
            for name, insts in isa_lint.parse(s).items():
                text = [t for _, _, _, t in insts]
                # `s_getpc_b64 s[N:N+1]; s_add_u32 sN, sN, LITERAL`: the distance from here to a table in .rodata (k_soft_convert's
                # logf table) -- it moves with the size of .text, the code does not
                for i in range(1, len(text)):
                    if text[i - 1].startswith("s_getpc_b64") and text[i].startswith("s_add_u32"):
                        text[i] = text[i].rsplit(",", 1)[0] + ", <pc-relative>"
                raw[name] = text
        names = sorted(raw)
        for name, dem in zip(names, kernel_census.demangle(names)):
            out[kernel_census.key_of(dem)] = raw[name]
    return out


def main():
    parent, change = kernels(sys.argv[1]), kernels(sys.argv[2])
    families = tuple(sys.argv[3:]) or ("k_var_rec<", "k_check_minsum_rec<")
    differ = sorted(k for k in parent if k in change and parent[k] != change[k])
    gone, came = sorted(set(parent) - set(change)), sorted(set(change) - set(parent))
    print(f"kernels: {len(parent)} in the parent, {len(change)} in the change; {len(differ)} differ, {len(gone)} gone, {len(came)} new")
    for k in differ:
        print(f"DIFFERENT  {k}  ({len(parent[k])} -> {len(change[k])} instructions)")
    for k in gone:
        print(f"GONE       {k}")
    for k in came:
        print(f"NEW        {k}  ({len(change[k])} instructions)")
    print()
    for k in sorted(parent):
        if k.startswith(families):
            verdict = "gone" if k not in change else ("identical" if parent[k] == change[k] else "DIFFERENT")
            print(f"{verdict:10s} {k}  ({len(parent[k])} instructions)")
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
