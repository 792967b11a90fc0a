#!/usr/bin/env python3
"""Are the device code objects of two builds of libscaldpc.so the same bytes?  (no GPU needed)

    python3 profiles/mc_entries/compare_code_objects.py PARENT/libscaldpc.so CHANGE/libscaldpc.so

Prints size and SHA-256 of every gfx950 code object of both libraries (profiles/isa_lint.extract_code_objects unbundles
them) and exits 1 where a pair differs."""
import hashlib
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import isa_lint  # noqa: E402


def code_objects(so_path):
    with tempfile.TemporaryDirectory() as wd:
        out = []
        for s in isa_lint.extract_code_objects(so_path, wd):
            with open(s[:-2], "rb") as fh:  # (the object next to its disassembly)
                blob = fh.read()
            out.append((os.path.basename(s[:-2]), len(blob), hashlib.sha256(blob).hexdigest()))
        return out


def main():
    parent, change = code_objects(sys.argv[1]), code_objects(sys.argv[2])
    same = len(parent) == len(change)
    for i, (p, c) in enumerate(zip(parent, change)):
        print(f"code object {i}  parent {p[1]:>9} B sha256 {p[2]}\n               change {c[1]:>9} B sha256 {c[2]}  "
              f"{'same' if p[1:] == c[1:] else 'DIFFERENT'}")
        same = same and p[1:] == c[1:]
    print("identical" if same else f"NOT identical ({len(parent)} and {len(change)} code objects)")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
