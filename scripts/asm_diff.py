#!/usr/bin/env python3
"""Compare the device code of two directories of `make asm` listings (build/*.s), function by function.

    python3 scripts/asm_diff.py OLD_DIR NEW_DIR

A function is matched by its mangled symbol, whichever file of a directory holds it: its instructions and, for a
kernel, its .amdhsa_kernel block.  Comments and debug directives are dropped, and the per-file function number
in local labels (.LBB20_7, .Lfunc_end20, .LJTI20_0) is removed, so moving a function between files changes
nothing.  Prints the symbols that differ and those on one side only; exit status 1 if there are any.
"""
import glob
import os
import re
import sys

START = re.compile(r"^([A-Za-z_$][\w$.]*):")
SKIP = re.compile(r"^\.(loc|file|cfi_\w+|section|text|ident)\b")
NUM = re.compile(r"(\.L[A-Za-z_]*[A-Za-z])\d+(_\d+)\b")
FUNC = re.compile(r"\.Lfunc_(begin|end)\d+")


def functions(directory):
    """symbol -> (is_kernel, normalised lines) over every .s file of `directory`."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        sym, typed, body = None, set(), []
        for raw in open(path, errors="replace"):
            line = " ".join(raw.split(";", 1)[0].split())
            if not line:
                continue
            if line.startswith(".type ") and line.endswith(",@function"):
                typed.add(line[6:].split(",")[0])
            m = START.match(line)
            if sym is None:
                if m and m.group(1) in typed:
                    sym, body = m.group(1), []
                continue
            if line.startswith(".size " + sym + ","):
                if sym in out and out[sym][1] != body:   # (a library's kernel instantiated in two files: one copy)
                    sys.exit(f"{directory}: {sym} has two definitions that differ")
                out[sym] = (any(b.startswith(".amdhsa_kernel ") for b in body), body)
                sym = None
            elif not SKIP.match(line):
                body.append(FUNC.sub(r".Lfunc_\1", NUM.sub(r"\1\2", line)))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            print(f"only in {sys.argv[1] if sym in old else sys.argv[2]}: {sym}")
        elif old[sym][1] != new[sym][1]:
            a, b = old[sym][1], new[sym][1]
            n = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            print(f"differs: {sym} ({'kernel' if new[sym][0] else 'function'}, {len(a)} -> {len(b)} lines, "
                  f"{n} differ in place)")
        else:
            continue
        bad += 1
    print(f"{len(old)} / {len(new)} functions, {sum(k for k, _ in new.values())} kernels compared, {bad} differ or are unmatched",
          file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
