#!/usr/bin/env python3
"""Compare two builds' gfx950 device assembly kernel by kernel.

    make -C distml_amd/csrc asm            # build/asm/<unit>.s, in each of two checkouts
    scripts/compare_device_asm.py A/distml_amd/csrc/build/asm B/distml_amd/csrc/build/asm

Each argument is a directory of .s files (hipcc --cuda-device-only -S with the Makefile's
flags, one file per translation unit). A kernel is a symbol with an .amdhsa_kernel block.
Two things are compared per kernel symbol, wherever its unit:

  * the instruction lines of its body: comments, blank lines and assembler directives
    dropped, local labels (.LBB<function>_<n> and the like) renumbered in order of first
    appearance, because a function's ordinal changes when it moves to another file;
  * its .amdhsa_* descriptor block (register counts, LDS, scratch and the rest).

Prints one verdict per kernel that is not identical (-v: per kernel), then one summary
line. Exit status 0 when both builds define the same kernels, each once, all identical.
"""
import difflib
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")


def _renumber(lines):
    names = {}
    return [LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l) for l in lines]


def kernels_of(path):
    """{symbol: (body lines, descriptor lines)} of one .s file."""
    out = {}
    lines = open(path, errors="replace").read().split("\n")
    starts = {}  # symbol -> line index of its label
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m:
            starts.setdefault(m.group(1), i)
    for i, l in enumerate(lines):
        m = KERNEL.match(l)
        if not m or m.group(1) not in starts:
            continue
        sym = m.group(1)
        desc = []
        for d in lines[i + 1:]:
            if d.strip().startswith(".end_amdhsa_kernel"):
                break
            desc.append(" ".join(d.split(";")[0].split()))
        body = []
        for b in lines[starts[sym] + 1:]:
            if FUNC_END.match(b):
                break
            b = b.split(";")[0].strip()
            if not b or (b.startswith(".") and not b.endswith(":")):
                continue  # comment, blank or directive (local labels end with ':')
            body.append(" ".join(b.split()))
        out[sym] = (_renumber(body), [d for d in desc if d])
    return out


def build_of(directory):
    """({symbol: (unit, body, descriptor)}, [symbols defined in two units])."""
    ks, twice = {}, {}
    for p in sorted(glob.glob(os.path.join(directory, "*.s"))):
        unit = os.path.basename(p)
        for sym, (body, desc) in kernels_of(p).items():
            if sym in ks:
                twice[sym] = "%s, %s" % (ks[sym][0], unit)
            ks[sym] = (unit, body, desc)
    return ks, twice


def short(sym):
    return sym if len(sym) <= 120 else sym[:117] + "..."


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv[1:] if a != "-v"]
    if len(dirs) != 2:
        sys.exit(__doc__)
    (a, twice_a), (b, twice_b) = build_of(dirs[0]), build_of(dirs[1])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    same = differ = 0
    for sym in sorted(set(a) & set(b)):
        (ua, ba, da), (ub, bb, db) = a[sym], b[sym]
        what = [w for w, x, y in (("body", ba, bb), ("descriptor", da, db)) if x != y]
        if not what:
            same += 1
            if verbose:
                print("identical   %s (%s -> %s)" % (sym, ua, ub))
            continue
        differ += 1
        print("DIFFERS     %s (%s -> %s): %s" % (short(sym), ua, ub, ", ".join(what)))
        for w, x, y in (("body", ba, bb), ("descriptor", da, db)):
            if x != y:
                d = list(difflib.unified_diff(x, y, "a", "b", lineterm="", n=0))
                print("    %s: %d -> %d lines, %d diff lines" % (w, len(x), len(y), len(d) - 2))
                for l in d[2:12]:
                    print("      " + l)
    for s in only_a:
        print("ONLY IN A   %s (%s)" % (short(s), a[s][0]))
    for s in only_b:
        print("ONLY IN B   %s (%s)" % (short(s), b[s][0]))
    # a library template both builds instantiate in the same two units (rocprim's, as
    # comdat) is no finding; a kernel that B alone defines twice is
    twice_new = sorted(s for s in twice_b if twice_b[s] != twice_a.get(s))
    for s in twice_new:
        print("TWICE IN B  %s (%s)" % (short(s), twice_b[s]))
    print("kernels compared %d, identical %d, differing %d; only in A %d, only in B %d; "
          "defined in two units: A %d, B %d, new in B %d"
          % (same + differ, same, differ, len(only_a), len(only_b), len(twice_a), len(twice_b), len(twice_new)))
    return 0 if not (differ or only_a or only_b or twice_new) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
