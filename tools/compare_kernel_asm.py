#!/usr/bin/env python3
"""Compare the device code of two builds of cpecan_kernels.hip, kernel by kernel.

    make -C cpecan_amd/csrc asm                  # in each tree: cpecan_kernels.s (hipcc -S --cuda-device-only)
    python tools/compare_kernel_asm.py OLD.s NEW.s [--added-false-arg FAMILY]

A change that only moves host code (the launch plan, the kernel table) must leave every kernel as it was, but the order in
which the templates are instantiated may move, and with it the function index in the local labels (.LBB<n>_<m>,
.Lfunc_end<n>, .Ltmp<n>) and in the compiler's comments.  So both files are cut into one body per function symbol -- code, .amdhsa_* resource lines and
the compiler's resource comments -- and into one metadata entry per kernel; the indices are normalised, and the pieces are
compared symbol by symbol.  It only splits and compares text.  Exit status 0: same symbols, every piece identical.

--added-false-arg FAMILY: NEW gave the kernel template FAMILY one more `bool` parameter at the end, false by default (GANG of
cpecan_pairhmm_sweep).  The instantiations with false there are the old kernels under a longer mangled name: that last
argument is dropped from their names in NEW before comparing, so they are compared with their old selves, and the ones
with true there show as only in the second without counting against the exit status."""
import re
import sys

FAMILIES = ("cpecan_pairhmm_sweep", "cpecan_pairhmm_packed", "cpecan_pairhmm_team")
BEGIN = re.compile(r"; -- Begin function (\S+)")
INDEXED = re.compile(r"(\.L|\b)(BB|JTI)\d+(?=_\d)|(\.L)(func_begin|func_end)\d+")  # in code and in the compiler's loop comments
TMP = re.compile(r"\.Ltmp\d+")


def normalise(lines):
    seen = {}
    out = []
    for line in lines:
        line = re.sub(r"\s+;", " ;", INDEXED.sub(lambda m: "%s%s#" % (m.group(1) or m.group(3), m.group(2) or m.group(4)), line))  # (comment column: label widths)
        out.append(TMP.sub(lambda m: ".Ltmp%d" % seen.setdefault(m.group(0), len(seen)), line))
    return out


def pieces(path, added_false_arg=None):
    """{symbol: normalised lines of its function body}, {symbol: lines of its metadata entry}"""
    bodies, meta, name, cur = {}, {}, None, None
    entry, in_meta = None, False
    # (Itanium mangling: _Z<len><name>I<template arguments>E<signature>; a false bool argument is Lb0E)
    longer = re.compile(r"(_Z\d+%s\w*?)Lb0EEv" % re.escape(added_false_arg)) if added_false_arg else None
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if longer:
                line = longer.sub(r"\1Ev", line)
            if in_meta:
                if line.startswith("  - ") or not line.startswith("   "):  # the next kernel's entry, or the end of the list
                    if entry:
                        sym = [l.split()[-1] for l in entry if l.strip().startswith(".symbol:")][0][:-3]
                        meta[sym] = entry
                    if not line.startswith("  - "):
                        break
                    entry = [line]
                else:
                    entry.append(line)
                continue
            if line.startswith("amdhsa.kernels:"):
                in_meta = True
                continue
            m = BEGIN.search(line)
            if m or ".AMDGPU.gpr_maximums" in line:
                if name:
                    while cur[-1].startswith(("\t.text", "\t.section\t.text")):  # the section of the NEXT function
                        cur.pop()
                    bodies[name] = normalise(cur)
                name, cur = (m.group(1), []) if m else (None, None)
            if name:
                cur.append(line)
    return bodies, meta


def main():
    added = None
    if len(sys.argv) == 5 and sys.argv[3] == "--added-false-arg":
        added = sys.argv[4]
    elif len(sys.argv) != 3:
        sys.exit(__doc__)
    (b0, m0), (b1, m1) = pieces(sys.argv[1]), pieces(sys.argv[2], added)
    ok = True
    for what, old, new in (("function bodies", b0, b1), ("kernel metadata entries", m0, m1)):
        only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
        print("%s: %d / %d, only in the first %d, only in the second %d, different %d, identical %d" %
              (what, len(old), len(new), len(only_old), len(only_new), len(differ), len(set(old) & set(new)) - len(differ)))
        for s in only_old + only_new + differ:
            print("  %s %s" % ("-" if s in only_old else "+" if s in only_new else "!", s))
        if added:  # the instantiations with true in the added argument are new by design
            only_new = [s for s in only_new if not re.match(r"_Z\d+%s\w*Lb1EEv" % re.escape(added), s)]
        ok = ok and not (only_old or only_new or differ)
    for which, meta in (("first", m0), ("second", m1)):
        counts = [sum(1 for s in meta if fam in s) for fam in FAMILIES]
        print("kernels of the %s: %d = %s, others %d" % (which, len(meta), " / ".join(
            "%d %s" % (c, fam) for c, fam in zip(counts, FAMILIES)), len(meta) - sum(counts)))
    print("lines compared: %d / %d" % (sum(map(len, b0.values())) + sum(map(len, m0.values())),
                                        sum(map(len, b1.values())) + sum(map(len, m1.values()))))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
