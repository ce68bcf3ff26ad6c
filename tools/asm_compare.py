#!/usr/bin/env python3
"""Compares the gfx950 kernels of two sets of assembly files (hipcc ... --cuda-device-only -S), kernel by kernel.

    python tools/asm_compare.py --before old.s --after a.s b.s c.s

Kernels are matched by mangled name; a kernel's text is its instruction lines plus its .amdhsa_* block.  Dropped before
comparing: comments, .file / .ident, the __hip_cuid_* symbol and the function index <n> inside the local labels
.LBB<n>_<m> / .LJTI<n>_<m> (it changes when a kernel moves to another file; the block index <m> is kept).  Text only:
nothing is compiled or run.  Exit status 0 iff both sides hold the same kernels with the same text.
"""
import argparse
import re
import sys

_LOCAL = re.compile(r"\.L(BB|JTI)\d+_")


def _clean(line):
    line = line.split(";", 1)[0].strip()
    if not line or line.startswith((".file", ".ident")) or "__hip_cuid_" in line:
        return None
    return _LOCAL.sub(lambda m: ".L" + m.group(1) + "_", line)


def kernels(paths):
    """{mangled name: [cleaned lines of the body and of the .amdhsa_kernel block]}"""
    out = {}
    for path in paths:
        lines = open(path).read().splitlines()
        names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            if name in out:
                sys.exit("kernel defined twice: " + name)
            start = lines.index(name + ":") if name + ":" in lines else next(
                i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
            out[name] = [c for c in map(_clean, lines[start:end + 1]) if c is not None]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--show", type=int, default=6, help="differing lines printed per kernel")
    a = ap.parse_args()
    old, new = kernels(a.before), kernels(a.after)
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differing = []
    for name in sorted(set(old) & set(new)):
        if old[name] != new[name]:
            differing.append(name)
            print("DIFFERS %s (%d -> %d lines)" % (name, len(old[name]), len(new[name])))
            shown = 0
            for x, y in zip(old[name], new[name]):
                if x != y and shown < a.show:
                    print("    - %s\n    + %s" % (x, y))
                    shown += 1
    for name in missing:
        print("MISSING " + name)
    for name in added:
        print("ADDED   " + name)
    print("%d kernels before, %d after, %d missing, %d added, %d differing" %
          (len(old), len(new), len(missing), len(added), len(differing)))
    return 1 if (missing or added or differing) else 0


if __name__ == "__main__":
    sys.exit(main())
