#!/usr/bin/env python3
"""Are the kernels of two ISA listings (`make -C ceng795_amd/csrc isa`) the same code?

    tools/isa_same.py before.s after.s

Per kernel symbol, the instruction lists are compared after dropping comments, directives and
label lines and replacing every basic-block label (.LBB<i>_<j>) with one token, so a kernel that
merely moved within the file compares equal.  Exit status 0: the same kernels, all equal."""
import re
import sys


def kernels(path):
    """kernel symbol -> its normalised instruction list"""
    out, entry, cur = {}, set(), None
    for line in open(path):
        line = line.split(";")[0].strip()
        if line.startswith(".amdhsa_kernel "):
            entry.add(line.split()[1])
        if not line or line.startswith("//"):
            continue
        if line.endswith(":"):
            if line.startswith(".Lfunc_end"):
                cur = None
            elif not line.startswith(".L"):
                cur = out.setdefault(line[:-1], [])
            continue
        if line.startswith(".") or cur is None:
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", " ".join(line.split())))
    return {k: v for k, v in out.items() if k in entry}


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    differ = sorted(k for k in ka.keys() & kb.keys() if ka[k] != kb[k])
    for k in sorted(ka.keys() ^ kb.keys()):
        print("only in", a if k in ka else b, k)
    for k in differ:
        print("differs", k, len(ka[k]), "->", len(kb[k]), "instructions")
    same = ka.keys() == kb.keys() and not differ
    print(f"{len(ka)} / {len(kb)} kernels, {sum(map(len, ka.values()))} / "
          f"{sum(map(len, kb.values()))} instructions:", "identical" if same else "NOT identical")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
