#!/usr/bin/env python3
"""Are the kernels of two ISA listings (`make -C ceng795_amd/csrc isa`) the same code?

    tools/isa_same.py before.s after.s [--appended-flag]

Per kernel symbol, the instruction lists are compared after dropping comments, directives and
label lines and replacing every basic-block label (.LBB<i>_<j>) with one token, so a kernel that
merely moved within the file compares equal.  Exit status 0: the same kernels, all equal.

--appended-flag: `after` gave some kernel templates one more bool parameter at the end (a new
compile-time variant, as SMOOTH).  An instantiation of `after` whose new flag is false is compared
with the instantiation of `before` that has the same name and the same flags before it; those
whose new flag is true are listed as new and counted apart.  Exit status 0: every kernel of
`before` has its counterpart and all are equal."""
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


def variant(symbol):
    """(name, bool template arguments) of a mangled rt:: kernel template instantiation, or None."""
    m = re.match(r"_ZN2rt(\d+)", symbol)
    if not m:
        return None
    name = symbol[m.end():m.end() + int(m.group(1))]
    # (the bools may be followed by a parameter pack, J...E, before the list's closing E)
    flags = re.match(r"I((?:Lb[01]E)+)[EJ]", symbol[m.end() + len(name):])
    if not flags:
        return None
    return name, tuple(int(x) for x in re.findall(r"Lb([01])E", flags.group(1)))


def rename_appended(ka, kb):
    """kb with its flag-appended flat instantiations under their names in ka; the new ones apart."""
    before = {variant(k): k for k in ka if k not in kb and variant(k)}
    renamed, new = {}, {}
    for k, v in kb.items():
        var = None if k in ka else variant(k)
        if var and (var[0], var[1][:-1]) in before:
            if var[1][-1] == 0:
                renamed[before[(var[0], var[1][:-1])]] = v
            else:
                new[k] = v
        else:
            renamed[k] = v
    return renamed, new


def main(a, b, *options):
    ka, kb = kernels(a), kernels(b)
    new = {}
    if "--appended-flag" in options:
        kb, new = rename_appended(ka, kb)
    differ = sorted(k for k in ka.keys() & kb.keys() if ka[k] != kb[k])
    for k in sorted(ka.keys() ^ kb.keys()):
        print("only in", a if k in ka else b, k)
    for k in differ:
        print("differs", k, len(ka[k]), "->", len(kb[k]), "instructions")
    # (with --appended-flag, kernels that only `after` has are additions, not differences)
    same = (ka.keys() <= kb.keys() if "--appended-flag" in options else ka.keys() == kb.keys()) \
        and not differ
    print(f"{len(ka)} / {len(kb)} kernels, {sum(map(len, ka.values()))} / "
          f"{sum(map(len, kb.values()))} instructions:", "identical" if same else "NOT identical")
    if new:
        print(f"{len(new)} new instantiations with the appended flag set, "
              f"{sum(map(len, new.values()))} instructions")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
