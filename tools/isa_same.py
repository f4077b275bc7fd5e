#!/usr/bin/env python3
"""Are two device assembly listings (hipcc --cuda-device-only -S) the same code, function by function?

A host-only edit may reorder the functions of a listing and renumber their local labels, so the files differ
while every function body is identical.  This compares the symbol sets and each function's text between its
"Begin function" and "End function" markers, with the function ordinal stripped from local labels (and the
padding in front of a line's comment, which the printer sizes by the label's length, ordinal included).

usage: isa_same.py PARENT.s NEW.s      exit status 1 on any difference
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.search(r"-- Begin function (\S+)", line)
        if m:
            name, body = m.group(1), []
        elif name and "-- End function" in line:
            out[name], name = "".join(body), None
        elif name:
            line = re.sub(r"BB\d+_(\d+)", r"BB_\1", line)   # (labels, and the comments that name them)
            line = re.sub(r"[ \t]+;", " ;", line)
            body.append(re.sub(r"\.L(func_begin|func_end|tmp|JTI)\d+", r".L\1", line))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    same = len(set(a) & set(b)) - len(differ)
    print(f"{sys.argv[2]}: {same} of {len(a)} functions equal, {len(differ)} differ, "
          f"{len(only_a)} only in parent, {len(only_b)} only in new")
    for title, names in (("differs", differ), ("only in parent", only_a), ("only in new", only_b)):
        for n in names:
            print(f"  {title}: {n}")
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main())
