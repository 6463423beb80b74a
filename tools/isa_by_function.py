#!/usr/bin/env python3
"""Hash a hipcc -S --cuda-device-only listing function by function, so that two builds can be compared
when functions were added or removed between them.

    isa_by_function.py FILE.s                 prints `name sha256` per function, sorted, then the count and one hash of that list
    isa_by_function.py PARENT.s HEAD.s [NAME] prints the functions only in one side and those whose text differs;
                                              with NAME, that function's normalised text as a unified diff as well

Normalisation: the listing is cut at the `name: ; @name` labels and ends at .amdgpu_metadata; the preamble directives and the
__hip_cuid_ line go; trailing comments go, whole-line comments (register and scratch figures) stay; the function's ordinal
in local labels (.LBB<n>_, BB<n>_, .Lfunc_end<n>, .Lpost_getpc<n>) becomes N."""
import difflib
import hashlib
import re
import sys

START = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$")
PREAMBLE = re.compile(r"^\s*\.(globl|protected|type|p2align|text)\b")
ORDINAL = re.compile(r"(\.?LBB|\bBB|\.Lfunc_end|\.Lpost_getpc)\d+")


def functions(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        if ".amdgpu_metadata" in line:
            break
        m = START.match(line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None or PREAMBLE.match(line) or "__hip_cuid_" in line:
            continue
        if not line.lstrip().startswith(";"):
            line = line.split(";", 1)[0]
        line = ORDINAL.sub(lambda g: g.group(1) + "N", line.rstrip())
        if line:
            out[name].append(line)
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main(argv):
    if len(argv) == 2:
        rows = sorted("%s %s" % (n, digest(t)) for n, t in functions(argv[1]).items())
        print("\n".join(rows))
        print("functions %d  sha256(list) %s" % (len(rows), digest(rows)))
        return 0
    a, b = functions(argv[1]), functions(argv[2])
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if digest(a[n]) != digest(b[n]))
    same = sorted("%s %s" % (n, digest(b[n])) for n in set(a) & set(b) if n not in differ)
    print("parent %d  head %d  equal %d  sha256(equal list) %s" % (len(a), len(b), len(same), digest(same)))
    print("only in parent (%d): %s" % (len(gone), " ".join(gone)))
    print("only in head (%d): %s" % (len(new), " ".join(new)))
    print("differ (%d): %s" % (len(differ), " ".join(differ)))
    if len(argv) > 3 and argv[3] in a and argv[3] in b:
        sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[argv[3]], b[argv[3]], "parent", "head", lineterm=""))
    return 0 if not new and not differ else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
