#!/usr/bin/env python3
"""Compare the device assembly of two builds function by function (the build keeps it: build/temps/*-hip-amdgcn-amd-amdhsa-gfx950.s).

    python tools/compare_device_asm.py OLD_TEMPS_DIR NEW_TEMPS_DIR

Each translation unit's functions are cut out between their label and .Lfunc_endN; local label numbers, which shift when a function is added
in front of others, are normalised, and so are comment lines.  Prints the functions whose code differs, those only one side has, and the counts
of unchanged / changed / new / removed functions.  Exit status 1 if any function of the old build changed or is missing."""
import glob
import os
import re
import sys

_LOCAL = re.compile(r"\.(LBB|Lfunc_end|Ltmp|LJTI|Lfunc_begin)\d+(_\d+)?")


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, encoding="utf-8", errors="replace"):
        if name is None:
            m = re.match(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$", line)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name] = "\n".join(body)
            name = None
            continue
        s = line.split(";", 1)[0].rstrip()
        if s:
            body.append(_LOCAL.sub(lambda m: "." + m.group(1), s))
    return out


def main(old_dir, new_dir):
    same = changed = new = removed = 0
    for old in sorted(glob.glob(os.path.join(old_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        unit = os.path.basename(old)
        a, b = functions(old), functions(os.path.join(new_dir, unit))
        for f in sorted(set(a) | set(b)):
            if f not in b:
                removed += 1
                print("removed  %s  %s" % (unit, f))
            elif f not in a:
                new += 1
                print("new      %s  %s" % (unit, f))
            elif a[f] != b[f]:
                changed += 1
                print("CHANGED  %s  %s" % (unit, f))
            else:
                same += 1
    print("unchanged %d, changed %d, new %d, removed %d" % (same, changed, new, removed))
    return 1 if changed or removed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
