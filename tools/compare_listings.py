#!/usr/bin/env python3
"""Compares two `hipcc --offload-device-only -S` listings of tcgnn_device.hip kernel by kernel, whatever their order:
the set of kernel symbols, every kernel's instruction text (comments dropped, block labels renumbered: they carry the
kernel's position in the file) and its .amdhsa_ figures (registers, LDS, scratch).  Exit status 1 on any difference.
usage: compare_listings.py PARENT.s CHANGE.s"""
import re
import sys


def kernels(path):
    """symbol -> (instruction lines, .amdhsa_ lines)"""
    out, name, body, figures = {}, None, [], []
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body, figures = m.group(1), [], []
        elif name and line.strip().startswith(".amdhsa_kernel"):
            figures = [line.strip()]
        elif name and figures:
            figures.append(line.strip())
            if line.strip() == ".end_amdhsa_kernel":
                out[name] = (body, figures)
                name = None
        elif name and line.strip() and not line.lstrip().startswith((".section", ".p2align")):
            body.append(re.sub(r"\.L(BB|JTI|func_end|tmp)\d+", r".L\1", line.strip()))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("kernels: parent %d, change %d" % (len(a), len(b)))
    missing, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    code = [k for k in sorted(set(a) & set(b)) if a[k][0] != b[k][0]]
    figs = [k for k in sorted(set(a) & set(b)) if a[k][1] != b[k][1]]
    print("kernels only in the parent: %d, only in the change: %d" % (len(missing), len(new)))
    print("kernels with other instructions: %d, with other .amdhsa_ figures: %d" % (len(code), len(figs)))
    print("instructions compared: %d" % sum(len(v[0]) for v in a.values()))
    for title, names in (("only in the parent", missing), ("only in the change", new), ("other instructions", code), ("other figures", figs)):
        for k in names:
            print("  %s: %s" % (title, k))
    return 1 if missing or new or code or figs else 0


if __name__ == "__main__":
    sys.exit(main())
