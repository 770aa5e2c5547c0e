#!/usr/bin/env python3
"""Are kernels of two device listings the same instruction streams?

    hipcc <build.py's flags> -x hip --cuda-device-only -S csrc/pre.hip -o new.s      (and old.s from the parent)
    python tools/isa_same.py old.s new.s letterbox_s2d_lds_kernel letterbox_tiles_kernel=letterbox_tiles_kernelILi0E

Each argument is a substring of a mangled kernel name (OLD=NEW where the name changed, e.g. a kernel
that became a template). Every kernel of old.s whose name contains OLD is paired with the kernel of
new.s whose name is the same with OLD replaced by NEW. Bodies are compared line by line after labels
and symbol names are replaced by their order of first appearance, so only renames are forgiven.
Exit status 0 when every pair is identical, 1 otherwise."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") or re.match(r"^\.LBB\w+:", s):
                body.append(s)
    return out


def normal(body):
    names = {}

    def sub(m):
        return names.setdefault(m.group(0), f"@{len(names)}")
    return [re.sub(r"\.LBB\w+|_Z\w+|__\w+", sub, s) for s in body]


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for arg in sys.argv[3:]:
        a, _, b = arg.partition("=")
        b = b or a
        hits = [k for k in old if a in k]
        if not hits:
            print(f"{arg}: no kernel of {sys.argv[1]} matches")
            bad += 1
        for k in hits:
            k2 = k.replace(a, b)
            if k2 not in new:
                print(f"{k}: no {k2} in {sys.argv[2]}")
                bad += 1
                continue
            x, y = normal(old[k]), normal(new[k2])
            same = x == y
            print(f"{'same' if same else 'DIFFERENT'}  {len(x):6d} / {len(y):6d} lines  {k} -> {k2}")
            bad += not same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
