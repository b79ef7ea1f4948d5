#!/usr/bin/env python3
"""Compare the kernels of two gfx950 device assembly files (hipcc -S --cuda-device-only -fuse-cuid=none), kernel by kernel.

    asm_kernels.py OLD.s NEW.s [--mnemonics REGEX]

A kernel's body is the text between its label and its end marker, comments stripped and function-local label numbers normalised
(they shift when kernels in front of it appear or disappear).  Kernels on both sides must have identical bodies; those whose
demangled-or-mangled name matches --mnemonics need only the same mnemonic sequence (register numbers and the operand order of
commutative operations may differ).  Prints one line per kernel family (name up to the template arguments) with the number of
instances and a sha256 over their bodies, the kernels on one side only, and every mismatch; exit status 1 on a mismatch."""
import argparse
import hashlib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
        if name is None:
            if m and not line.startswith(".L"):
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") and not t.startswith(".L"):
            continue
        t = re.sub(r"\.L(BB|tmp|func_begin)\d+_", r".L\1_", t)
        body.append(t)
    return out


def mnemonics(body):
    return [t.split()[0] for t in body if not t.endswith(":")]


def family(name):
    m = re.match(r"_Z(?:N12_GLOBAL__N_1|N)?(\d+)", name)
    if not m:
        return name
    return name[m.end(1):m.end(1) + int(m.group(1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--mnemonics", default=None)
    a = ap.parse_args()
    ko, kn = kernels(a.old), kernels(a.new)
    bad = 0
    fam = {}
    for name in sorted(set(ko) & set(kn)):
        loose = a.mnemonics and re.search(a.mnemonics, name)
        same = ko[name] == kn[name]
        if not same and loose:
            same = mnemonics(ko[name]) == mnemonics(kn[name])
        f = fam.setdefault((family(name), "mnemonics" if loose else "body"), [0, hashlib.sha256(), hashlib.sha256()])
        f[0] += 1
        for h, k in ((f[1], ko), (f[2], kn)):
            h.update(("\n".join(mnemonics(k[name]) if loose else k[name]) + "\n").encode())
        if not same:
            bad += 1
            print("DIFFERS (%s): %s  %d -> %d instructions" % ("mnemonics" if loose else "body", name, len(mnemonics(ko[name])), len(mnemonics(kn[name]))))
    for (f, how), (n, ho, hn) in sorted(fam.items()):
        print("%-32s %3d instances  %-9s old %s new %s" % (f, n, how, ho.hexdigest(), hn.hexdigest()))
    for name in sorted(set(ko) - set(kn)):
        print("only in old: " + name)
    for name in sorted(set(kn) - set(ko)):
        print("only in new: " + name)
    print("%d kernels on both sides, %d differ" % (len(set(ko) & set(kn)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
