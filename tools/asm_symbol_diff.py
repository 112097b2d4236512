#!/usr/bin/env python3
"""Compare device assembly symbol by symbol: did moving code between units change what the compiler emits?

   hipcc <the Makefile's FLAGS> --cuda-device-only -S unit.hip -o unit.s      (for every unit, before and after)
   python tools/asm_symbol_diff.py --before old.s [...] --after new1.s new2.s [...]

Every function (kernels and out-of-line device functions) and every kernel descriptor (.amdhsa_kernel block) of the
`before` files is looked up in the `after` files.  Only what the numbering of functions inside a file changes is normalised:
assembler comment lines go, and the local labels .LBB<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n> are renumbered by first
appearance inside the function.  Everything else must be equal line for line.  Prints one line per symbol with its VGPRs, LDS
and scratch bytes on both sides; exit status 1 if any symbol is missing, extra or different.  A symbol that differs is "same-ops"
if its descriptor is equal and it has the same number of each opcode (only order, registers or operands differ); otherwise
the opcodes whose counts changed are listed."""
import argparse
import collections
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp)(\d+)(_\d+)?")


def normalise(lines):
    seen = {}

    def sub(m):
        key = (m.group(1), m.group(2))
        n = seen.setdefault(key, sum(1 for k in seen if k[0] == m.group(1)))
        return ".%s#%d%s" % (m.group(1), n, m.group(3) or "")

    out = []
    for ln in lines:
        s = ln.split(";")[0].strip()   # (comments, whole lines or trailing: they quote block numbers)
        if not s:
            continue
        out.append(LABEL.sub(sub, s))
    return out


def parse(path):
    """-> ({symbol: normalised body lines}, {kernel: descriptor lines})"""
    funcs, descs = {}, {}
    lines = open(path).read().splitlines()
    types = {m.group(1) for ln in lines for m in [re.match(r"\s*\.type\s+([^,\s]+),@function", ln)] if m}
    # (a kernel's descriptor sits between its last instruction and its .Lfunc_end label: taken out of the body, kept apart)
    body, in_desc = None, None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            in_desc = descs.setdefault(m.group(1), [])
        elif in_desc is not None:
            if ln.strip().startswith(".end_amdhsa_kernel"):
                in_desc = None
            else:
                in_desc.append(ln)
        elif re.match(r"\s*\.Lfunc_end\d+:", ln):
            body = None
        elif body is not None:
            body.append(ln)
        else:
            m = re.match(r"([A-Za-z_$.][\w$.]*):", ln)
            if m and m.group(1) in types:
                body = funcs.setdefault(m.group(1), [])
    return {k: normalise(v) for k, v in funcs.items()}, {k: normalise(v) for k, v in descs.items()}


def merged(paths):
    funcs, descs = {}, {}
    for p in paths:
        f, d = parse(p)
        for name in f:
            if name in funcs:
                sys.exit("symbol %s is defined in two files" % name)
        funcs.update(f)
        descs.update(d)
    return funcs, descs


def opcodes(body):
    return collections.Counter(ln.split()[0] for ln in body if not ln.endswith(":") and not ln.startswith("."))


def field(desc, key):
    for ln in desc or []:
        if ln.startswith(key + " "):
            return ln.split()[1]
    return "-"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    a = ap.parse_args()
    f0, d0 = merged(a.before)
    f1, d1 = merged(a.after)
    bad = 0
    keys = (".amdhsa_next_free_vgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")
    print("%-9s %-22s %-22s symbol" % ("", "vgpr/lds/scratch before", "after"))
    for name in sorted(set(f0) | set(f1)):
        if name not in f0 or name not in f1:
            verdict = "MISSING" if name not in f1 else "EXTRA"
        elif f0[name] != f1[name] or d0.get(name) != d1.get(name):
            c0, c1 = opcodes(f0[name]), opcodes(f1[name])
            verdict = "same-ops" if c0 == c1 and d0.get(name) == d1.get(name) else "DIFFERENT"
            print("    %d -> %d instructions%s" % (sum(c0.values()), sum(c1.values()),
                                                  "".join("  %s %+d" % (op, c1[op] - c0[op]) for op in sorted(set(c0) | set(c1)) if c0[op] != c1[op])))
            for k, (x, y) in enumerate(zip(f0[name], f1[name])):
                if x != y:
                    print("    first difference at instruction line %d:\n      - %s\n      + %s" % (k, x, y))
                    break
        else:
            verdict = "equal"
        bad += verdict != "equal"
        res = ["/".join(field(d.get(name), k) for k in keys) if name in d else "(function)" for d in (d0, d1)]
        print("%-9s %-22s %-22s %s" % (verdict, res[0], res[1], name))
    print("%d symbols, %s" % (len(set(f0) | set(f1)), "all equal" if not bad else "%d not equal" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
