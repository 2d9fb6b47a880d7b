#!/usr/bin/env python3
"""Compare two device assembly listings (hipcc --cuda-device-only -S) of one source file.

    tools/asm_symbol_diff.py OLD.s NEW.s

Lines that carry the per-compile ``__hip_cuid_<hash>`` symbol are dropped.  If the rest is equal
line for line, that is the result.  Otherwise (the functions came out in another order) the
listings are compared per symbol: a function's text from its ``.type NAME,@function`` to its
``.size``, and a kernel's ``.amdhsa_kernel NAME`` ... ``.end_amdhsa_kernel`` resource block.  The
compiler numbers its local labels (.LBB<f>_<b>, .Lfunc_end<f>) by the function's position, so
that number is masked (and the padding before such a line's comment, which follows the number's
width: the positions change from one to two digits when a kernel is removed).  The lines outside those blocks (data symbols, section directives, the
metadata) are compared as a sorted multiset.  The two sets of names must be equal and every
symbol's text, and the lines outside, equal.  Exit status 0: nothing differs.
"""
import re
import sys

LOCAL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b")  # (BB<f>_<b>: the loop comments)


def read(path):
    return [l.rstrip("\n") for l in open(path) if "__hip_cuid_" not in l]


REST = "<lines outside the symbols>"


def symbols(lines):
    out, name = {REST: []}, None
    for l in lines:
        s = l.strip()
        f = re.match(r"\.type\s+(\S+),@function", s)
        k = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if f or k:
            name = ("text:" if f else "amdhsa:") + (f or k).group(1)
            out[name] = []
        m = LOCAL.sub(r"\1N\2", l)
        if m != l:  # (a label's comment is padded to a column: the number's width moves it)
            m = re.sub(r"\s+;", " ;", m)
        out[name or REST].append(m)
        if s == ".end_amdhsa_kernel" or (name and name.startswith("text:") and
                                         s.startswith(".size")):
            name = None
    out[REST].sort()  # (data symbols, sections, metadata: their order follows the functions')
    return out


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    so, sn = symbols(old), symbols(new)
    print("kernels: %d (old) %d (new)" % tuple(
        sum(n.startswith("amdhsa:") for n in s) for s in (so, sn)))
    if old == new:
        print("equal line for line: 0 symbols differ")
        return 0
    bad = sorted(set(so) ^ set(sn))
    for n in bad:
        print("only in", "old:" if n in so else "new:", n)
    differ = [n for n in sorted(set(so) & set(sn)) if so[n] != sn[n]]
    for n in differ:
        print("differs:", n)
    print("not equal line for line; compared per symbol: %d symbols differ" %
          (len(differ) + len(bad)))
    return 1 if differ or bad else 0


if __name__ == "__main__":
    sys.exit(main())
