#!/usr/bin/env python3
"""Are two builds' device code the same?  Compares `hipcc -S --cuda-device-only` outputs
pair by pair: the set of kernels and device functions (by demangled name), each one's
instruction stream (comments, directives and labels dropped, label numbers normalised)
and each kernel's resource metadata.  Prints one line per symbol and a verdict; exit
status 0 only when nothing differs.

  python tools/diag/isa_diff.py base.s new.s [base2.s new2.s ...]
      [--only SUBSTRING]        only symbols whose demangled name contains it
      [--drop-last-arg NAME]    base side: drop the last template argument of NAME<...>
                                (a template parameter removed in `new`)"""
import argparse
import re
import shutil
import subprocess
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def demangle(names):
    tool = (shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def drop_last_arg(name, tmpl):
    """`tmpl<a, b, c>(...)` -> `tmpl<a, b>(...)` (the arguments hold no nested template)."""
    return re.sub(r'(\b%s<[^<>]*), [^,<>]+>' % re.escape(tmpl), r'\1>', name)


def load(path):
    """{mangled name: (instructions, metadata or None)} of one assembly file."""
    s = open(path).read()
    meta = {}
    for blk in s[s.find("amdhsa.kernels:"):].split("\n  - "):
        m = re.search(r'^    \.name:\s+(\S+)', blk, re.M)
        if m:
            meta[m.group(1)] = {k: re.search(r'^    %s:\s+(\S+)' % re.escape(k), blk, re.M).group(1) for k in META}
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M):
        ins = [re.sub(r'\.L(BB|tmp|func_begin|func_end)\d+(_?)', r'.L\1\2', l.strip()) for l in m.group(2).split('\n')
               if l.strip() and not l.strip().startswith((';', '.')) and not l.rstrip().endswith(':')]
        out[m.group(1)] = (ins, meta.get(m.group(1)))
    return out


def compare(base, new, only, drops):
    a, b = load(base), load(new)
    dm = demangle(sorted(set(a) | set(b)))

    def keyed(d, side_drops):
        out = {}
        for k, v in d.items():
            n = dm[k]
            for t in side_drops:
                n = drop_last_arg(n, t)
            if only in n:
                out[n] = (k, v)
        return out
    ka, kb = keyed(a, drops), keyed(b, ())
    # the symbols renamed by the dropped argument, so that references to them compare equal
    ren = {ka[n][0]: kb[n][0] for n in ka if n in kb and ka[n][0] != kb[n][0]}
    pat = re.compile("|".join(sorted(map(re.escape, ren), key=len, reverse=True))) if ren else None
    diffs = 0
    print(f"== {base} -> {new}")
    for n in sorted(set(ka) | set(kb)):
        if n not in kb or n not in ka:
            print(f"ONLY IN {'BASE' if n in ka else 'NEW '}  {n}")
            diffs += 1
            continue
        (ia, ma), (ib, mb) = ka[n][1], kb[n][1]
        if pat:
            ia = [pat.sub(lambda m: ren[m.group(0)], l) for l in ia]
        what = []
        if ia != ib:
            k = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            what.append(f"stream {len(ia)} -> {len(ib)} instructions, first at {k}: "
                        f"`{' '.join(ia[k:k + 1])}` -> `{' '.join(ib[k:k + 1])}`")
        if ma != mb:
            what.append("metadata " + ", ".join(f"{k} {ma[k]} -> {mb[k]}" for k in META if ma[k] != mb[k])
                        if ma and mb else "kernel on one side only")
        tag = "kernel" if ma else "func  "
        if what:
            diffs += 1
            print(f"DIFF   {tag} {n}: " + "; ".join(what))
        else:
            res = " ".join(f"{k[1:]}={ma[k]}" for k in META) if ma else ""
            print(f"same   {tag} {n}: {len(ia)} instructions {res}".rstrip())
        if ka[n][0] != kb[n][0]:
            print(f"       (mangled {ka[n][0]} -> {kb[n][0]})")
    print(f"   {len(ka)} symbols in base, {len(kb)} in new, {diffs} differences")
    return diffs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+", help="base.s new.s pairs")
    ap.add_argument("--only", default="")
    ap.add_argument("--drop-last-arg", action="append", default=[])
    args = ap.parse_args()
    if len(args.files) % 2:
        ap.error("assembly files come in base / new pairs")
    total = sum(compare(args.files[i], args.files[i + 1], args.only, args.drop_last_arg)
                for i in range(0, len(args.files), 2))
    print(f"VERDICT: {'IDENTICAL' if total == 0 else f'{total} DIFFERENCES'}")
    sys.exit(1 if total else 0)
