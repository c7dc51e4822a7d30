#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of one unit, kernel by kernel.

  hipcc $(FLAGS) -x hip --cuda-device-only -S unit.hip -o old.s -Rpass-analysis=kernel-resource-usage 2> old.res
  (the same in the other tree: new.s, new.res)
  scripts/isa_compare.py old.s new.s [--rename PATTERN=REPLACEMENT ...]

A kernel's instruction stream is its lines with comments, directives and blank lines dropped and its branch
labels numbered in order of first appearance.  Kernels are paired by demangled name without namespaces and
parameter list; --rename (a regular expression and its replacement, applied to the old names) follows a kernel
that changed its name or its template arguments.  Prints one line per pair: old name, new name, instruction
counts, VGPRs, scratch bytes per lane, LDS bytes per workgroup and occupancy of both (from the .res file next to
each .s, when there is one), and "identical" or the opcodes whose counts differ.  Exit status 1: a kernel has no
partner, gained scratch or lost occupancy."""
import argparse
import collections
import os
import re
import subprocess
import sys

CXXFILT = "c++filt"


def demangle(names):
    out = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def short(name):
    name = re.sub(r"^void ", "", name)
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):  # the parameter list: the first '(' outside template brackets, namespaces aside
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not name.startswith("(anonymous namespace)", i):
            cut = i
            break
    return re.sub(r"(\w+|\(anonymous namespace\))::", "", name[:cut])


def kernels(path):
    """{mangled name: [instruction, ...]} of the .amdhsa kernels in an assembly file"""
    lines = open(path).read().splitlines()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    out, cur, labels = {}, None, {}
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        m = re.match(r"^(\S+):$", ln)
        if m and m.group(1) in names:
            cur, labels = m.group(1), {}
            out[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:$", ln):
            cur = None
            continue
        s = ln.strip()
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        s = re.sub(r"\.LBB\d+_\d+", lambda g: labels.setdefault(g.group(0), "L%d" % len(labels)), s)
        if not s.endswith(":"):
            out[cur].append(re.sub(r"\s+", " ", s))
    return out


def resources(path):
    res, cur = {}, None
    if not os.path.exists(path):
        return res
    for ln in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]):\s+(\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[])
    a = ap.parse_args()
    ko, kn = kernels(a.old), kernels(a.new)
    ro, rn = resources(a.old[:-2] + ".res"), resources(a.new[:-2] + ".res")
    do, dn = demangle(list(ko)), demangle(list(kn))
    new_by_name = {short(dn[k]): k for k in kn}
    bad = 0
    for k in ko:
        old_name = want = short(do[k])
        for r in a.rename:
            pat, rep = r.split("=", 1)
            want = re.sub(pat, rep, want)
        if want not in new_by_name:
            print("%s -> %s: NO PARTNER" % (old_name, want))
            bad = 1
            continue
        j = new_by_name.pop(want)
        so, sn = ko[k], kn[j]
        if so == sn:
            verdict = "identical"
        else:
            co = collections.Counter(i.split()[0] for i in so)
            cn = collections.Counter(i.split()[0] for i in sn)
            diff = ["%s %d->%d" % (op, co[op], cn[op]) for op in sorted(set(co) | set(cn)) if co[op] != cn[op]]
            verdict = "DIFFERENT: " + (", ".join(diff) if diff else "same opcode counts, other order or operands")
        x, y = ro.get(k, {}), rn.get(j, {})
        f = lambda key: "%s->%s" % (x.get(key, "?"), y.get(key, "?"))
        if x and y and (y["ScratchSize"] > x["ScratchSize"] or y["Occupancy"] < x["Occupancy"]):
            verdict += " [MORE SCRATCH OR LESS OCCUPANCY]"
            bad = 1
        print("%s -> %s: instructions %d->%d, VGPRs %s, scratch %s, LDS %s, occupancy %s: %s" %
              (old_name, want, len(so), len(sn), f("VGPRs"), f("ScratchSize"), f("LDS"), f("Occupancy"), verdict))
    for name in new_by_name:
        print("(new only) %s" % name)
        bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())
