#!/usr/bin/env python3
"""Static instruction census of one kernel in a `hipcc -S --cuda-device-only` listing.

  scripts/isa_census.py FILE.s KERNEL_SUBSTRING [--blocks] [--regs-all]

Cuts the kernel's ISA into blocks at labels, branches and s_barrier and prints
per block the VALU / MFMA / DS / VMEM / SALU counts with a histogram of its
VALU mnemonics (--blocks), then the kernel's totals and its register and
scratch figures.  --regs-all prints the VGPR / scratch figures of every kernel
of the file whose name holds the substring.  The counts are static, per wave:
a block inside a loop runs once per trip.
"""
import collections
import re
import sys


def classify(m):
    if m.startswith("v_mfma") or m.startswith("v_smfma"):
        return "MFMA"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("ds_"):
        return "DS"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith("s_"):
        return "SALU"
    return "other"


def kernels(path):
    """name -> (instruction lines, metadata dict)"""
    out, name, body = {}, None, []
    meta = collections.defaultdict(dict)
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(\S+):\s*; @(\S+)", line)
        if m and m.group(1) == m.group(2):
            name, body = m.group(1), []
            continue
        if name and s.startswith(".end_amdhsa_kernel"):
            out[name] = body
            name = None
            continue
        if name:
            m = re.match(r"\.amdhsa_(next_free_vgpr|private_segment_fixed_size|accum_offset)\s+(\d+)", s)
            if m:
                meta[name][m.group(1)] = int(m.group(2))
            body.append(s)
    return out, meta


def blocks(body):
    cur = {"label": "entry", "ins": []}
    res = [cur]
    for s in body:
        if s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith((";", ".")) and not re.match(r"^\.LBB\S+:", s):
            continue
        m = re.match(r"^(\.LBB\S+):", s)
        if m:
            cur = {"label": m.group(1), "ins": []}
            res.append(cur)
            continue
        mn = s.split()[0]
        if not re.match(r"^[a-z_0-9]+$", mn):
            continue
        cur["ins"].append(mn)
        if mn.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm")):
            cur = {"label": "(after %s)" % mn, "ins": []}
            res.append(cur)
    return [b for b in res if b["ins"]]


def main():
    path, sub = sys.argv[1], sys.argv[2]
    ks, meta = kernels(path)
    names = [n for n in ks if sub in n]
    if "--regs-all" in sys.argv:
        for n in names:
            print(meta[n].get("next_free_vgpr"), "VGPRs", meta[n].get("private_segment_fixed_size"), "B scratch", n)
        return
    if len(names) != 1:
        sys.exit("%d kernels match %r" % (len(names), sub))
    name = names[0]
    tot = collections.Counter()
    for i, b in enumerate(blocks(ks[name])):
        c = collections.Counter(classify(m) for m in b["ins"])
        tot.update(c)
        if "--blocks" in sys.argv:
            h = collections.Counter(m for m in b["ins"] if classify(m) == "VALU")
            top = " ".join("%s:%d" % kv for kv in h.most_common(8))
            print("%3d %-22s VALU %4d MFMA %2d DS %3d VMEM %2d SALU %3d | %s" %
                  (i, b["label"], c["VALU"], c["MFMA"], c["DS"], c["VMEM"], c["SALU"], top))
    print("total", dict(tot))
    print("meta", dict(meta[name]))


if __name__ == "__main__":
    main()
