#!/usr/bin/env python3
"""Static ISA table of the pointwise kernels: for every k_pwss / k_pwsq instance of one or two
assembly listings (hipcc -S --cuda-device-only of pwss.hip / pwsq.hip) the v_mad_u64_u32 count,
all VALU instructions, VGPRs, spilled VGPRs and scratch bytes (kernel metadata).
usage: pw_isa.py LABEL=file.s[,file.s...] [LABEL2=...]   (e.g. parent=... new=...)"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def parse(path):
    body, meta, cur = {}, {}, None
    mname = None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = [0, 0]
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur and s.startswith("v_"):
            body[cur][1] += 1
            if s.startswith("v_mad_u64_u32"):
                body[cur][0] += 1
        # a kernel's metadata entry lists its keys in alphabetical order: the scratch size comes
        # before .symbol, the VGPR counts after it
        m = re.match(r"^\s*-?\s*\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", line)
        if m and m.group(1) == "private_segment_fixed_size":
            scratch = int(m.group(2))
        elif m and mname:
            meta[mname][m.group(1)] = int(m.group(2))
        if s.startswith(".symbol:"):
            mname = s.split()[1].replace(".kd", "")
            meta[mname] = {"private_segment_fixed_size": scratch}
    rows = {}
    for k, (mad, valu) in body.items():
        if k in meta and meta[k]:
            rows[k] = dict(mad=mad, valu=valu, **meta[k])
    return rows


def main():
    sets = []
    for arg in sys.argv[1:]:
        label, files = arg.split("=", 1)
        rows = {}
        for f in files.split(","):
            rows.update(parse(f))
        sets.append((label, rows))
    names = sorted({k for _, r in sets for k in r if "k_pws" in k})
    dm = demangle(names)
    print("%-24s %-8s %8s %8s %6s %8s %8s" % ("kernel", "build", "mad_u64", "VALU", "VGPRs", "spilled", "scratch"))
    for n in sorted(names, key=lambda x: dm[x]):
        short = re.sub(r"^void (k_pws\w<[^>]*>).*", r"\1", dm[n]).replace(" ", "")
        for label, rows in sets:
            r = rows.get(n)
            if r:
                print("%-24s %-8s %8d %8d %6d %8d %8d" % (short, label, r["mad"], r["valu"], r.get("vgpr_count", -1),
                                                        r.get("vgpr_spill_count", -1), r.get("private_segment_fixed_size", -1)))


if __name__ == "__main__":
    main()
