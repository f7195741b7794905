#!/usr/bin/env python3
"""Static figures of the kernels (every __global__ k_*) in `hipcc -S --cuda-device-only` output, of
pwss.hip / pwsq.hip first of all: per kernel the register and scratch sizes of the code object's
metadata and the counts of the instructions the wrap selects of pw_combine turn into.

    pw_isa_stats.py LABEL=file.s [LABEL=file.s ...]

With two or more labels the last column says whether a kernel's instruction stream is identical
in all of them (labels, comments and directives ignored)."""
import hashlib
import re
import sys

KERN = re.compile(r"^(_Z\d+k_\w+):\s*(;.*)?$")
PATS = [("v_cndmask", r"v_cndmask"), ("v_cmp", r"v_cmpx?_"), ("ds_read", r"ds_read"), ("ds_write", r"ds_write"),
        ("v_alignbit", r"v_alignbit"), ("s_nop", r"s_nop"), ("valu", r"v_"), ("all", r"[a-z]")]


def demangle(sym):
    """k_name<a,b,...> for integer and bool template arguments, k_name without; else the symbol"""
    n = int(re.match(r"_Z(\d+)", sym).group(1))
    at = sym.index("k_")
    name, rest = sym[at:at + n], sym[at + n:]
    if not rest.startswith("I"):
        return name
    m = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
    if not m:
        return sym
    return "%s<%s>" % (name, ",".join(a.replace("n", "-") for a in re.findall(r"L[a-z](n?\d+)E", m.group(1))))


def parse(path):
    out, cur, body = {}, None, []
    meta, mname = {}, None
    for line in open(path):
        m = KERN.match(line)
        if m:
            cur, body = demangle(m.group(1)), []
            continue
        if cur is not None:
            s = line.strip()
            if s.startswith(".Lfunc_end"):
                cnt = {k: sum(1 for i in body if re.match(p, i)) for k, p in PATS}
                cnt["hash"] = hashlib.sha1("\n".join(body).encode()).hexdigest()[:12]
                out[cur] = cnt
                cur = None
            elif s and not s.startswith((";", ".")) and not s.endswith(":"):
                body.append(re.sub(r"\s*;.*$", "", s))
            continue
        m = re.match(r"\s+\.name:\s+(_Z\d+k_\w+)", line)
        if m and not m.group(1).endswith(".kd"):
            mname = demangle(m.group(1))
        for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count"):
            m2 = re.match(r"\s+\.%s:\s+(\d+)" % key, line)
            if m2:
                meta.setdefault("pending", {})[key] = int(m2.group(1))
        if re.match(r"\s+\.wavefront_size:", line) and "pending" in meta:
            pend = meta.pop("pending")
            if mname:
                meta[mname] = pend
            mname = None
    return out, meta


def main():
    sets = [a.split("=", 1) for a in sys.argv[1:]]
    data = {lab: parse(p) for lab, p in sets}
    kernels = sorted({k for c, _ in data.values() for k in c})
    cols = ["vgpr", "scratch", "lds_static"] + [k for k, _ in PATS]
    wk = max([18] + [len(k) for k in kernels])
    print("%-*s %-8s " % (wk, "kernel", "build") + " ".join("%10s" % c for c in cols) + "  same_code")
    for k in kernels:
        hashes = {data[lab][0][k]["hash"] if k in data[lab][0] else None for lab, _ in sets}   # None: not in that build
        for lab, _ in sets:
            c, meta = data[lab]
            if k not in c:
                continue
            m = meta.get(k, {})
            row = [m.get("vgpr_count", -1), m.get("private_segment_fixed_size", -1), m.get("group_segment_fixed_size", -1)]
            row += [c[k][n] for n, _ in PATS]
            print("%-*s %-8s " % (wk, k, lab) + " ".join("%10d" % v for v in row) + ("  yes" if len(hashes) == 1 else "  no"))


if __name__ == "__main__":
    main()
