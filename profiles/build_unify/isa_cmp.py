#!/usr/bin/env python3
"""Compares the device assembly of the LTV build kernels of two trees (KEEP_ISA=1 make ..., fsae-mpc_amd/lib/ltv_build*.s): per
instantiation, the instruction lines in order (labels, directives and comments dropped; mangled kernel names, the unit id and the
function number in local labels normalised) and the "Kernel info" figures.  Where the lines differ: how many, and the instruction counts by mnemonic that moved.
usage: isa_cmp.py PARENT_LIB_DIR THIS_LIB_DIR"""
import collections
import re
import subprocess
import sys

USAGE = ["codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"]


def kernels(path):
    """{(NX, EXACT, BLK, PAR): (instruction lines, {figure: value})} of every build kernel of the file"""
    out, key, ins, info = {}, None, [], {}
    for ln in open(path):
        m = re.match(r"^(_Z\S*ltv_build\w*kernel\S*):", ln)
        if m:
            dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
            a = [x.strip() for x in re.search(r"kernel<([^>]*)>", dn).group(1).split(",")]
            blocked = "blocked" in dn
            if len(a) >= 4:      # <NX, EXACT, BLK, PAR[, LtvBlockMap]>
                key = (a[0], a[1], a[2], a[3])
            elif blocked:        # the parent's <NX, PAR>
                key = (a[0], "false", "true", a[1])
            else:                # the parent's <NX, EXACT, PAR>
                key = (a[0], a[1], "false", a[2])
            key = tuple(k.split("::")[-1] for k in key)
            ins, info = [], {}
            continue
        if key is None:
            continue
        body = ln.split(";")[0].strip()
        for u in USAGE:
            m = re.match(r"^; " + u + r":?\s*=?\s*(\d+)", ln)
            if m:
                info[u] = int(m.group(1))
        if ln.startswith("; Occupancy"):
            out[key] = (ins, info)
            key = None
        elif body and not body.startswith(".") and not body.endswith(":") and not body.startswith("//"):
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", re.sub(r"__hip_cuid_\w+", "CUID", body))))
    return out


def main():
    old, new = {}, {}
    for unit in ("ltv_build.s", "ltv_build_blocked.s"):
        old.update(kernels(sys.argv[1] + "/" + unit))
        new.update(kernels(sys.argv[2] + "/" + unit))
    assert sorted(old) == sorted(new), (sorted(old), sorted(new))
    print("NX EXACT BLK PAR | instructions parent/this | lines | VGPRs parent/this | scratch parent/this | occupancy parent/this | LDS parent/this")
    for k in sorted(old):
        (a, ia), (b, ib) = old[k], new[k]
        same = "identical" if a == b else "DIFFERENT"
        print(" ".join(k), "|", "%d/%d" % (len(a), len(b)), "|", same, "|", "%d/%d" % (ia["NumVgprs"], ib["NumVgprs"]), "|",
              "%d/%d" % (ia["ScratchSize"], ib["ScratchSize"]), "|", "%d/%d" % (ia["Occupancy"], ib["Occupancy"]), "|",
              "%d/%d" % (ia.get("LDSByteSize", -1), ib.get("LDSByteSize", -1)))
        if a != b:
            ca, cb = collections.Counter(x.split()[0] for x in a), collections.Counter(x.split()[0] for x in b)
            moved = {m: (ca[m], cb[m]) for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]}
            print("   counts by mnemonic that differ (parent, this):", moved if moved else "none")
            if len(a) == len(b):
                d = [(x, y) for x, y in zip(a, b) if x != y]
                print("   %d line(s) differ in place; the first: %r -> %r" % (len(d), d[0][0], d[0][1]))


if __name__ == "__main__":
    main()
