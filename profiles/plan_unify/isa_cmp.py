#!/usr/bin/env python3
"""Compares the device assembly of the twelve plan kernels of two trees (KEEP_ISA=1 make ..., fsae-mpc_amd/lib/planner.s, raceline.s,
minlap.s), as profiles/build_unify/isa_cmp.py does for the LTV build kernels: per instantiation the instruction lines in order
(labels, directives and comments dropped; mangled names, the unit id and the function number in local labels normalised), the
"Kernel info" figures, the counts by mnemonic that moved, and the lane-0 loops: the basic blocks (label to label) that hold a square
root, an LDS write and a back edge on a scalar counter, which are the two recurrences (and, in the parent's line kernels with a
parameter block, one block of the corner-speed loop, which comes first and has no partner).  They are compared from the last one
back, with register numbers masked; a block that is not the parent's in the same order is printed as a diff.
usage: isa_cmp.py PARENT_LIB_DIR THIS_LIB_DIR"""
import collections
import difflib
import re
import subprocess
import sys

USAGE = ["codeLenInByte", "TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize"]
NAMES = r"plan_profile_kernel|plan_line_profile_kernel|plan_line_lapgrad_kernel"


def kernels(path):
    """{(kernel, DYN, PAR): (blocks of instruction lines, {figure: value})}; kernel: centre, line (the parent's
    plan_line_profile_kernel or plan_profile_kernel<.., LINE = true>) or lapgrad"""
    out, key, blocks, info = {}, None, [[]], {}
    for ln in open(path):
        m = re.match(r"^(_Z\S*(?:%s)\S*):" % NAMES, ln)
        if m:
            dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
            name, args = re.search(r"(%s)<([^>]*)>" % NAMES, dn).groups()
            a = [x.strip().split("::")[-1] for x in args.split(",")]
            kind = "lapgrad" if "lapgrad" in name else ("line" if "line" in name or a[2:] == ["true"] else "centre")
            key, blocks, info = (kind, a[0], a[1]), [[]], {}
            continue
        if key is None:
            continue
        body = ln.split(";")[0].strip()
        for u in USAGE:
            m = re.match(r"^; " + u + r":?\s*=?\s*(\d+)", ln)
            if m:
                info[u] = int(m.group(1))
        if ln.startswith("; Occupancy"):
            out[key] = (blocks, info)
            key = None
        elif re.match(r"^\.LBB\d+_\d+:", body):
            blocks.append([])
        elif body and not body.startswith(".") and not body.endswith(":") and not body.startswith("//"):
            blocks[-1].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", re.sub(r"__hip_cuid_\w+", "CUID", body))))
    return out


def serial(blocks):
    has = lambda b, p: any(x.startswith(p) for x in b)
    return [b for b in blocks if has(b, "v_rsq_f64") and has(b, "ds_write_b64") and has(b, "s_cbranch_scc")]


def masked(b):
    return [re.sub(r"\b([vs])\[?\d+(:\d+)?\]?", r"\1", re.sub(r"\.LBB_\d+", "L", x)) for x in b]


def main():
    old, new = {}, {}
    for unit in ("planner.s", "raceline.s", "minlap.s"):
        old.update(kernels(sys.argv[1] + "/" + unit))
        new.update(kernels(sys.argv[2] + "/" + unit))
    assert sorted(old) == sorted(new) and len(old) == 12, (sorted(old), sorted(new))
    print("kernel DYN PAR | instructions parent/this | lines | VGPRs | SGPRs | scratch | static LDS | occupancy   (each parent/this)")
    for k in sorted(old):
        (ba, ia), (bb, ib) = old[k], new[k]
        a, b = sum(ba, []), sum(bb, [])
        fig = lambda u: "%d/%d" % (ia.get(u, -1), ib.get(u, -1))
        print(" ".join(k), "|", "%d/%d" % (len(a), len(b)), "|", "identical" if a == b else "DIFFERENT", "|", fig("NumVgprs"), "|", fig("TotalNumSgprs"), "|",
              fig("ScratchSize"), "|", fig("LDSByteSize"), "|", fig("Occupancy"))
        if a == b:
            continue
        ca, cb = collections.Counter(x.split()[0] for x in a), collections.Counter(x.split()[0] for x in b)
        moved = {m: (ca[m], cb[m]) for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]}
        print("   counts by mnemonic that differ (parent, this):", moved if moved else "none")
        sa, sb = serial(ba), serial(bb)
        print("   lane-0 loop blocks, instructions: parent %s, this %s" % ([len(x) for x in sa], [len(x) for x in sb]))
        for n, (x, y) in enumerate(zip(reversed(sa), reversed(sb))):
            mx, my = masked(x), masked(y)
            verdict = "the parent's instructions in the parent's order" if mx == my else (
                "the parent's instructions in another order" if collections.Counter(mx) == collections.Counter(my) else "not the parent's instructions")
            print("   block %d from the end (%d/%d): %s, register numbers masked" % (n + 1, len(x), len(y), verdict))
            if mx != my:
                print("\n".join("      " + d for d in difflib.unified_diff(mx, my, "parent", "this", n=1, lineterm="")))


if __name__ == "__main__":
    main()
