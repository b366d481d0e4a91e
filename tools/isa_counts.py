#!/usr/bin/env python3
"""Reads device assembly kept by the checked compile (KEEP_ISA=1 make ..., fsae-mpc_amd/lib/*.s) and prints, per qp_solve_kernel
instantiation, the "Kernel info" figures of the assembly (code bytes, registers, scratch, occupancy; spill counts come from the
compiler's -Rpass-analysis=kernel-resource-usage remarks instead); with --segments KERNEL (a demangled-name fragment such as "<5, 1>"; the unit compiled with
-DQP_STAMPS=1) the opcode counts of that kernel cut at its s_memtime stamps (the files of profiles/chol_panels/).
usage: tools/isa_counts.py FILE.s [--segments "<5, 1>"] [--min 300]"""
import re
import subprocess
import sys

COLS = [("mov0", r"v_mov_b32(_e32)? v\d+, 0$"), ("movdpp", r"v_mov_b32_dpp"), ("snop", r"s_nop"), ("fma", r"v_(fma|fmac)_f64"),
        ("add", r"v_add_f64"), ("mul", r"v_mul_f64"), ("mfma", r"v_mfma"), ("rsq", r"v_rsq_f64"), ("saveexec", r"s_and_saveexec"),
        ("execz", r"s_cbranch_execz"), ("readlane", r"v_readlane"), ("accvgpr", r"v_accvgpr_"), ("cndmask", r"v_cndmask"),
        ("gload", r"global_load"), ("gstore", r"global_store"), ("vmwait", r"s_waitcnt.*vmcnt")]
USAGE = ["codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy"]


def kernels(path):
    """[(mangled name, lines from the label to the end of the "Kernel info" comment block)] of every qp_solve_kernel in the file"""
    out, name, body = [], None, []
    for ln in open(path):
        m = re.match(r"^(_Z\S*qp_solve_kernel\S*):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(ln.rstrip("\n"))
            if ln.startswith("; Occupancy"):
                out.append((name, body))
                name = None
    return out


def demangle(n):
    try:
        return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
    except OSError:
        return n


def main():
    path = sys.argv[1]
    seg = sys.argv[sys.argv.index("--segments") + 1] if "--segments" in sys.argv else None
    nmin = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 300
    for name, body in kernels(path):
        dn = re.sub(r".*(qp_solve_kernel<[^>]*>).*", r"\1", demangle(name))
        if seg is None:
            vals = []
            for u in USAGE:
                m = [re.search(r"^; " + re.escape(u) + r":?\s*=?\s*(\d+)", b) for b in body if b.startswith("; " + u)]
                vals.append("%s: %s" % (u, m[0].group(1) if m and m[0] else "?"))
            print(dn, " ".join(vals))
            continue
        if seg.replace(" ", "") not in dn.replace(" ", ""):
            continue
        ins = [b.split(";")[0].strip() for b in body]
        ins = [i for i in ins if i and not i.startswith(".") and not i.endswith(":") and not i.startswith("//")]
        cuts = [i for i, x in enumerate(ins) if x.startswith("s_memtime")] + [len(ins)]
        print(dn)
        print("seg  n  " + " ".join(c for c, _ in COLS))
        tot = [0] * (len(COLS) + 1)
        lo = 0
        for s, hi in enumerate(cuts):
            part = ins[lo:hi]
            lo = hi
            row = [len(part)] + [sum(1 for x in part if re.match(r, x)) for _, r in COLS]
            tot = [a + b for a, b in zip(tot, row)]
            if len(part) >= nmin:
                print(s, *row)
        print("total", *tot)


if __name__ == "__main__":
    main()
