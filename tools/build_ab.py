#!/usr/bin/env python3
"""The LTV build kernels of two builds of the library, bit for bit, on one MI355X: every build and fused step below runs once per
library in a child process of its own (a library is bound once per process, FSAEMPC_LIB selects it) and leaves an .npz; the parent
process then compares the raw 64-bit words of every tensor, so NaNs and signed zeros compare too.  Cases: the blocked batches of
tests/test_blocking_cpu.py::SHAPES at B = 16 with the constants compiled in and with param_draws(spread 0.1); the unblocked and
the exact build at tests/test_params_gpu.py's shapes with integrators 0, 1, 2, likewise; the exact build behind a compacted
sub-batch (per-instance blocks, every third instance skipped) through one SQP sweep.  Exit status 1 if any word differs.
usage: build_ab.py LIB_A LIB_B [out.txt]      (child: build_ab.py --run OUT.npz)"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT, SEED, B = 0.05, 31, 16
BUILD = ("H", "g", "A", "lb", "ub", "lbA", "ubA", "Bt", "pred", "const")
STEP = ("x_opt", "u_opt", "slack", "fval", "exitflag", "iter")


def run(out_path):
    import torch
    import fsae_mpc_amd as fm
    from test_blocking_cpu import SHAPES as BLOCKED
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    res = {}
    keep = lambda tag, d, keys: res.update({"%s/%s" % (tag, k): d[k].cpu().numpy() for k in keys})
    for model, N, lens, track, _ in BLOCKED:
        tr = fm.Track.load(track)
        x0, xl, ul, xr = (up(v) for v in fm.instances(model, N, DT, tr.L, SEED, range(B)))
        for pn, P in (("fixed", None), ("par", fm.param_draws(model, range(B), SEED, 0.1))):
            mpc = fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens)
            tag = "blocked m%d N%d M%d %s" % (model, N, len(lens), pn)
            keep(tag, mpc.build_qp(x0, xr, xl, ul), BUILD)
            keep(tag, mpc.step(x0, xr, xl, ul), STEP)
    tr = fm.Track.load("fsg2019")
    for model, N in ((0, 20), (0, 40), (1, 40), (1, 60)):
        x0, xl, ul, xr = (up(v) for v in fm.instances(model, N, DT, tr.L, SEED, range(B)))
        P = fm.param_draws(model, range(B), SEED, 0.1)
        for integ in (0, 1, 2):
            for pn, par in (("fixed", None), ("par", P)):
                tag = "m%d N%d integ%d %s" % (model, N, integ, pn)
                mpc = fm.LtvBatch(model, N, DT, tr, B, integrator=integ, params=par)
                keep("plain " + tag, mpc.build_qp(x0, xr, xl, ul), BUILD)
                keep("plain " + tag, mpc.step(x0, xr, xl, ul), STEP)
                keep("exact " + tag, fm.SqpBatch(model, N, DT, tr, B, integrator=integ, params=par).build_qp(x0, xr, ul), BUILD)
        skip = torch.tensor([1 if i % 3 == 0 else 0 for i in range(B)], dtype=torch.int32, device="cuda")
        out = fm.SqpBatch(model, N, DT, tr, B, params=P).solve(x0, xr, ul, skip=skip, max_sweeps=1)
        keep("exact idx m%d N%d" % (model, N), out, ("u_opt", "x_opt", "slack", "fval", "status", "sweeps", "qp_iter", "lambda"))
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def main():
    if sys.argv[1] == "--run":
        return run(sys.argv[2])
    libs, lines, bad = [os.path.abspath(p) for p in sys.argv[1:3]], [], 0
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate(libs):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--run", os.path.join(d, "%d.npz" % i)], check=True, timeout=600,
                           env=dict(os.environ, FSAEMPC_LIB=lib))
        a, b = (np.load(os.path.join(d, "%d.npz" % i)) for i in (0, 1))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            wa, wb = (np.ascontiguousarray(v[k]).view(np.uint64 if v[k].dtype.itemsize == 8 else np.uint32) for v in (a, b))
            n = int((wa != wb).sum()) if wa.shape == wb.shape else -1
            bad += n != 0
            lines.append("%-52s %9d words  %d differ" % (k, wa.size, n))
    lines.append("A = %s\nB = %s\n%d tensors, %d with differing words" % (sys.argv[1], sys.argv[2], len(lines), bad))
    text = "\n".join(lines)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print("\n".join(lines[-3:]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
