#!/usr/bin/env python3
"""The LTV build kernels of two builds of the library, bit for bit, on one MI355X: every build and fused step below runs once per
library in a child process of its own (a library is bound once per process, FSAEMPC_LIB selects it) and leaves an .npz; the parent
process then compares the raw 64-bit words of every tensor, so NaNs and signed zeros compare too.  Cases: the blocked batches of
tests/test_blocking_cpu.py::SHAPES at B = 16 with the constants compiled in and with param_draws(spread 0.1); the unblocked and
the exact build at tests/test_params_gpu.py's shapes with integrators 0, 1, 2, likewise; the exact build behind a compacted
sub-batch (per-instance blocks, every third instance skipped) through one SQP sweep.  Exit status 1 if any word differs.
--plan: the plan kernels instead, both models throughout: Plan.profile at N_s 37, 97, 500 with the constants
compiled in and with 5 blocks of param_draws(spread 0.2); Plan.raceline and the line-profile entry on a given line at (128, 32),
(130, 32), (500, 117), with a line that folds (a NaN plan) and, through a solver that may not iterate, flagged plans;
Plan.lap_gradient on tests/minlap_cases.py's GRAD_CASES and WRAP_CASE; Plan.minlap(iters=2) on its STEP_CASES.
usage: build_ab.py [--plan] LIB_A LIB_B [out.txt]      (child: build_ab.py --run OUT.npz [--plan])"""
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


def run_plan(out_path):
    import torch
    import fsae_mpc_amd as fm
    import oracle as orc
    import minlap_cases as mc
    res = {}
    keep = lambda tag, **d: res.update({"%s/%s" % (tag, k): v.cpu().numpy() for k, v in d.items()})
    tr = fm.Track.load("fss2019")
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        blocks = fm.param_draws(model, range(5), SEED, 0.2)
        for N_s in (37, 97, 500):
            for pn, par in (("fixed", None), ("par", blocks)):
                pl = fm.Plan.profile(model, tr, N_s=N_s, params=par)
                keep("profile m%d Ns%d %s" % (model, N_s, pn), table=pl.table, t=pl.t)
        for N_s, N_c in ((128, 32), (130, 32), (500, 117)):
            tag = "m%d %dx%d" % (model, N_s, N_c)
            lines = 0.4 * np.sin(np.arange(N_c) * 0.9)[None] * np.linspace(0.2, 1.0, 5)[:, None]
            lines[3] = 30.0                                   # folds over the centre of every corner: a NaN plan
            for pn, par in (("fixed", None), ("par", blocks)):
                pl = fm.Plan.profile(model, tr, N_s=N_s, params=par, line=lines)
                keep("line %s %s" % (tag, pn), table=pl.table, t=pl.t)
                assert bool(pl.t.isnan().all(1).eq(torch.arange(5, device="cuda") == 3).all()), "plan 3, and no other, is NaN"
                pl = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, params=par)
                keep("raceline %s %s" % (tag, pn), table=pl.table, t=pl.t, line=pl.line, flag=pl.line_flag)
            opts = fm.default_opts(max_iter=1)                # no line QP ends in one iteration: every plan is flagged
            pl = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, params=blocks, options=opts)
            keep("raceline %s flagged" % tag, table=pl.table, t=pl.t, line=pl.line, flag=pl.line_flag)
            assert bool((pl.line_flag != 0).all()) and bool((pl.line == 0).all()) and bool(pl.t.isfinite().all()), "flagged: the centre line"
    for case in mc.GRAD_CASES:                                # (the last one is WRAP_CASE: mc.line gives it the spike)
        name, model, N_s, N_c, v_cap, grip = case
        c = np.array(mc.line(orc, orc.Track.load(fm.tracks._HERE + "/tracks/%s.json" % name), case))
        for pn, par in (("fixed", None), ("par", fm.param_draws(model, [1], SEED, 0.2)[0])):
            T, grad = fm.Plan.lap_gradient(model, fm.Track.load(name), c, N_s=N_s, v_cap=v_cap, grip=grip, params=par)
            keep("lapgrad %s %s" % (case, pn), T=T, grad=grad)
    for name, model, N_s, N_c, v_cap, grip in mc.STEP_CASES:
        for pn, par in (("fixed", None), ("par", fm.param_draws(model, range(3), SEED, 0.2))):
            pl = fm.Plan.minlap(model, fm.Track.load(name), N_s=N_s, N_c=N_c, iters=2, margin=mc.MARGIN, v_cap=v_cap, grip=grip, params=par)
            keep("minlap %s m%d %dx%d %s" % (name, model, N_s, N_c, pn), table=pl.table, t=pl.t, line=pl.line, flag=pl.line_flag,
                 lap_history=pl.lap_history, step_history=pl.step_history)
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def main():
    plan = "--plan" in sys.argv
    if plan:
        sys.argv.remove("--plan")
    if sys.argv[1] == "--run":
        return (run_plan if plan else run)(sys.argv[2])
    libs, lines, bad = [os.path.abspath(p) for p in sys.argv[1:3]], [], 0
    with tempfile.TemporaryDirectory() as d:
        for i, lib in enumerate(libs):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--run", os.path.join(d, "%d.npz" % i)] + ["--plan"] * plan, check=True, timeout=600,
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
