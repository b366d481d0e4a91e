"""Cost of the QP vector-Jacobian product (fsaempc_qp_vjp_batch_device) beside the forward solve it differentiates, on one MI355X.

    python tools/sens_bench.py [--batch 4096] [--reps 5] [--out profiles/sens/sens_bench_B4096.json]

For kinematic N = 40 and dynamic N = 60 it builds `batch` LTV-MPC QPs (fsae_mpc_amd.instances), solves them with multipliers, then
times the solve and the VJP (one cotangent column, and two) with HIP events, median of `reps`, and records
the VJP's status histogram.  Writes one JSON file (DESIGN.md 6f quotes it)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def _time(torch, fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sens", "sens_bench_B4096.json"))
    a = ap.parse_args()
    import torch
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name or "", arch=getattr(props, "gcnArchName", ""), batch=a.batch, reps=a.reps, shapes=[])
    for model, N in ((fm.KINEMATIC, 40), (fm.DYNAMIC, 60)):
        B = a.batch
        x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 20190, range(B))
        q = fm.LtvBatch(model, N, 0.05, tr, B).build_qp(dev(x0), dev(xr), dev(xl), dev(ul))
        solve = lambda: fm.qp_solve_batch_device(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"], want_lambda=True, want_aux=True)
        r = solve()
        torch.cuda.synchronize()
        rng = np.random.default_rng(1)
        nV = q["g"].shape[1]
        xb1 = dev(rng.standard_normal((B, nV)))
        xb2 = dev(rng.standard_normal((B, 2, nV)))
        vjp = lambda xb: fm.qp_vjp(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"], r["x"], r["lam"], r["exitflag"],
                                   r["polished"], xb)
        o = vjp(xb1)
        torch.cuda.synchronize()
        t_solve = _time(torch, solve, a.reps)
        t_vjp1 = _time(torch, lambda: vjp(xb1), a.reps)
        t_vjp2 = _time(torch, lambda: vjp(xb2), a.reps)
        st = o["status"].cpu().numpy()
        pol = (r["polished"].cpu().numpy() > 0)
        hist = {int(s): int(c) for s, c in zip(*np.unique(st, return_counts=True))}
        row = dict(model="kinematic" if model == fm.KINEMATIC else "dynamic", N=N, nV=nV, nC=q["lbA"].shape[1],
                   solve_ms=t_solve, vjp_ms_k1=t_vjp1, vjp_ms_k2=t_vjp2, vjp_over_solve_k1=t_vjp1 / t_solve,
                   status_histogram=hist, polished=int(pol.sum()))
        print(json.dumps(row), flush=True)
        res["shapes"].append(row)
        del q, r, o
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
