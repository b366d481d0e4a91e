"""Measures the batched SQP of the nonlinear MPC step on one GPU: BASELINE configs[4] (dynamic N = 80) and kinematic N = 40, B
instances each (synthetic, seed 31, u_init = u_lin).  Per shape: NLPs/s, QP solves, sweep histogram, status counts, ms per phase
(device events: compaction + gather, build, solve, line search), warm start on vs off, and the fixed-sweep loop LtvBatch.sqp(sweeps=8,
step=0.5) at the same B for comparison.  One JSON line per shape (and --out: all of them in one file).  Kernel names: run under
`rocprofv3 --kernel-trace --stats` separately."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--shapes", default="dyn80,kin40")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    import fsae_mpc_amd as fm
    assert torch.cuda.is_available(), "sqp_bench needs the GPU"
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tr = fm.Track.load("fsg2019")
    res = []
    for shape in a.shapes.split(","):
        model = fm.DYNAMIC if shape.startswith("dyn") else fm.KINEMATIC
        N, B = int(shape[3:]), a.batch
        x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 31, range(B))
        X0, XR, XL, UL = dev(x0), dev(xr), dev(xl), dev(ul)
        sb = fm.SqpBatch(model, N, 0.05, tr, B)
        sb.solve(X0, XR, UL, max_sweeps=1)   # warm-up: code objects, workspace
        torch.cuda.synchronize()
        line = dict(shape=shape, model=int(model), N=N, batch=B)
        for ws in (1, 0):
            fm.lib().fsaempc_qp_set_timing(1)
            sb.solve(X0, XR, UL, warm_start=ws)
            torch.cuda.synchronize()
            ph = fm.sqp_timing()
            fm.lib().fsaempc_qp_set_timing(0)
            t0 = time.perf_counter()
            out = sb.solve(X0, XR, UL, warm_start=ws)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st, sw = out["status"].cpu().numpy(), out["sweeps"].cpu().numpy()
            key = "warm" if ws else "cold"
            line[key] = dict(seconds=dt, nlps_per_s=B / dt, qp_solves=int(sw.sum()), qp_iters=int(out["qp_iter"].cpu().numpy().sum()),
                             sweeps_hist={int(k): int(v) for k, v in zip(*np.unique(sw, return_counts=True))},
                             status={int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                             phase_ms=ph, linesearch_share=ph["linesearch"] / max(1e-9, sum(ph.values())))
        if not a.no_baseline:
            lb = fm.LtvBatch(model, N, 0.05, tr, B)
            lb.sqp(X0, XR, XL, UL, sweeps=1, step=0.5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = lb.sqp(X0, XR, XL, UL, sweeps=8, step=0.5)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            du = o["du"][-1].cpu().numpy()
            line["fixed_sweeps_baseline"] = dict(sweeps=8, step=0.5, seconds=dt, nlps_per_s=B / dt, qp_solves=8 * B,
                                                 exitflag0=int((o["exitflag"].cpu().numpy() == 0).sum()),
                                                 last_sweep_du_below_1e_6=int(np.sum(du <= 1e-6)))
        line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)
        res.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
