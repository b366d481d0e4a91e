#!/usr/bin/env python3
"""Measurements of the minimum-time racing line, one JSON line per mode.
--laps: lap times of the centre line, the minimum-curvature line and the minimum-time line (K iterations) on the three tracks, both
models, with the iteration records; --restated FILE.json (lap histories of tests/minlap_numpy.py as {"track_model": {"lap": [..]}})
adds the largest relative difference to them.
--time: whole-call wall time of Plan.raceline and of Plan.minlap (K iterations) on the same inputs for --plans 1 256: median, min and
max of --reps synchronised calls after one warm-up call.
--once P: one Plan.profile, one Plan.raceline and one Plan.minlap call with P plans after a warm-up of each (for a kernel trace: all
three plan kernels in one).
usage: tools/minlap_bench.py (--laps [--restated FILE.json] | --time [--plans 1 256] [--reps 10] | --once P) [--iters 12] [--cells 500] [--points 100]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(f, reps, sync):
    f(); sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", action="store_true")
    ap.add_argument("--restated", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--once", type=int, default=0, metavar="P")
    ap.add_argument("--plans", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--cells", type=int, default=500)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--margin", type=float, default=0.25)
    a = ap.parse_args()
    import torch
    import fsae_mpc_amd as fm
    sync = torch.cuda.synchronize
    kw = dict(N_s=a.cells, N_c=a.points, margin=a.margin)
    if a.laps:
        restated = json.load(open(a.restated)) if a.restated else {}
        rows = []
        for name in ("fss2019", "fsg2019", "fso2020"):
            tr = fm.Track.load(name)
            for model in (fm.KINEMATIC, fm.DYNAMIC):
                centre = float(fm.Plan.profile(model, tr, N_s=a.cells).lap_time()[0])
                plan = fm.Plan.minlap(model, tr, iters=a.iters, **kw)
                lap, step = plan.lap_history.cpu().numpy()[0], plan.step_history.cpu().numpy()[0]
                row = {"track": name, "model": int(model), "centre_s": centre, "min_curvature_s": float(lap[0]), "min_time_s": float(lap[-1]),
                       "table_sum_s": float(plan.lap_time()[0]), "lap_history": lap.tolist(), "step_history": step.tolist(), "qp_flag": int(plan.line_flag[0])}
                ref = restated.get("%s_%d" % (name, model))
                if ref is not None and len(ref["lap"]) == len(lap):
                    row["max_rel_diff_to_restated"] = float(np.max(np.abs(lap - np.array(ref["lap"])) / np.array(ref["lap"])))
                    row["steps_equal_restated"] = bool(step.tolist() == ref.get("step"))
                rows.append(row)
        print(json.dumps({"what": "lap times, N_s %d, N_c %d, margin %g, K %d, default ladder" % (a.cells, a.points, a.margin, a.iters), "rows": rows}))
    if a.time:
        tr = fm.Track.load("fss2019")
        rows = []
        for model in (fm.KINEMATIC, fm.DYNAMIC):
            for P in a.plans:
                blocks = fm.param_draws(model, range(P), 77, 0.1) if P > 1 else None
                race = timed(lambda: fm.Plan.raceline(model, tr, params=blocks, **kw), a.reps, sync)
                ml = timed(lambda: fm.Plan.minlap(model, tr, iters=a.iters, params=blocks, **kw), a.reps, sync)
                ml0 = timed(lambda: fm.Plan.minlap(model, tr, iters=0, params=blocks, **kw), a.reps, sync)
                rows.append({"model": int(model), "n_plans": P, "raceline": race, "minlap_K0": ml0, "minlap": ml})
        print(json.dumps({"what": "whole-call wall time (allocation included), fss2019, N_s %d, N_c %d, K %d, ladder of 8" % (a.cells, a.points, a.iters), "rows": rows}))
    if a.once:
        tr = fm.Track.load("fss2019")
        P = a.once
        blocks = fm.param_draws(fm.DYNAMIC, range(P), 77, 0.1) if P > 1 else None
        for rep in range(2):
            fm.Plan.profile(fm.DYNAMIC, tr, N_s=a.cells, params=blocks); sync()
            fm.Plan.raceline(fm.DYNAMIC, tr, params=blocks, **kw); sync()
            fm.Plan.minlap(fm.DYNAMIC, tr, iters=a.iters, params=blocks, **kw); sync()
        print(json.dumps({"what": "two Plan.profile, two Plan.raceline and two Plan.minlap calls", "n_plans": P, "iters": a.iters}))


if __name__ == "__main__":
    main()
