#!/usr/bin/env python3
"""What a track corridor costs, and the corridor file of the driven-lap comparison.
  --make TRACK OUT.npz   writes n_lo, n_hi of (N_w,) for tools/closed_loop_bench.py --corridor: +-WIDE where |kappa| < KAPPA, +-NARROW
                         elsewhere (defaults 1.5 m, 0.02 1/m, 0.75 m; N_w 500); kappa from the track's Bezier table on the host.
  default                one JSON line: the fused step with a (constant) corridor (_c entry) against the step without one (kinematic N = 40,
                         B = 4096, same process, median of 20 launches after 5 warm-ups, HIP events), and Plan.raceline with and
                         without a corridor (N_s 500, N_c 100) and the line's control-point bounds kernel alone, measured the same way.
  --line-rows            one JSON line: Plan.raceline (N_s 500, N_c 100, fsg2019, the corridor of --make) with rows="cells" against rows="points",
                         for 1 and 256 plans (a corridor each), and the rows call alone (Corridor.line_rows), measured the same way.
  --line-rows-once P     P plans through one Plan.raceline(rows="cells") call after one warm-up, for a kernel trace.
  --from-cones P         one JSON line: the corridors of P noisy cone maps (fsg2019, 77 cones per side, sigma 0.05 m, N_w =
                         --cells, margin 0.7) through the C entry alone -- the maps and the outputs are on the device before the
                         events --, measured the same way; the numpy restatement's time per map next to it (--restate: tests/ is on
                         the path).  With --once: one call after one warm-up, for a kernel trace.
usage: tools/corridor_bench.py [--make TRACK OUT.npz [--wide W] [--narrow W] [--kappa K] [--cells N_w]] [--batch 4096] [--horizon 40]
                               [--line-rows | --line-rows-once P | --from-cones P [--once] [--restate] [--cones FILE.npz]]"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def kappa_host(tr, s):
    """curvature of the centre line at s from the M x 4 Bezier tables (first and second derivative in the segment's own parameter)"""
    r = np.mod(s, tr.dl * tr.M); i = np.minimum(np.floor(r / tr.dl).astype(int), tr.M - 1); u = r / tr.dl - i; w = 1 - u

    def d12(P):
        d1 = 3 * (w * w * (P[i, 1] - P[i, 0]) + 2 * w * u * (P[i, 2] - P[i, 1]) + u * u * (P[i, 3] - P[i, 2])) / tr.dl
        d2 = 6 * (w * (P[i, 2] - 2 * P[i, 1] + P[i, 0]) + u * (P[i, 3] - 2 * P[i, 2] + P[i, 1])) / tr.dl ** 2
        return d1, d2
    (xd, xdd), (yd, ydd) = d12(np.asarray(tr.xP)), d12(np.asarray(tr.yP))
    return (xd * ydd - yd * xdd) / (xd * xd + yd * yd) ** 1.5


def median_ms(torch, fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", nargs=2, metavar=("TRACK", "OUT.npz"), default=None)
    ap.add_argument("--wide", type=float, default=1.5)
    ap.add_argument("--narrow", type=float, default=0.75)
    ap.add_argument("--kappa", type=float, default=0.02)
    ap.add_argument("--cells", type=int, default=500)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--line-rows", action="store_true")
    ap.add_argument("--line-rows-once", type=int, default=0, metavar="P")
    ap.add_argument("--from-cones", type=int, default=0, metavar="P")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--restate", action="store_true")
    ap.add_argument("--cones", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "tracks", "cones.npz"))
    a = ap.parse_args()
    import fsae_mpc_amd as fm
    if a.make is not None:
        tr = fm.Track.load(a.make[0])
        s = np.arange(a.cells) * tr.L / a.cells
        w = np.where(np.abs(kappa_host(tr, s)) < a.kappa, a.wide, a.narrow)
        np.savez(a.make[1], n_lo=-w, n_hi=w)
        print(json.dumps({"track": a.make[0], "cells": a.cells, "wide_share": float((w == a.wide).mean()), "file": a.make[1]}))
        return
    import torch
    tr = fm.Track.load("fsg2019")
    if a.from_cones:
        import ctypes as C
        import time
        P, N_w = a.from_cones, a.cells
        with np.load(a.cones) as z:
            left, right = z["fsg2019_left"], z["fsg2019_right"]
        dl, dr = (torch.from_numpy(v).cuda() for v in fm.cone_draws(left, right, 0.05, P, 20190))
        xP, yP = tr.device("cuda:0")
        sp = fm._lib.Spline(tr.M, tr.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        maps = fm._lib.ConeMaps(C.c_void_p(dl.data_ptr()), C.c_void_p(dr.data_ptr()), left.shape[0], right.shape[0], 1)
        lo, hi = torch.empty((P, N_w), dtype=torch.float64, device="cuda"), torch.empty((P, N_w), dtype=torch.float64, device="cuda")
        info = torch.empty((P, 8), dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            rc = fm.lib().fsaempc_corridor_from_cones_device(C.byref(sp), C.c_double(tr.L), C.byref(maps), P, N_w, C.c_double(0.7), C.c_double(5.0),
                                                             C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), C.c_void_p(info.data_ptr()), st)
            assert rc == 0, fm.lib().fsaempc_last_error()
        out = {"what": "fsaempc_corridor_from_cones_device alone: fsg2019, %d + %d cones per map, sigma 0.05 m, N_w %d, margin 0.7, %d maps in one call"
                       % (left.shape[0], right.shape[0], N_w, P)}
        if a.once:
            call(); torch.cuda.synchronize(); call(); torch.cuda.synchronize()
        else:
            out["call_ms_median_min_max"] = median_ms(torch, call)
        h = info.cpu().numpy()
        out.update(kept_min=[float(h[:, 0].min()), float(h[:, 1].min())], dropped=float(h[:, 2:5].sum()), cells_off_segment=float(h[:, 5].sum()),
                   cells_no_room=float(h[:, 6].sum()), width_min=float(h[:, 7].min()), width_min_mean=float(h[:, 7].mean()))
        if a.restate:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
            import cones_numpy as cq
            hl, hr = dl.cpu().numpy(), dr.cpu().numpy()
            t0 = time.perf_counter()
            n = min(P, 4)
            for p in range(n):
                wlo, whi, _ = cq.corridor_from_cones(tr, tr.L, hl[p], hr[p], N_w, 0.7, 5.0)
            out["numpy_restatement_ms_per_map"] = (time.perf_counter() - t0) / n * 1e3
            out["max_abs_diff_to_restatement_last_map"] = float(max(np.abs(lo[n - 1].cpu().numpy() - wlo).max(), np.abs(hi[n - 1].cpu().numpy() - whi).max()))
        print(json.dumps(out))
        return
    if a.line_rows or a.line_rows_once:
        s = np.arange(a.cells) * tr.L / a.cells
        w = np.where(np.abs(kappa_host(tr, s)) < a.kappa, a.wide, a.narrow)
        cors = {P: fm.Corridor.from_table(np.tile(-w, (P, 1)), np.tile(w, (P, 1)), tr.L) for P in sorted({1, 256, max(1, a.line_rows_once)})}
        line = lambda P, rows: fm.Plan.raceline(fm.DYNAMIC, tr, N_s=500, N_c=100, corridor=cors[P], rows=rows)
        if a.line_rows_once:
            for _ in range(2):
                plan = line(a.line_rows_once, "cells")
                torch.cuda.synchronize()
            print(json.dumps({"plans": a.line_rows_once, "flags_not_0": int((plan.line_flag != 0).sum().item()), "lap_s": float(plan.lap_time()[0])}))
            return
        out = {"what": "median / min / max ms of 20 calls after 5 warm-ups, HIP events, one process; fsg2019, dynamic model, N_s 500, N_c 100, "
                       "+-%g m where |kappa| < %g, +-%g m elsewhere (%d cells), one corridor per plan; whole Plan.raceline call, allocations included"
                       % (a.wide, a.kappa, a.narrow, a.cells)}
        for P in (1, 256):
            out["plans_%d" % P] = {"points_ms": median_ms(torch, lambda: line(P, "points")), "cells_ms": median_ms(torch, lambda: line(P, "cells")),
                                   "points_again_ms": median_ms(torch, lambda: line(P, "points")),
                                   "rows_call_alone_ms": median_ms(torch, lambda: cors[P].line_rows(500, 100, 0.25)),
                                   "bounds_call_alone_ms": median_ms(torch, lambda: cors[P].line_bounds(500, 100, 0.25))}
            pc, pp = line(P, "cells"), line(P, "points")
            out["plans_%d" % P].update(flags_not_0=int((pc.line_flag != 0).sum().item()), lap_cells_s=float(pc.lap_time()[0]), lap_points_s=float(pp.lap_time()[0]))
        print(json.dumps(out))
        return
    model, N, B = fm.KINEMATIC, a.horizon, a.batch
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    x0, xl, ul, xr = (dev(v) for v in fm.instances(model, N, 0.05, tr.L, 20190, range(B)))
    cor = fm.Corridor.constant(tr.L, 0.75, N_w=500)   # +-N_MAX: the QPs keep their bits, so the difference is the corridor's kernels alone
    plain, inside = fm.LtvBatch(model, N, 0.05, tr, B), fm.LtvBatch(model, N, 0.05, tr, B, corridor=cor)
    t_plain = median_ms(torch, lambda: plain.step(x0, xr, xl, ul))
    t_cor = median_ms(torch, lambda: inside.step(x0, xr, xl, ul))
    t_plain2 = median_ms(torch, lambda: plain.step(x0, xr, xl, ul))
    l_plain = median_ms(torch, lambda: fm.Plan.raceline(model, tr, N_s=500, N_c=100))
    l_cor = median_ms(torch, lambda: fm.Plan.raceline(model, tr, N_s=500, N_c=100, corridor=cor))
    # the control-point bounds kernel on its own (fsaempc_corridor_line_bounds_device), one plan and 256 plans
    cor256 = fm.Corridor.from_table(np.tile(cor.n_lo.cpu().numpy(), (256, 1)), np.tile(cor.n_hi.cpu().numpy(), (256, 1)), tr.L)
    b_1 = median_ms(torch, lambda: cor.line_bounds(500, 100, 0.25))
    b_256 = median_ms(torch, lambda: cor256.line_bounds(500, 100, 0.25))
    print(json.dumps({"what": "median / min / max ms of 20 launches after 5 warm-ups, HIP events, one process; the corridor is the constant +-0.75 "
                              "(500 cells): the same QPs bit for bit with and without it",
                      "step": {"model": "kinematic", "N": N, "B": B, "without_corridor_ms": t_plain, "with_corridor_ms": t_cor,
                               "without_corridor_again_ms": t_plain2},
                      "raceline": {"N_s": 500, "N_c": 100, "without_corridor_ms": l_plain, "with_corridor_ms": l_cor,
                                   "note": "whole Plan.raceline call, allocations included"},
                      "line_bounds_kernel": {"N_s": 500, "N_c": 100, "one_plan_ms": b_1, "plans_256_ms": b_256,
                                             "note": "the bounds call alone (two output allocations and one launch between the events)"}}))


if __name__ == "__main__":
    main()
