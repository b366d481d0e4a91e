#!/usr/bin/env python3
"""BASELINE configs[3]: closed-loop Monte-Carlo -- B cars on fss2019, every receding-horizon step is
one batch of B LTV-MPC QPs (frame transform + reference -> linearise/condense/solve -> PID + plant), all on the device with
no per-step read-back (fsae_mpc_amd.monte_carlo).  Prints one JSON line: QP solves/s over the QPs of the cars still
driving, the exit-flag tally the way main.m:209,222 reports it ("abnormal exits %"), iterations, progress.
--plan: the cars track a plan of the planner stand-in (fsaempc.Plan.profile) instead of the live ramp to 20 m/s.
--raceline: the plan is made on a minimum-curvature racing line (fsaempc.Plan.raceline) instead of the centre line.
--minlap K: the plan is made on a minimum-time racing line (fsaempc.Plan.minlap): K iterations from the minimum-curvature
line; takes --margin, --points, --grip, --cells and --corridor / --cones (the boxes of the control points) as --raceline does.
--report: the lap report (main.m:196-228 over the batch) joins the JSON line as "lap_report".
--corridor FILE.npz: an s-varying track corridor (fsaempc.Corridor) from arrays n_lo, n_hi of (N_w,) over the lap of the
track; the controller's track rows, the report's track violation and, with --raceline, the line's bounds are taken against it.
--line-rows points|cells: with --raceline and --corridor, the form of the line's corridor constraints: the box of every control point (the
default) or one constraint row per cell (Plan.raceline(rows="cells")).
--cones FILE [--car-half-width W]: the corridor comes from the cones that mark the track (Corridor.from_cones), W (default
0.7 m) taken off both edges.  FILE is a race-line CSV in the reference's format (cone columns 8-11) or an .npz with arrays left, right of
(K, 2) -- optionally a string `track`, which must then name --track -- or with TRACK_left, TRACK_right per track as tests/golden/tracks/cones.npz
has them.  Exclusive with --corridor; everything a corridor composes with composes with it.
--lap: every car starts at s = 0 on the centre line, at rest, with the usual lateral and heading scatter (main.m:63), and the step cap
defaults to 1000 (main.m:62): a finished car's STEPS * dt is then a lap time.
--laps K: every car drives K consecutive laps (ClosedLoop(laps=K), DESIGN.md 6m: the lap gate carries it over the line and times the
crossing to a fraction of dt); with --lap the step cap defaults to 1000 K; the per-lap summary (cars that completed the lap, mean, min and
max of its time) joins the JSON line as "lap_summary".
--delay D [--compensate] [--noise s1,...,snx [--noise-seed S]]: the imperfect loop (fsaempc.Latency): a plan reaches the plant
D periods after the state it was solved from; --compensate solves from that state predicted over the D periods; --noise adds
state-estimate noise with these standard deviations (the model's state layout: 5 values kinematic, 7 dynamic).  Echoed as "latency".
--estimator q1,...,qnx [--meas-var r1,...,rnx] [--unmeasured i,j]: the state estimator (fsaempc.Estimator) between the observation
and the solve: process variances per period, measurement variances (default: the squares of --noise) and the indices of components that
are not measured (their variance becomes +inf).  Echoed as "estimator", with the batch's re-initialisations and the mean NIS over the
driving cars' periods.
--sensors s1,...,snx [--sensor-seed S]: Cartesian sensor models (fsaempc.CartesianSensors): the car measures
[X, Y, psi, v, delta] (kinematic) or [X, Y, psi, x_d, y_d, theta_d, delta] (dynamic) with these standard deviations; without --estimator the
loop drives on the projection of the measurement, with it the filter reads the measurement through h(x) (--meas-var is then in the
sensor layout and defaults to the squares of --sensors).  Excludes --noise.  Echoed as "sensors", with the projections that lost the track.
--cone-sensor r_max,fov_deg,s_rho,s_beta[,p_detect] [--cone-k K] [--cone-map FILE.npz] [--unmeasured-pose]: cone-based localisation
(fsaempc.ConeSensor) next to --sensors and --estimator: every period each car observes range and bearing of its K nearest
detected cones within r_max m and fov_deg degrees, and the filter processes them as rows behind its own; the cone draws share
--sensor-seed.  --unmeasured-pose switches the rows of X, Y and psi off (a GPS outage).  Echoed as "cone_sensor", with the mean numbers
of rows applied, cones kept and cones seen per car and period.
--nmpc K [--nmpc-trials T] [--nmpc-timing]: the batched SQP of the nonlinear problem as the controller (fsaempc.Nmpc), K sweeps
per period, warm-started from the previous period's plan shifted by one stage.  "value" then counts the periods of driving cars that
ended with status 0 or 1; "nmpc" joins the JSON line: the status shares over the driving cars' periods, mean sweeps and QP iterations per
period and, with --nmpc-timing, the SQP's phase sums.  Excludes --corridor, --cones and --warm.
usage: tools/closed_loop_bench.py [--model dynamic|kinematic] [--batch 2048] [--steps 200] [--horizon 40] [--track fss2019]
                                  [--plan | --raceline | --minlap K [--margin M] [--points N_c]] [--grip G] [--cells N_s] [--report [--slack-tol T]] [--lap] [--laps K]
                                  [--corridor FILE.npz | --cones FILE [--car-half-width W]] [--line-rows points|cells]
                                  [--delay D [--compensate]] [--noise s1,...,snx [--noise-seed S]]
                                  [--estimator q1,...,qnx [--meas-var r1,...,rnx] [--unmeasured i,j]]
                                  [--sensors s1,...,snx [--sensor-seed S]]
                                  [--cone-sensor r_max,fov_deg,s_rho,s_beta[,p_detect] [--cone-k K] [--cone-map FILE.npz] [--unmeasured-pose]]
                                  [--nmpc K [--nmpc-trials T] [--nmpc-timing]]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import fsae_mpc_amd as fm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="dynamic", choices=["kinematic", "dynamic"])
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=None, help="step cap (default 200; with --lap 1000, main.m:62)")
    ap.add_argument("--track", default="fss2019", choices=["fsg2019", "fss2019", "fso2020"])
    ap.add_argument("--report", action="store_true", help="keep the lap report's records on the device and add its summary to the JSON line")
    ap.add_argument("--lap", action="store_true", help="all cars start at s = 0 at rest; step cap 1000")
    ap.add_argument("--laps", type=int, default=1, help="consecutive laps per car (the lap gate); with --lap the step cap becomes 1000 per lap")
    ap.add_argument("--slack-tol", type=float, default=1e-6, help="with --report: a slack counts as in use above this value")
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--seed", type=int, default=20190)
    ap.add_argument("--max-iter", type=int, default=100, help="interior-point iteration limit (bounds the batch tail)")
    ap.add_argument("--no-launch-hint", action="store_true", help="do not hand the previous iteration counts to the solve as its launch-order estimate (A/B)")
    ap.add_argument("--warm", action="store_true", help="start every solve from the previous plan shifted by one stage (ClosedLoop(warm_start=True))")
    ap.add_argument("--plan", action="store_true", help="track a speed-profile plan (Plan.profile) instead of the live ramp")
    ap.add_argument("--grip", type=float, default=1.0, help="with --plan: share of the lateral / longitudinal limits the plan uses, (0, 1]")
    ap.add_argument("--cells", type=int, default=500, help="with --plan: cells per lap (N_s)")
    ap.add_argument("--raceline", action="store_true", help="track a plan on a minimum-curvature racing line (Plan.raceline); takes --grip and --cells too")
    ap.add_argument("--minlap", type=int, default=None, metavar="K", help="track a plan on a minimum-time racing line (Plan.minlap, K iterations); takes what --raceline takes")
    ap.add_argument("--margin", type=float, default=0.25, help="with --raceline: distance the line keeps from N_MAX, m")
    ap.add_argument("--points", type=int, default=100, help="with --raceline: control points of the line (N_c)")
    ap.add_argument("--corridor", default=None, metavar="FILE.npz", help="track corridor: arrays n_lo, n_hi of (N_w,) over the lap (Corridor.from_table)")
    ap.add_argument("--cones", default=None, metavar="FILE", help="track corridor from cone positions: a race-line CSV or an .npz (Corridor.from_cones)")
    ap.add_argument("--car-half-width", type=float, default=0.7, help="with --cones: taken off both edges of the corridor, m")
    ap.add_argument("--cone-cells", type=int, default=500, help="with --cones: cells of the corridor's tables (N_w)")
    ap.add_argument("--line-rows", default="points", choices=["points", "cells"],
                    help="with --raceline and --corridor or --cones: the line's corridor as boxes on the control points or as one row per cell")
    ap.add_argument("--delay", type=int, default=0, metavar="D", help="whole periods between the state a plan is solved from and the plant following it (Latency)")
    ap.add_argument("--compensate", action="store_true", help="with --delay >= 1: solve from the observed state predicted over the delay")
    ap.add_argument("--noise", default=None, metavar="s1,...,snx", help="standard deviations of the state-estimate noise, one per state component")
    ap.add_argument("--noise-seed", type=int, default=0, metavar="S", help="with --noise: seed of the counter-based generator")
    ap.add_argument("--estimator", default=None, metavar="q1,...,qnx", help="run the EKF state estimator with these process variances per period (Estimator)")
    ap.add_argument("--meas-var", default=None, metavar="r1,...,rnx", help="with --estimator: measurement variances (default: the squares of --noise)")
    ap.add_argument("--unmeasured", default=None, metavar="i,j", help="with --estimator: state components that are not measured (variance +inf)")
    ap.add_argument("--sensors", default=None, metavar="s1,...,snx", help="Cartesian sensor models: standard deviations in the sensor layout (CartesianSensors); excludes --noise")
    ap.add_argument("--sensor-seed", type=int, default=0, metavar="S", help="with --sensors: seed of the counter-based generator")
    ap.add_argument("--cone-sensor", default=None, metavar="r_max,fov_deg,s_rho,s_beta[,p_detect]",
                    help="cone-based localisation (ConeSensor): range m, opening angle deg, noise of range m and bearing rad, detection probability; needs --sensors and --estimator")
    ap.add_argument("--cone-k", type=int, default=16, metavar="K", help="with --cone-sensor: observations per car and period (k_max)")
    ap.add_argument("--cone-map", default=None, metavar="FILE.npz", help="with --cone-sensor: the cones, left / right or <track>_left / <track>_right (default: tests/golden/tracks/cones.npz)")
    ap.add_argument("--unmeasured-pose", action="store_true", help="with --estimator and --sensors: X, Y and psi are not measured (variance +inf): a GPS outage")
    ap.add_argument("--nmpc", type=int, default=None, metavar="K", help="the batched SQP as the controller, K sweeps per period (Nmpc); excludes --corridor, --cones and --warm")
    ap.add_argument("--nmpc-trials", type=int, default=None, metavar="T", help="with --nmpc: step lengths the line search tries at once (default 8)")
    ap.add_argument("--nmpc-timing", action="store_true", help="with --nmpc: the SQP's phase sums by device events (fsaempc_qp_set_timing: one more synchronisation per sweep)")
    a = ap.parse_args()
    ctl = None
    if (a.nmpc_trials is not None or a.nmpc_timing) and a.nmpc is None:
        ap.error("--nmpc-trials and --nmpc-timing need --nmpc")
    if a.nmpc is not None:
        if a.corridor is not None or a.cones is not None or a.warm:
            ap.error("--nmpc excludes --corridor, --cones and --warm")
        try:
            ctl = fm.Nmpc(sweeps=a.nmpc, **({"trials": a.nmpc_trials} if a.nmpc_trials is not None else {}))
        except ValueError as e:
            ap.error(str(e))
    sigma = None
    if a.noise is not None:
        try:
            sigma = [float(v) for v in a.noise.split(",")]
        except ValueError:
            ap.error("--noise takes comma-separated numbers")
    try:
        lat = fm.Latency(delay=a.delay, compensate=a.compensate, sigma=sigma, seed=a.noise_seed)
        lat.check_batch(5 if a.model == "kinematic" else 7, a.batch)
    except ValueError as e:
        ap.error(str(e))
    est = None
    nx_ = 5 if a.model == "kinematic" else 7
    sens = sens_sigma = None
    if a.sensors is not None:
        if a.noise is not None:
            ap.error("--sensors excludes --noise (two noise sources)")
        try:
            sens_sigma = [float(v) for v in a.sensors.split(",")]
        except ValueError:
            ap.error("--sensors takes comma-separated numbers")
        try:
            sens = fm.CartesianSensors(sens_sigma, seed=a.sensor_seed)
            sens.check_batch(nx_, a.batch)
        except ValueError as e:
            ap.error(str(e))
    if a.estimator is None and (a.meas_var is not None or a.unmeasured is not None):
        ap.error("--meas-var and --unmeasured need --estimator")
    if a.estimator is not None:
        try:
            q = [float(v) for v in a.estimator.split(",")]
            r = [float(v) for v in a.meas_var.split(",")] if a.meas_var is not None else ([v * v for v in (sigma if sigma is not None else sens_sigma)] if sigma is not None or sens_sigma is not None else None)
            skip = [int(v) for v in a.unmeasured.split(",")] if a.unmeasured is not None else []
        except ValueError:
            ap.error("--estimator and --meas-var take comma-separated numbers, --unmeasured comma-separated indices")
        if r is None:
            ap.error("--estimator needs --meas-var, --noise or --sensors")
        if len(r) != nx_ or any(not 0 <= i < nx_ for i in skip):
            ap.error("--meas-var takes %d values, --unmeasured indices 0 .. %d" % (nx_, nx_ - 1))
        if a.unmeasured_pose:
            if sens is None:
                ap.error("--unmeasured-pose needs --sensors (the pose is a component of the sensor layout)")
            skip = sorted(set(skip) | {0, 1, 2})
        for i in skip:
            r[i] = float("inf")
        try:
            est = fm.Estimator(q, r)
            est.resolve(lat, nx_, a.batch, a.laps, sens)
        except ValueError as e:
            ap.error(str(e))
    elif a.unmeasured_pose:
        ap.error("--unmeasured-pose needs --estimator")
    cone_sensor = cone_cfg = None
    if a.cone_sensor is not None:
        if sens is None or est is None:
            ap.error("--cone-sensor needs --sensors and --estimator")
        try:
            cv = [float(v) for v in a.cone_sensor.split(",")]
        except ValueError:
            ap.error("--cone-sensor takes comma-separated numbers")
        if len(cv) not in (4, 5):
            ap.error("--cone-sensor takes r_max,fov_deg,s_rho,s_beta[,p_detect]")
        path = a.cone_map if a.cone_map is not None else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "tracks", "cones.npz")
        with np.load(path) as z:
            if "left" in z.files:
                c_left, c_right = z["left"], z["right"]
            elif a.track + "_left" in z.files:
                c_left, c_right = z[a.track + "_left"], z[a.track + "_right"]
            else:
                ap.error("%s holds neither left / right nor %s_left / %s_right" % (path, a.track, a.track))
        try:
            cone_sensor = fm.ConeSensor(c_left, c_right, r_max=cv[0], fov=np.deg2rad(cv[1]), sigma=(cv[2], cv[3]), p_detect=cv[4] if len(cv) == 5 else 1.0,
                                        k_max=a.cone_k, seed=a.sensor_seed)
        except ValueError as e:
            ap.error(str(e))
        cone_cfg = {"r_max": cv[0], "fov_deg": cv[1], "sigma": [cv[2], cv[3]], "p_detect": cone_sensor.p_detect, "k_max": a.cone_k, "map": path,
                    "cones": [int(len(c_left)), int(len(c_right))]}
    if a.corridor is not None and a.cones is not None:
        ap.error("--cones and --corridor exclude each other")
    if a.line_rows == "cells" and not (a.raceline and (a.corridor is not None or a.cones is not None)):
        ap.error("--line-rows cells needs --raceline and --corridor or --cones")
    if a.minlap is not None and (a.raceline or a.minlap < 0):
        ap.error("--minlap K needs K >= 0 and excludes --raceline")
    if a.steps is None:
        a.steps = 1000 * a.laps if a.lap else 200
    model = fm.KINEMATIC if a.model == "kinematic" else fm.DYNAMIC
    tr = fm.Track.load(a.track)
    cor = None
    if a.corridor is not None:
        with np.load(a.corridor) as z:
            cor = fm.Corridor.from_table(z["n_lo"], z["n_hi"], tr.L)
    cone_info = None
    if a.cones is not None:
        if a.cones.endswith(".npz"):
            with np.load(a.cones) as z:
                if "left" in z.files:
                    if "track" in z.files and str(z["track"]) != a.track:
                        ap.error("%s holds the cones of %s, not of %s" % (a.cones, str(z["track"]), a.track))
                    left, right = z["left"], z["right"]
                elif a.track + "_left" in z.files:
                    left, right = z[a.track + "_left"], z[a.track + "_right"]
                else:
                    ap.error("%s holds neither left / right nor %s_left / %s_right" % (a.cones, a.track, a.track))
        else:
            left, right = fm.Track.cones_from_csv(a.cones)
        cor = fm.Corridor.from_cones(tr, left, right, a.cone_cells, margin=a.car_half_width)
        cone_info = {k: float(cor.info[0, i]) for k, i in fm.CONE_INFO_INDEX.items()}
        cone_info.update(file=a.cones, car_half_width=a.car_half_width, cells=a.cone_cells, n_hi_min=float(cor.n_hi.min().item()), n_hi_max=float(cor.n_hi.max().item()),
                         n_lo_min=float(cor.n_lo.min().item()), n_lo_max=float(cor.n_lo.max().item()))
    plan = fm.Plan.profile(model, tr, N_s=a.cells, grip=a.grip) if a.plan else None
    if a.raceline:
        plan = fm.Plan.raceline(model, tr, N_s=a.cells, N_c=a.points, margin=a.margin, grip=a.grip, corridor=cor, rows=a.line_rows)
    if a.minlap is not None:
        plan = fm.Plan.minlap(model, tr, N_s=a.cells, N_c=a.points, iters=a.minlap, margin=a.margin, grip=a.grip, corridor=cor)
    fm.monte_carlo(model, a.horizon, tr, min(a.batch, 64), 2, a.seed, warm_start=a.warm, reference=plan, corridor=cor, latency=lat, estimator=est, controller=ctl, sensors=sens, cones=cone_sensor)          # warm-up (allocations, code load)
    n_max = float(fm.default_params(model)[fm.PARAM_INDEX["N_MAX"]])
    opts = fm.default_opts(max_iter=a.max_iter)
    t0 = time.perf_counter()
    # the loop of fm.monte_carlo with two more counts kept on the device: steps off the track (|n| > N_MAX) and the last arc length of
    # every car while it drives
    cart0, s_init = fm.monte_carlo_carts(tr, a.batch, a.seed, lap=a.lap)
    cl = fm.ClosedLoop(model, a.horizon, 0.05, tr, cart0, options=opts, warm_start=a.warm, launch_hint=not a.no_launch_hint, reference=plan,
                       metrics=a.report, slack_tol=a.slack_tol, corridor=cor, laps=a.laps, latency=lat, estimator=est, controller=ctl, sensors=sens, cones=cone_sensor)
    cl.x_opt[:, :, 0] += torch.from_numpy(s_init).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(cart0[:, 3]).to(cl.device)[:, None]
    fl_d = torch.zeros((a.steps, a.batch), dtype=torch.int32, device=cl.device)
    it_d = torch.zeros((a.steps, a.batch), dtype=torch.int32, device=cl.device)
    ac_d = torch.zeros((a.steps, a.batch), dtype=torch.bool, device=cl.device)
    off = torch.zeros((), dtype=torch.int64, device=cl.device)
    nis_sum = torch.zeros((), dtype=torch.float64, device=cl.device)
    nis_cnt = torch.zeros((), dtype=torch.int64, device=cl.device)
    rows_sum = torch.zeros((), dtype=torch.int64, device=cl.device)      # with --cone-sensor: rows applied, cones kept and seen, over the same periods
    kept_sum = torch.zeros((), dtype=torch.int64, device=cl.device)
    seen_sum = torch.zeros((), dtype=torch.int64, device=cl.device)
    s_first = s_last = None
    if ctl is not None:   # the SQP's verbatim status and sweep count per (period, car), and its phase sums by device events
        st_d = torch.zeros((a.steps, a.batch), dtype=torch.int32, device=cl.device)
        sw_d = torch.zeros((a.steps, a.batch), dtype=torch.int32, device=cl.device)
        phase = dict(build=0.0, solve=0.0, linesearch=0.0, compact=0.0) if a.nmpc_timing else None
        if phase is not None:
            fm.lib().fsaempc_qp_set_timing(1)
    for t in range(a.steps):
        out = cl.step()
        drv = cl.finished == 0
        fl_d[t] = out["exitflag"]; it_d[t] = out["iter"]; ac_d[t] = drv
        if ctl is not None:
            st_d[t] = out["status"]; sw_d[t] = out["sweeps"]
            if phase is not None:
                for k_, v_ in fm.sqp_timing().items():
                    phase[k_] += v_
        if s_first is None:
            s_first = cl.x0[:, 0].clone(); s_last = cl.x0[:, 0].clone()
        off += ((cl.x0[:, 1].abs() > n_max) & drv).sum()
        s_last = torch.where(drv, cl.x0[:, 0], s_last)
        if est is not None:   # (a car that stopped driving in this very period still had its filter run)
            nis_sum += cl.est_nis.sum(); nis_cnt += (cl.est_nis != 0).sum()
            if cone_sensor is not None:
                rows_sum += cl.est_rows.sum(); kept_sum += cl.cone_n.sum(); seen_sum += cl.cone_seen.sum()
    torch.cuda.synchronize(cl.device)
    fl, it, ac = fl_d.cpu().numpy(), it_d.cpu().numpy(), ac_d.cpu().numpy()
    dt_wall = time.perf_counter() - t0
    dist = (s_last - s_first).cpu().numpy()
    if a.laps > 1:   # (s is wrapped by L at every crossing the car drove on from; the final crossing leaves it beyond L)
        dist = dist + tr.L * np.minimum(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]].cpu().numpy(), a.laps - 1)
    n_act = int(ac.sum())
    hist = {int(k_): int(c_) for k_, c_ in zip(*np.unique(fl[ac], return_counts=True))}
    solved = int(((fl == 0) & ac).sum())
    bad_data = int(((fl == -1) & (it == 0) & ac).sum())    # -1 before the first iteration = non-finite QP data (vehicle state outside
                                                           # the model's domain, e.g. v_x -> 0 in the dynamic model): the reference's
                                                           # MEX gateway rejects such a call ("Argument contains NaN")
    x0 = cl.x0.cpu().numpy()
    fin = cl.finished.cpu().numpy()
    lap_summary = None
    if a.laps > 1:
        lt = cl.lap_times.cpu().numpy()
        lap_summary = np.zeros((a.laps, 4))
        fm._lib.check(fm.lib().fsaempc_cl_lap_summary(lt.ctypes.data, a.batch, a.laps, lap_summary.ctypes.data), "fsaempc_cl_lap_summary")
    lost_qps = int((~ac[:, fin == 2]).sum())   # steps the lost cars sat out
    nmpc = None
    if ctl is not None:   # (mean sweeps = QPs solved per period and driving car; the accept entry's iter is the SQP's qp_iter)
        st, sw = st_d.cpu().numpy(), sw_d.cpu().numpy()
        nmpc = {"sweeps": a.nmpc, "trials": a.nmpc_trials if a.nmpc_trials is not None else 8,
                "status_share_driving_cars": {fm.sqp.STATUS.get(int(k_), str(int(k_))): float(c_) / max(1, n_act) for k_, c_ in zip(*np.unique(st[ac], return_counts=True))},
                "mean_sweeps_per_period": float(sw[ac].mean()) if n_act else 0.0, "mean_qp_iterations_per_period": float(it[ac].mean()) if n_act else 0.0,
                **({"sqp_phase_ms_sum": phase, "sqp_phase_ms_per_step": {k_: v_ / a.steps for k_, v_ in phase.items()}} if phase is not None else {})}
    print(json.dumps({
        "metric": "QP solves/sec (closed loop, %s N=%d, fp64)" % (a.model, a.horizon), "value": solved / dt_wall, "unit": "QP solves/s",
        "n_gpus": 1, "steps": a.steps, "ms_per_step": 1e3 * dt_wall / a.steps, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE configs[3] share of one GPU: %d cars on %s, %d receding-horizon steps, every step one batch of QPs "
                               "(frame transform + reference + linearise/condense/solve + PID/plant, device-resident loop, no per-step read-back; "
                               "wall time includes the allocation of the run)" % (a.batch, a.track, a.steps),
                   "track": a.track, "corridor": a.corridor,
                   "latency": {"delay": a.delay, "compensate": bool(a.compensate), "noise": sigma, "noise_seed": a.noise_seed},
                   **({"estimator": {"q": q, "r": [None if v == float("inf") else v for v in r], "unmeasured": skip, "resets": int(cl.est_resets.sum().item()),
                                     "cars_reset": int((cl.est_resets > 0).sum().item()),
                                     "nis_mean": float((nis_sum / nis_cnt.clamp(min=1)).item()), "nis_periods": int(nis_cnt.item()),
                                     "measured_components": nx_ - len(skip)}} if est is not None else {}),
                   **({"sensors": {"sigma": sens_sigma, "seed": a.sensor_seed, "filter": est is not None, "projections_lost": int(cl.proj_lost.sum().item()),
                                   "cars_with_a_lost_projection": int((cl.proj_lost > 0).sum().item())}} if sens is not None else {}),
                   **({"cone_sensor": dict(cone_cfg, rows_mean=float(rows_sum.item()) / max(1, int(nis_cnt.item())),
                                           cones_kept_mean=float(kept_sum.item()) / max(1, int(nis_cnt.item())),
                                           cones_seen_mean=float(seen_sum.item()) / max(1, int(nis_cnt.item())))} if cone_sensor is not None else {}),
                   "controller": "LTV-MPC" if ctl is None else "MS-NMPC (batched SQP)", **({"nmpc": nmpc} if nmpc is not None else {}),
                   **({"cones": cone_info} if cone_info is not None else {}), "start": "s = 0 at rest (--lap)" if a.lap else "random s, speed U[0, 15]",
                   # (a mean over an empty set is NaN in the report: null in the JSON line)
                   **({"lap_report": {k: (None if v != v else v) for k, v in cl.report().summary().items()}, "slack_tol": a.slack_tol} if a.report else {}),
                   **({"laps": a.laps, "lap_summary": [{"lap": i + 1, "cars": int(r[0]), "mean_s": None if r[1] != r[1] else float(r[1]),
                                                         "min_s": None if r[2] != r[2] else float(r[2]), "max_s": None if r[3] != r[3] else float(r[3])}
                                                        for i, r in enumerate(lap_summary)]} if lap_summary is not None else {}),
                   "qps_of_driving_cars": n_act, "qps_total_launched": int(a.batch * a.steps),
                   "exitflag_histogram_driving_cars": hist, "minus1_with_nonfinite_qp_data": bad_data,
                   "minus1_on_finite_qp_data_pct": 100.0 * (hist.get(-1, 0) - bad_data) / max(1, n_act), "abnormal_exit_pct": 100.0 * (1.0 - solved / max(1, n_act)),
                   # the same tally with the QPs a lost car (|n| >= 3 m, |v| >= 100 m/s or |state| >= 1e6: `finished` = 2, plant.hip) would still
                   # have launched counted as abnormal: lost cars leave the denominator above, round 1 had no such rule
                   "abnormal_exit_pct_lost_cars_counted": 100.0 * (1.0 - solved / max(1, n_act + lost_qps)), "qps_not_launched_for_lost_cars": lost_qps,
                   "mean_ipm_iterations": float(it[ac].mean()) if n_act else 0.0,
                   "cars_past_end_of_track_parameter": int((cl.finished == 1).sum().item()), "cars_lost": int((cl.finished == 2).sum().item()),
                   "mean_speed_end": float(cl.cart[:, 3].mean().item()),
                   "reference": ("plan: racing line, N_s = %d, N_c = %d, margin %g, grip %g, corridor rows: %s, QP flag %d, lap %.2f s" % (a.cells, a.points, a.margin, a.grip, a.line_rows, int(plan.line_flag[0]), float(plan.lap_time()[0]))) if a.raceline
                                else ("plan: minimum-time line, N_s = %d, N_c = %d, margin %g, grip %g, %d iterations, QP flag %d, lap %.3f s -> %.3f s, steps %s" % (
                                    a.cells, a.points, a.margin, a.grip, a.minlap, int(plan.line_flag[0]), float(plan.lap_history[0, 0]), float(plan.lap_history[0, -1]),
                                    plan.step_history[0].tolist())) if a.minlap is not None
                                else ("plan: speed profile, N_s = %d, grip %g, lap %.2f s" % (a.cells, a.grip, float(plan.lap_time()[0]))) if a.plan else "live ramp to 20 m/s",
                   "steps_off_track_abs_n_gt_N_MAX": int(off.item()), "mean_distance_covered_m": float(np.nanmean(dist)),
                   "total_distance_covered_m": float(np.nansum(dist)),
                   "median_abs_lateral_offset_end": float(np.nanmedian(np.abs(x0[:, 1]))), "seed": a.seed, "max_iter": a.max_iter, "warm_start": bool(a.warm), "launch_hint": not a.no_launch_hint}}))


if __name__ == "__main__":
    main()
