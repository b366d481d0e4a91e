"""numpy restatement of the lap report, written from the reference's main.m:196-228 and the semantics of the record slots:
a recorded per-step history in, the 16 slots per car and the batch summary out.  Test infrastructure: it shares no code with the product.

History (dict, T steps, B cars): x0 (T, B, nx) with s = [..., 0], n = [..., 1]; finished (T, B) as the pre-step left it (0 driving,
1 s >= L, 2 lost); flag, iter (T, B); fval (T, B); slack (T, B, ns); a (T, B) first acceleration of the plan the car drives on;
cart (T, B, 7) the state after the plant."""
import numpy as np

SLOTS = ["STEPS", "STATUS", "N_VIOL_INT", "N_VIOL_MAX", "N_ABS_MAX", "ABNORMAL", "OBJ_SUM", "OBJ_CNT", "SLACK_N_CNT", "SLACK_TYRE_CNT",
         "ELL_VIOL_INT", "ELL_VIOL_MAX", "ITER_SUM", "ITER_MAX", "S_START", "S_LAST"]
IDX = {name: i for i, name in enumerate(SLOTS)}
COUNT_SLOTS = ["STEPS", "STATUS", "ABNORMAL", "OBJ_CNT", "SLACK_N_CNT", "SLACK_TYRE_CNT", "ITER_SUM", "ITER_MAX"]
SUMMARY = ["CARS_DRIVING", "CARS_FINISHED", "CARS_LOST", "LAP_MEAN", "LAP_MIN", "LAP_MAX", "STEPS", "ABNORMAL_PCT", "SLACK_N_PCT",
           "SLACK_TYRE_PCT", "OBJ_MEAN", "N_VIOL_INT_MEAN", "N_VIOL_INT_MAX", "N_VIOL_MAX", "ELL_VIOL_INT_MEAN", "ELL_VIOL_INT_MAX",
           "ELL_VIOL_MAX", "ITER_MEAN", "ITER_MAX", "N_ABS_MAX"]
# the constants the reference writes out where it uses them (f_curv_dyn.m:13-18, 47-50; main.m:199, 204)
REF = dict(M=280.0, LF=0.8672, LR=0.6183, GRAV=9.81, PB=12.56, PC=1.38, PD=1.60, PE=-0.58, N_MAX=0.75, ELL_LONG=10.0, ELL_LAT=9.163)
BLOCK_POS = dict(M=0, LF=2, LR=3, GRAV=4, PB=5, PC=6, PD=7, PE=8, N_MAX=22, ELL_LONG=26, ELL_LAT=27)   # positions in a 32-entry block


def constants(block):
    """None -> the reference's literals; a 32-entry parameter block -> the car's own"""
    if block is None:
        return dict(REF)
    return {k: float(block[i]) for k, i in BLOCK_POS.items()}


def fcr(c, cart):
    """rear lateral force, f_curv_dyn.m:32-53, at a Cartesian state (main.m:180 passes x as it is: x_d, y_d, theta_d sit at 4..6)"""
    x_d, y_d, theta_d = cart[3], cart[4], cart[5]
    x_d_hat = x_d + 5 * np.exp(-x_d / 5)
    alpha_r = -np.arctan((y_d - c["LR"] * theta_d) / x_d_hat)
    Fzr = c["M"] * c["GRAV"] * c["LF"] / (c["LR"] + c["LF"])
    B, C_, D, E = c["PB"], c["PC"], c["PD"], c["PE"]
    return Fzr * D * np.sin(C_ * np.arctan(B * alpha_r - E * (B * alpha_r - np.arctan(B * alpha_r))))


def ellipse(c, cart, a):
    return (fcr(c, cart) / (c["M"] * c["ELL_LAT"])) ** 2 + (a / c["ELL_LONG"]) ** 2   # main.m:199


def car_record(h, b, dt, slack_tol, block=None):
    """The 16 slots of car b, the way main.m keeps its lists: collect per step, reduce at the end."""
    c = constants(block)
    T = h["finished"].shape[0]
    tyre = 3 if h["slack"].shape[2] == 4 else 0        # main.m:133 reads slack_opt(4); the kinematic model has one slack for both
    n_list, s_list, flags, iters, obj, sl_n, sl_t, ell = [], [], [], [], [], [], [], []
    status = 0
    for t in range(T):
        fin = int(h["finished"][t, b])
        if fin == 2:                                   # lost: x0 is a placeholder, nothing of this step counts
            status = 2
            break
        n_list.append(float(h["x0"][t, b, 1]))         # main.m:101, before the break
        if fin == 1:
            status = 1
            break
        s_list.append(float(h["x0"][t, b, 0]))
        flags.append(int(h["flag"][t, b])); iters.append(int(h["iter"][t, b])); obj.append(float(h["fval"][t, b]))
        sl_n.append(float(h["slack"][t, b, 0])); sl_t.append(float(h["slack"][t, b, tyre]))
        ell.append(float(ellipse(c, h["cart"][t, b], float(h["a"][t, b]))))
    n_abs = np.abs(np.array(n_list)); flags = np.array(flags, dtype=int); ell = np.array(ell)
    use_n = np.array([v > slack_tol for v in sl_n], dtype=bool); use_t = np.array([v > slack_tol for v in sl_t], dtype=bool)
    out_n = n_abs[n_abs > c["N_MAX"]] - c["N_MAX"]
    out_e = ell[ell > 1.0] - 1.0
    clean = (flags == 0) & ~use_n & ~use_t             # main.m:198 (and the exit flag: an abnormal exit may carry a non-finite fval)
    r = np.zeros(16)
    r[IDX["STEPS"]] = len(s_list); r[IDX["STATUS"]] = status
    r[IDX["N_VIOL_INT"]] = sum(v * dt for v in out_n); r[IDX["N_VIOL_MAX"]] = out_n.max() if out_n.size else 0.0
    r[IDX["N_ABS_MAX"]] = n_abs.max() if n_abs.size else 0.0
    r[IDX["ABNORMAL"]] = int((flags != 0).sum())
    r[IDX["OBJ_SUM"]] = sum(v for v, k in zip(obj, clean) if k); r[IDX["OBJ_CNT"]] = int(clean.sum())
    r[IDX["SLACK_N_CNT"]] = int(use_n.sum()); r[IDX["SLACK_TYRE_CNT"]] = int(use_t.sum())
    r[IDX["ELL_VIOL_INT"]] = sum(v * dt for v in out_e); r[IDX["ELL_VIOL_MAX"]] = out_e.max() if out_e.size else 0.0
    r[IDX["ITER_SUM"]] = sum(iters); r[IDX["ITER_MAX"]] = max(iters) if iters else 0
    r[IDX["S_START"]] = s_list[0] if s_list else 0.0; r[IDX["S_LAST"]] = s_list[-1] if s_list else 0.0
    return r


def records(h, dt, slack_tol=1e-6, params=None):
    """(B, 16).  params: None, one 32-entry block for all cars, or (B, 32)."""
    B = h["finished"].shape[1]
    P = None if params is None else np.asarray(params, dtype=np.float64)
    return np.stack([car_record(h, b, dt, slack_tol, None if P is None else (P if P.ndim == 1 else P[b])) for b in range(B)])


def _mean(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.sum(v) / v.size) if v.size else float("nan")     # MATLAB's mean([]) is NaN


def summary(rec, dt):
    """The batch summary of (B, 16) records as a dict keyed by SUMMARY."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 16)
    col = lambda name: rec[:, IDX[name]]
    st = col("STATUS")
    lap = col("STEPS")[st == 1] * dt
    steps = float(col("STEPS").sum())
    pct = lambda name: float(col(name).sum() / steps * 100) if steps > 0 else float("nan")
    drove = col("STEPS") > 0
    big = lambda name: float(col(name).max()) if rec.shape[0] else 0.0
    return {
        "CARS_DRIVING": float((st == 0).sum()), "CARS_FINISHED": float((st == 1).sum()), "CARS_LOST": float((st == 2).sum()),
        "LAP_MEAN": _mean(lap), "LAP_MIN": float(lap.min()) if lap.size else float("nan"), "LAP_MAX": float(lap.max()) if lap.size else float("nan"),
        "STEPS": steps, "ABNORMAL_PCT": pct("ABNORMAL"), "SLACK_N_PCT": pct("SLACK_N_CNT"), "SLACK_TYRE_PCT": pct("SLACK_TYRE_CNT"),
        "OBJ_MEAN": float(col("OBJ_SUM").sum() / col("OBJ_CNT").sum()) if col("OBJ_CNT").sum() > 0 else float("nan"),
        "N_VIOL_INT_MEAN": _mean(col("N_VIOL_INT")[drove]), "N_VIOL_INT_MAX": big("N_VIOL_INT"), "N_VIOL_MAX": big("N_VIOL_MAX"),
        "ELL_VIOL_INT_MEAN": _mean(col("ELL_VIOL_INT")[drove]), "ELL_VIOL_INT_MAX": big("ELL_VIOL_INT"), "ELL_VIOL_MAX": big("ELL_VIOL_MAX"),
        "ITER_MEAN": float(col("ITER_SUM").sum() / steps) if steps > 0 else float("nan"), "ITER_MAX": big("ITER_MAX"), "N_ABS_MAX": big("N_ABS_MAX"),
    }


def compare(got, want, tol=1e-10):
    """Count slots and STATUS exactly, the sums to tol absolute plus relative.  Returns the worst deviation of a sum."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 16), np.asarray(want, dtype=np.float64).reshape(-1, 16)
    assert got.shape == want.shape, (got.shape, want.shape)
    worst = 0.0
    for name in SLOTS:
        g, w = got[:, IDX[name]], want[:, IDX[name]]
        if name in COUNT_SLOTS:
            assert np.array_equal(g, w), (name, np.nonzero(g != w)[0][:8], g[g != w][:8], w[g != w][:8])
        else:
            err = np.abs(g - w) - tol * np.abs(w)
            assert (err <= tol).all(), (name, int(np.argmax(err)), g[np.argmax(err)], w[np.argmax(err)])
            worst = max(worst, float(np.abs(g - w).max()) if g.size else 0.0)
    return worst


# ---- the cars of the closed-loop tests (kinematic / dynamic N = 10 on fsg2019) --------------------------------------------------
def cart_on_track(otr, s, n, v):
    """Cartesian state [x, y, theta, v, 0, 0, 0] of a car at arc length s, lateral offset n, heading along the track (the Bezier table
    of the track on the host: point and tangent of segment floor(s / dl))."""
    r = np.mod(s, otr.dl * otr.M); i = min(int(np.floor(r / otr.dl)), otr.M - 1); u = r / otr.dl - i; w = 1 - u
    ev = lambda P: (P[i, 0] * w ** 3 + 3 * P[i, 1] * w * w * u + 3 * P[i, 2] * w * u * u + P[i, 3] * u ** 3,
                    (-3 * w * w * P[i, 0] + 3 * (3 * u * u - 4 * u + 1) * P[i, 1] + 3 * (2 * u - 3 * u * u) * P[i, 2] + 3 * u * u * P[i, 3]) / otr.dl)
    (x, xd), (y, yd) = ev(np.asarray(otr.xP)), ev(np.asarray(otr.yP))
    nrm = np.hypot(xd, yd)
    return np.array([x - yd / nrm * n, y + xd / nrm * n, np.arctan2(yd, xd), v, 0.0, 0.0, 0.0])


CAR_NAMES = ["centre", "off-line", "near end", "lost", "mirror"]


def starts(otr):
    """(s0, n0, v0) of the five cars: on the centre line; 0.15 m outside the track; 3 m before the end of the track parameter; 3.5 m off
    (out of the race at once); the off-line car mirrored."""
    return [(20.0, 0.0, 8.0), (20.0, 0.9, 8.0), (otr.L - 3.0, 0.0, 10.0), (20.0, 3.5, 8.0), (20.0, -0.9, 8.0)]


def cars(otr, B, st=None):
    """The five cars tiled to B: (cart (B, 7), s0 (B,), v0 (B,), kind (B,) index into CAR_NAMES)"""
    st = starts(otr) if st is None else st
    kind = np.arange(B) % len(st)
    cart = np.stack([cart_on_track(otr, *st[k]) for k in kind])
    return cart, np.array([st[k][0] for k in kind]), np.array([st[k][2] for k in kind]), kind


def is_lost(x0n, cart):
    """the loop's out-of-race rule on a pre-step result: 3 m off the 1.5 m wide track, or a state outside every physical range"""
    return not (np.isfinite(x0n[0]) and abs(x0n[1]) < 3.0 and abs(cart[3]) < 100.0 and abs(cart[4]) < 100.0 and (np.abs(cart) < 1e6).all())


def drive_oracle(orc, otr, model, N, dt, cart0, s0, v0, steps):
    """The closed loop of main.m:91-179 on the CPU oracle, one car at a time, with the plan initialised as the Monte-Carlo driver does
    (main.m:47-55 with s offset by s0 and speed by v0) and the loop's hand-over rule (a plan is taken over after exit flag 0 or 1 if it
    is finite).  Returns the history the restatement reads."""
    nx, ns = orc.dims(model, N)[:2]
    B = cart0.shape[0]
    h = dict(x0=np.zeros((steps, B, nx)), finished=np.zeros((steps, B), dtype=int), flag=np.zeros((steps, B), dtype=int),
             iter=np.zeros((steps, B), dtype=int), fval=np.zeros((steps, B)), slack=np.zeros((steps, B, ns)), a=np.zeros((steps, B)),
             cart=np.zeros((steps, B, 7)))
    k = np.arange(1, N + 1) * dt
    for b in range(B):
        cart, pid, fin = cart0[b].copy(), np.zeros(4), 0
        x_opt = np.zeros((N, nx)); u_opt = np.zeros((N, 2))
        x_opt[:, 0] = 10 * k ** 2 / 2 + s0[b]; x_opt[:, 3] = 10 * k + v0[b]; u_opt[:, 0] = 10
        for t in range(steps):
            if fin == 0:
                x0, x_ref, past = orc.cl_pre(model, N, dt, otr, cart, x_opt[0, 0])
                fin = 2 if is_lost(x0, cart) else (1 if past else 0)
                h["x0"][t, b] = x0
            h["finished"][t, b] = fin
            h["cart"][t, b] = cart
            if fin:
                continue
            u_new, x_new, slack, fval, flag, it = orc.ltv_step(model, otr, N, dt, x0, x_ref, x_opt.T, u_opt.T)
            if flag in (0, 1) and np.isfinite(x_new).all() and np.isfinite(u_new).all():
                x_opt, u_opt = x_new.reshape(N, nx).copy(), u_new.reshape(N, 2).copy()
            if np.isfinite(x_opt[0, 3]) and np.isfinite(x_opt[0, nx - 1]):
                cart, pid, _ = orc.plant_step(cart, pid, x_opt[0, 3], x_opt[0, nx - 1], dt)
            h["flag"][t, b], h["iter"][t, b], h["fval"][t, b], h["slack"][t, b], h["a"][t, b], h["cart"][t, b] = flag, it, fval, slack, u_opt[0, 0], cart
    return h
