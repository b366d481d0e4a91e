"""numpy restatement of the three kernels every closed-loop feature stands on (csrc/plant.hip, csrc/cl_frame.h): the frame transform
with x0, lap check, out-of-race rule and live reference (cl_pre_kernel, cl_pre_plan_kernel's frame part), the actuator loops and the
plant with its hold rules (cl_plant_kernel), and the plan take-over (cl_accept_kernel).  Written from the reference's own files --
spline/closest_point.m, vehicle_models/cartesian_to_curvilinear.m, spline/interpolate_spline{,_d,_dd}.m, spline/interpolate_angle.m,
vehicle_models/pid_controller.m, cartesian_dynamic/f_cart_dyn.m, integrate_cart_dyn.m (its stage formulas as written, the doubled
k2 term of k5 included), main.m:93-114 and main.m:163-175 -- not from the C of the oracle or the kernels.  What this project adds to
the reference is stated where it applies and named as such: the index guards of the segment lookup, the 1000-step guard of the
Newton search, the out-of-race rule (imported from lap_numpy.is_lost: it exists once), the hold rules and the accept rule.

Every function takes a dtype, np.float64 or np.longdouble (as tests/dual_numpy.py): run at np.longdouble this file is the reference
of tests/test_frame_gpu.py, and the gap between its two runs (e64) is the error a correct double implementation makes.  A track is any
object with xP, yP (M x 4), M, dl and L.  Parameter blocks are read with tests/param_numpy.py's g(); every literal is the double the
reference's text denotes, carried into the dtype (so x_d = -0.01 meets the slip angles' + 0.01 exactly in both).  `info`, where a
function takes it, is a dict that receives the discrete outcomes of the call (Newton steps, ramp sides, saturated sides)."""
import numpy as np

import lap_numpy as ln
import param_numpy as pn
from dual_numpy import default_block

PI = np.pi          # MATLAB's pi: the double


def mmod(a, b):
    """MATLAB mod(a, b) for b > 0"""
    return a - np.floor(a / b) * b


def seg_lookup(track, t, dtype):
    """interpolate_spline.m: t = mod(t, dl * length(P)); i = floor(t / dl) + 1; t = t / dl - (i - 1) -> (i - 1, t).
    Rule of this project (csrc/nlp_model.h seg_lookup): a remainder outside [0, period) -- a rounding of mod, or a non-finite arc
    length -- indexes no other row than 0 .. M - 1, and a non-finite one indexes row 0."""
    dl = dtype(track.dl)
    per = dl * track.M
    r = mmod(dtype(t), per)
    if r < 0:
        r = r + per
    if r >= per:
        r = r - per
    i = 0
    if r >= 0 and r < per:
        i = int(np.floor(r / dl))
    i = min(max(i, 0), track.M - 1)
    return i, r / dl - i


def spline3(track, P, t, dtype):
    """value, first and second derivative of one Bezier spline at arc length t (interpolate_spline.m, _d.m, _dd.m)"""
    i, u = seg_lookup(track, t, dtype)
    dl = dtype(track.dl)
    p0, p1, p2, p3 = (dtype(P[i, j]) for j in range(4))
    v = p0 * (1 - u) ** 3 + 3 * p1 * (1 - u) ** 2 * u + 3 * p2 * (1 - u) * u ** 2 + p3 * u ** 3
    d = (-3 * (1 - u) ** 2 * p0 + 3 * (3 * u ** 2 - 4 * u + 1) * p1 + 3 * (2 * u - 3 * u ** 2) * p2 + 3 * u ** 2 * p3) / dl
    dd = (6 * (1 - u) * p0 + 6 * (3 * u - 2) * p1 + 6 * (1 - 3 * u) * p2 + 6 * u * p3) / dl ** 2
    return v, d, dd


def closest_point(track, x0, y0, s, epsilon, dtype):
    """closest_point.m: Newton on the squared distance.  Returns (s, steps).  Rule of this project: at most 1000 steps (the
    reference spins for ever on a NaN)."""
    x0, y0, s, epsilon = dtype(x0), dtype(y0), dtype(s), dtype(epsilon)
    delta = epsilon * 2
    steps = 0
    while abs(delta) > epsilon and steps < 1000:
        X, Xd, Xdd = spline3(track, track.xP, s, dtype)
        Y, Yd, Ydd = spline3(track, track.yP, s, dtype)
        dist_d = 2 * (X - x0) * Xd + 2 * (Y - y0) * Yd
        dist_dd = 2 * (X - x0) * Xdd + 2 * Xd ** 2 + 2 * (Y - y0) * Ydd + 2 * Yd ** 2
        delta = dist_d / dist_dd
        s = s - delta
        steps += 1
    return s, steps


def angdiff(alpha, beta, dtype):
    """MATLAB angdiff(alpha, beta) = wrapToPi(beta - alpha).  wrapToPi leaves a value inside [-pi, pi] as it is; any other goes through
    wrapTo2Pi(d + pi) - pi, where wrapTo2Pi is mod(., 2 pi) with 2 pi instead of 0 for a positive argument."""
    pi = dtype(PI)
    d = dtype(beta) - dtype(alpha)
    if -pi <= d <= pi:
        return d
    w = mmod(d + pi, 2 * pi)
    if w == 0 and d + pi > 0:
        w = 2 * pi
    return w - pi


def cart_to_curv(track, x, y, theta, s0, dtype, info=None):
    """cartesian_to_curvilinear.m -> (s, n, mu)"""
    x, y = dtype(x), dtype(y)
    s, steps = closest_point(track, x, y, s0, 0.01, dtype)
    if info is not None:
        info["newton"] = steps
    X, Xd, _ = spline3(track, track.xP, s, dtype)
    Y, Yd, _ = spline3(track, track.yP, s, dtype)
    tx, ty = -Yd, Xd
    nrm = np.sqrt(tx * tx + ty * ty)
    n = (x - X) * (tx / nrm) + (y - Y) * (ty / nrm)
    mu = angdiff(np.arctan2(Yd, Xd), theta, dtype)       # interpolate_angle.m
    return s, n, mu


def pre(model, N, dt, target_vel, track, cart, s_guess, dtype, info=None):
    """main.m:93-114 for one car -> x0 (nx,), x_ref (N, nx), finished: 0 driving, 1 s >= L, 2 out of the race.  Rule of this project:
    a car that lap_numpy.is_lost() declares out gets x0 = 0 as finite placeholder data, and its reference ramps from that placeholder
    (the test of main.m:107 still reads the car's own x(4))."""
    with np.errstate(all="ignore"):
        cart = np.array([dtype(v) for v in cart], dtype=dtype)
        dt, target_vel = dtype(dt), dtype(target_vel)
        s, n, mu = cart_to_curv(track, cart[0], cart[1], cart[2], s_guess, dtype, info)
        if model == 0:
            x0 = np.array([s, n, mu, np.sqrt(cart[3] ** 2 + cart[4] ** 2), cart[6]], dtype=dtype)     # norm(x(4:5))
        else:
            x0 = np.array([s, n, mu, cart[3], cart[4], cart[5], cart[6]], dtype=dtype)
        finished = 1 if s >= dtype(track.L) else 0
        if ln.is_lost(x0, cart):
            finished = 2
            x0 = np.zeros(x0.size, dtype=dtype)
        x_ref = np.zeros((N, x0.size), dtype=dtype)
        up = bool(cart[3] < target_vel)
        sides = []
        cum = dtype(0)
        for k in range(N):      # main.m:107-114: start : step : end is start + k * step, i.e. x0(4) +- 10 dt (k + 1)
            if up:
                v = x0[3] + 10 * dt * (k + 1)
                clip = bool(v > target_vel)
            else:
                v = x0[3] - 10 * dt * (k + 1)
                clip = bool(v < target_vel)
            if clip:
                v = target_vel
            sides.append(clip)
            x_ref[k, 3] = v
            cum = cum + v * dt
            x_ref[k, 0] = x0[0] + cum
        if info is not None:
            info["ramp"] = (up, tuple(sides))
            info["finished"] = finished
    return x0, x_ref, finished


def f_cart_dyn(P, x, u, dtype):
    """f_cart_dyn.m:13-54 with the car's constants from the block P (None: the reference's own)"""
    P = default_block(1) if P is None else P
    m, iz, lf, lr, grav = (dtype(pn.g(P, k)) for k in ("M", "IZ", "LF", "LR", "GRAV"))
    B, C, D, E = (dtype(pn.g(P, k)) for k in ("PB", "PC", "PD", "PE"))
    theta, x_d, y_d, theta_d, delta = x[2], x[3], x[4], x[5], x[6]
    Fx, delta_d = u[0], u[1]
    alpha_f = delta - np.arctan((y_d + lf * theta_d) / (x_d + dtype(0.01)))
    alpha_r = -np.arctan((y_d - lr * theta_d) / (x_d + dtype(0.01)))
    Fzf = m * grav * lr / (lr + lf)
    Fzr = m * grav * lf / (lr + lf)
    Fcf = Fzf * D * np.sin(C * np.arctan(B * alpha_f - E * (B * alpha_f - np.arctan(B * alpha_f))))
    Fcr = Fzr * D * np.sin(C * np.arctan(B * alpha_r - E * (B * alpha_r - np.arctan(B * alpha_r))))
    return np.array([x_d * np.cos(theta) - y_d * np.sin(theta),
                     x_d * np.sin(theta) + y_d * np.cos(theta),
                     theta_d,
                     (Fx - Fcf * np.sin(delta) + m * y_d * theta_d) / m,
                     (Fcr + Fcf * np.cos(delta) - m * x_d * theta_d) / m,
                     (lf * Fcf * np.cos(delta) - lr * Fcr) / iz,
                     delta_d], dtype=dtype)


def integrate_cart_dyn(P, x, u, dt, dtype):
    """integrate_cart_dyn.m:12-22, stage formulas as written (k5 takes k2 twice and no k3)"""
    f = lambda xx: f_cart_dyn(P, xx, u, dtype)
    k1 = f(x)
    k2 = f(x + k1 * dt / 2)
    k3 = f(x + k1 * dt / 4 + k2 * dt / 8)
    k4 = f(x - k2 * dt + 2 * k3 * dt)
    k5 = f(x + dtype(7) / 27 * k2 * dt + dtype(10) / 27 * k2 * dt + k4 * dt / 27)
    k6 = f(x + dtype(28) / 625 * k1 * dt - k2 * dt / 5 + dtype(546) / 625 * k3 * dt + dtype(54) / 625 * k4 * dt - dtype(378) / 625 * k5 * dt)
    return x + dt * (k1 / 24 + dtype(5) / 48 * k4 + dtype(27) / 56 * k5 + dtype(125) / 336 * k6)


def pid(target, current, settings, status, dtype):
    """pid_controller.m:5-18 -> (output, status, side): settings (kp, ki, kd, max_output), status (integral, last error); side is
    -1 / 0 / +1 for an output clipped below / not clipped / clipped above.  MATLAB's min and max skip a NaN, as fmin and fmax do."""
    kp, ki, kd, max_output = (dtype(v) for v in settings)
    error = target - current
    integral_error = status[0] + error
    derivative_error = error - status[1]
    raw = kp * error + ki * integral_error + kd * derivative_error
    output = np.fmax(np.fmin(raw, max_output), -max_output)
    side = 1 if raw > max_output else (-1 if raw < -max_output else 0)
    return output, np.array([integral_error, error], dtype=dtype), side


def plant_step(params, cart, pid_state, v_ref, delta_ref, dt, dtype, info=None):
    """main.m:171-175: ten sub-steps of the two actuator loops (gains main.m:84-88, from the block) and the integrator.
    -> cart (7,), pid (4,) = [vel integral, vel error, steer integral, steer error], u_last (2,)"""
    with np.errstate(all="ignore"):
        P = default_block(1) if params is None else params
        vel_set = (pn.g(P, "PID_KP_V"), 0.0, 0.0, pn.g(P, "PID_MAX_F"))
        steer_set = (pn.g(P, "PID_KP_D"), 0.0, 0.0, pn.g(P, "PID_MAX_DRATE"))
        x = np.array([dtype(v) for v in cart], dtype=dtype)
        st = np.array([dtype(v) for v in pid_state], dtype=dtype)
        v_ref, delta_ref, dt = dtype(v_ref), dtype(delta_ref), dtype(dt)
        u = np.zeros(2, dtype=dtype)
        sides = []
        for _ in range(10):
            u[0], st[0:2], sv = pid(v_ref, x[3], vel_set, st[0:2], dtype)
            u[1], st[2:4], sd = pid(delta_ref, x[6], steer_set, st[2:4], dtype)
            sides.append((sv, sd))
            x = integrate_cart_dyn(P, x, u, dt / 10, dtype)
        if info is not None:
            info["pid"] = tuple(sides)
    return x, st, u


def block_is_bad(P):
    """Rule of this project (csrc/mpc_params.h): a block describes no car when an entry is non-finite, M, IZ or Q_TERMINAL is not
    > 0, a weight, slack cost or limit is negative, or LF + LR is not > 0."""
    P = np.asarray(P, dtype=np.float64)
    free = {"LF", "LR", "GRAV", "PB", "PC", "PD", "PE", "V_MIN", "PID_KP_V", "PID_KP_D"}
    bad = not np.isfinite(P).all()
    for name, i in pn.IDX.items():
        if name in ("M", "IZ", "Q_TERMINAL"):
            bad = bad or not P[i] > 0
        elif name not in free:
            bad = bad or not P[i] >= 0
    return bool(bad or not pn.g(P, "LR") + pn.g(P, "LF") > 0)


def plant(params, cart, pid_state, u_last, v_ref, delta_ref, dt, finished, exitflag, bad_block, dtype, info=None):
    """The plant of one car with this project's hold rules: a car whose block is bad, that is no longer driving (finished 1 or 2),
    whose caller's marker is below -100 (exitflag None: no marker; a solver's flag never holds a car, main.m:163-175), or whose set
    points are not finite keeps cart, pid and u_last as they are.  -> (cart, pid, u_last, held)"""
    held = bool(bad_block) or finished != 0 or (exitflag is not None and exitflag < -100) or not np.isfinite(v_ref) or not np.isfinite(delta_ref)
    if held:
        return (np.array(cart, dtype=dtype), np.array(pid_state, dtype=dtype), np.array(u_last, dtype=dtype), True)
    return plant_step(params, cart, pid_state, v_ref, delta_ref, dt, dtype, info) + (False,)


def accept(x_new, u_new, exitflag, x_keep, u_keep):
    """The take-over of one car's plan (main.m:122-126 with this project's rule): the new plan replaces the kept one after exit flag
    0 or 1 (None: no flags) when every entry of it is finite.  -> (x_keep, u_keep)"""
    ok = exitflag is None or exitflag in (0, 1)
    ok = ok and bool(np.isfinite(x_new).all()) and bool(np.isfinite(u_new).all())
    return (np.array(x_new), np.array(u_new)) if ok else (np.array(x_keep), np.array(u_keep))
