"""Numpy restatement of the closed loop's Cartesian sensor models (include/fsaempc.h, fsaempc_cl_sense_batch_device and
fsaempc_cl_estimate_cart_batch_device), sharing no code with csrc/cl_sensors.h / .hip: the sensor layout, the measurement with the draws
of tests/latency_numpy.py, the naive projection through tests/frame_numpy.py, the measurement function h on floats and on the dual
numbers of tests/dual_numpy.py (so H is the derivative of the very formulas, not a hand Jacobian), the heading wrap, the row-by-row
update, the textbook joint update it must equal, and one period of one car on the rules of tests/estimator_numpy.py.  The float64
functions restate csrc/cl_sensors.h operation for operation: tests/test_sensors_cpu.py holds the header, built for the host under the
sanitizers, to them bit for bit; the GPU tests compare the kernels against measure(), project() and period().

A track is any object with xP, yP (M x 4), M, dl and L (oracle.Track, dual_numpy.Table)."""
import math

import numpy as np

import estimator_numpy as en
import frame_numpy as fn
import lap_numpy as ln
import latency_numpy as lt
from dual_numpy import Dual, val

PI = np.pi


def nx_of(model):
    return 5 if model == 0 else 7


# ---- the sensor layout ----
def y_true(model, cart):
    """The exact measurement out of the plant's 7 Cartesian states, as the pre-step assembles x0."""
    c = np.asarray(cart, dtype=np.float64)
    if model == 0:
        a, b = c[3] * c[3], c[4] * c[4]
        return np.array([c[0], c[1], c[2], np.sqrt(a + b), c[6]])
    return c.copy()


def cart_from_y(model, y):
    """The Cartesian vector a measurement stands for."""
    y = np.asarray(y)
    if model == 0:
        return np.array([y[0], y[1], y[2], y[3], 0.0, 0.0, y[4]], dtype=y.dtype)
    return y.copy()


def measure(model, cart, sigma, finished, seed, id0, step):
    """y (B, nx) = y_true + sigma z with the draws of (seed, id0 + b, step); a finished car and a sigma of 0 copy."""
    yt = np.stack([y_true(model, c) for c in cart])
    return lt.observe(yt, sigma, finished, seed, id0, step)


def project(track, model, y, s_true, x0_true, dtype=np.float64, info=None):
    """The naive projection of one car: the frame transform of frame_numpy on the Cartesian vector y stands for, Newton started at the
    true arc length; lost (lap_numpy.is_lost) -> x0_true itself.  Returns (x_proj, lost)."""
    with np.errstate(all="ignore"):
        c = np.array([dtype(v) for v in cart_from_y(model, np.asarray(y, dtype=np.float64))], dtype=dtype)
        s, n, mu = fn.cart_to_curv(track, c[0], c[1], c[2], s_true, dtype, info)
        if model == 0:
            x = np.array([s, n, mu, np.sqrt(c[3] ** 2 + c[4] ** 2), c[6]], dtype=dtype)
        else:
            x = np.array([s, n, mu, c[3], c[4], c[5], c[6]], dtype=dtype)
        if ln.is_lost(x, c):
            return np.array([dtype(v) for v in x0_true], dtype=dtype), True
    return x, False


# ---- h(x) and H ----
def _atan2(y, x):
    """libm's atan2, as the host build calls it (numpy's vectorised arctan2 differs from it in the last bit on some inputs)"""
    return np.float64(math.atan2(y, x))


def dsqrt(a):
    if isinstance(a, Dual):
        r = np.sqrt(a.v)
        return Dual(r, a.d / (2.0 * r))
    return np.sqrt(a)


def datan2(y, x):
    if isinstance(y, Dual):
        num, den = x.v * y.d - y.v * x.d, x.v * x.v + y.v * y.v
        return Dual(_atan2(y.v, x.v), num / den)
    return _atan2(y, x)


def spline2(P, i, dl, u):
    """value and first derivative of one Bezier spline at the local parameter u (float or Dual) of segment i"""
    p0, p1, p2, p3 = (np.float64(P[i, k]) for k in range(4))
    w = 1 - u
    v = p0 * (w * w * w) + 3 * p1 * (w * w) * u + 3 * p2 * w * (u * u) + p3 * (u * u * u)
    d = (-3 * w * w * p0 + 3 * (3 * u * u - 4 * u + 1) * p1 + 3 * (2 * u - 3 * u * u) * p2 + 3 * u * u * p3) / dl
    return v, d


def h(track, x):
    """The measurement function (vehicle_models/curvilinear_to_cartesian.m:16-28) on a list of floats or of Duals -> list"""
    i, tau = fn.seg_lookup(track, np.float64(val(x[0])), np.float64)
    dl = np.float64(track.dl)
    u = Dual(tau, x[0].d / dl) if isinstance(x[0], Dual) else tau
    X, Xd = spline2(track.xP, i, dl, u)
    Y, Yd = spline2(track.yP, i, dl, u)
    tx, ty = -Yd, Xd
    nrm = dsqrt(tx * tx + ty * ty)
    tx, ty = tx / nrm, ty / nrm
    return [X + x[1] * tx, Y + x[1] * ty, datan2(Yd, Xd) + x[2]] + list(x[3:])


def h_values(track, x):
    with np.errstate(all="ignore"):
        return np.array(h(track, [np.float64(v) for v in x]), dtype=np.float64)


def linearise(track, x):
    """(h(x), H = dh/dx(x)): one pass of dual numbers per column"""
    n = len(x)
    H = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            out = h(track, [Dual(np.float64(x[k]), np.float64(1.0 if k == j else 0.0)) for k in range(n)])
            H[:, j] = [o.d for o in out]
            hv = np.array([o.v for o in out], dtype=np.float64)
    return hv, H


def angdiff(alpha, beta):
    """MATLAB angdiff(alpha, beta) in the form of the loop's kernels: mod(d + pi, 2 pi) - pi, +pi instead of -pi for a positive d"""
    d = np.float64(beta) - np.float64(alpha)
    a, b = d + PI, 2 * PI
    w = (a - np.floor(a / b) * b) - PI
    if w == -PI and d > 0:
        w = PI
    return w


def innovation0(y, h0):
    nu = np.asarray(y, dtype=np.float64) - np.asarray(h0, dtype=np.float64)
    nu[2] = angdiff(h0[2], y[2])
    return nu


# ---- the update ----
def row_update(x_prior, P, y, r, h0, H):
    """The EKF update linearised once at the prior (h0 = h(x-), H = dh/dx(x-)), processed row by row.  Returns (x, P, innov, nis)."""
    xm = np.array(x_prior, dtype=np.float64); x = xm.copy(); P = np.array(P, dtype=np.float64)
    nx = x.size
    innov = np.zeros(nx); nis = 0.0
    with np.errstate(all="ignore"):
        nu0 = innovation0(y, h0)
        for i in range(nx):
            if not en.measured(r[i]):
                continue
            nu = nu0[i] - H[i] @ (x - xm)
            c = P @ H[i]
            s = H[i] @ c + r[i]
            innov[i] = nu
            if not (s > 0.0):
                continue
            nis = nis + nu * nu / s
            x = x + c * nu / s
            P = P - np.outer(c, c) / s
    return x, P, innov, nis


def joint_update(x_prior, P, y, r, h0, H):
    """The textbook update with the measured rows of H: K = P H' (H P H' + R)^-1.  Returns (x, P, nis)."""
    x = np.array(x_prior, dtype=np.float64); P = np.array(P, dtype=np.float64)
    idx = [i for i in range(len(x)) if en.measured(r[i])]
    if not idx:
        return x, P, 0.0
    Hm = np.asarray(H, dtype=np.float64)[idx]
    S = Hm @ P @ Hm.T + np.diag(np.asarray(r, dtype=np.float64)[idx])
    K = np.linalg.solve(S, Hm @ P).T
    nu = innovation0(y, h0)[idx]
    return x + K @ nu, P - K @ Hm @ P, float(nu @ np.linalg.solve(S, nu))


def period(est_x, est_P, count, y, x_proj, u, finished, q, r, p0, L, predict, lin, par_bad=False):
    """One period of one car.  predict(x, u) -> (x-, F); lin(x) -> (h(x), H(x)).  Returns a dict with est_x, est_P, count, x0_est, innov,
    nis, F_out, x_prior, H_out."""
    nx = len(y)
    y = np.asarray(y, dtype=np.float64); xq = np.asarray(x_proj, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64); r = np.asarray(r, dtype=np.float64); p0 = np.asarray(p0, dtype=np.float64)
    if finished:
        return dict(est_x=np.array(est_x), est_P=np.array(est_P), count=tuple(count), x0_est=xq.copy(), innov=np.zeros(nx), nis=0.0, F_out=np.eye(nx),
                    x_prior=xq.copy(), H_out=np.eye(nx))
    c0, c1 = count
    with np.errstate(all="ignore"):
        if c0 == 0:
            xm, Pm, F = xq.copy(), np.diag(p0), np.eye(nx)
        else:
            xm, F = predict(np.asarray(est_x, dtype=np.float64), np.asarray(u, dtype=np.float64))
            M = (F @ np.asarray(est_P, dtype=np.float64)) @ F.T
            Pm = 0.5 * (M + M.T) + np.diag(q)
        bad = par_bad or not np.isfinite(u).all() or any(en.prior_bad(v, False) for v in xm) or \
            any(en.prior_bad(Pm[a, b], a == b) for a in range(nx) for b in range(nx))
        resets = 0
        if bad:
            xm, Pm, resets, c0 = xq.copy(), np.diag(p0), 1, 0
        xm = np.array(xm, dtype=np.float64)
        xm[0] = en.rebase(xm[0], xq[0], L, True)
        h0, H = lin(xm)
        x, Pn, innov, nis = row_update(xm, Pm, y, r, h0, H)
        if any(en.post_bad(v, False) for v in x) or any(en.post_bad(Pn[a, b], a == b) for a in range(nx) for b in range(nx)):
            resets += 1; c0 = 0
            h0, H = lin(xq)
            x, Pn, innov, nis = row_update(xq, np.diag(p0), y, r, h0, H)
    return dict(est_x=x, est_P=Pn, count=(c0 + 1, c1 + resets), x0_est=x.copy(), innov=innov, nis=nis, F_out=F, x_prior=xm, H_out=H)
