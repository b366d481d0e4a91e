"""Numpy restatement of the closed loop's state estimator (include/fsaempc.h, fsaempc_cl_estimate_batch_device), sharing no
code with csrc/cl_estimator.h / .hip: the scalar rules, the sequential scalar update, the textbook joint update it must equal, the
finite-difference Jacobian of param_numpy.psi and one period of one car.  tests/test_estimator_cpu.py pins the pieces; the GPU tests
compare the device against period()."""
import numpy as np

import param_numpy as pp


def finite(v):
    return bool(np.abs(v) < np.inf)


def measured(r):
    """Component measured iff its variance is finite and >= 0 (NaN, negative, +inf: not measured)."""
    return bool(r >= 0.0 and r < np.inf)


def rebase(x, z, L, s_measured):
    """The arc length x of the prior moved by whole laps towards the measurement z (ties of rint to even)."""
    if not (L > 0.0) or not s_measured:
        return x
    return x + L * np.rint((z - x) / L)


def prior_bad(v, diag):
    return (not finite(v)) or (diag and not (v > 0.0))


def post_bad(v, diag):
    return (not finite(v)) or (diag and v < 0.0)


def seq_update(x, P, z, r):
    """Sequential scalar update.  Returns (x, P, innov, nis)."""
    x = np.array(x, dtype=np.float64); P = np.array(P, dtype=np.float64)
    nx = x.size
    innov = np.zeros(nx); nis = 0.0
    with np.errstate(all="ignore"):
        for i in range(nx):
            if not measured(r[i]):
                continue
            nu = z[i] - x[i]
            s = P[i, i] + r[i]
            innov[i] = nu
            if not (s > 0.0):
                continue
            c = P[:, i].copy()
            nis = nis + nu * nu / s
            x = x + c * nu / s
            P = P - np.outer(c, c) / s
    return x, P, innov, nis


def joint_update(x, P, z, r):
    """The textbook update with H = the measured rows of I: K = P H' (H P H' + R)^-1.  Returns (x, P, nis)."""
    idx = [i for i in range(len(x)) if measured(r[i])]
    if not idx:
        return np.array(x, dtype=np.float64), np.array(P, dtype=np.float64), 0.0
    H = np.eye(len(x))[idx]
    S = H @ P @ H.T + np.diag(np.asarray(r, dtype=np.float64)[idx])
    K = np.linalg.solve(S, H @ P).T                    # P H' S^-1 (P and S symmetric)
    nu = np.asarray(z, dtype=np.float64)[idx] - H @ x
    return x + K @ nu, P - K @ H @ P, float(nu @ np.linalg.solve(S, nu))


def fd_jacobian(f, x, h):
    """Central differences of f at x with the steps h (per component), h / 2 and h / 4, Richardson-extrapolated pairwise: returns (J, gap)
    with J the extrapolation of the finer pair and gap its largest distance from the extrapolation of the coarser pair, an estimate of the
    coarser one's error (the finer one's is about 16 times smaller until rounding takes over)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size

    def level(hh):
        J = np.zeros((f(x).size, n))
        for k in range(n):
            e = np.zeros(n); e[k] = hh[k]
            J[:, k] = (f(x + e) - f(x - e)) / (2 * hh[k])
        return J
    h = np.asarray(h, dtype=np.float64)
    d1, d2, d4 = level(h), level(h / 2), level(h / 4)
    coarse, fine = (4 * d2 - d1) / 3, (4 * d4 - d2) / 3
    return fine, float(np.abs(fine - coarse).max())


def psi_jacobian(P, orc, model, track, x, u, dt, integ, h=1e-3):
    """The Jacobian of param_numpy.psi in x by fd_jacobian with the absolute step h in every component (an arc length must not be
    stepped in proportion to its size: the stencil has to stay inside one spline segment, kappa' jumps at the joints)."""
    f = lambda xx: pp.psi(P, orc, model, track, xx, u, dt, integ)
    return fd_jacobian(f, x, np.full(len(x), float(h)))


def period(est_x, est_P, count, z, x_start, u, finished, q, r, p0, L, predict, par_bad=False):
    """One period of one car.  count: (periods since the last (re-)initialisation, resets).  predict(x, u) -> (x-, F).  Returns a dict
    with est_x, est_P, count, x0_est, innov, nis, F_out, x_prior."""
    nx = len(z)
    z = np.asarray(z, dtype=np.float64); q = np.asarray(q, dtype=np.float64); r = np.asarray(r, dtype=np.float64); p0 = np.asarray(p0, dtype=np.float64)
    if finished:
        return dict(est_x=np.array(est_x), est_P=np.array(est_P), count=tuple(count), x0_est=z.copy(), innov=np.zeros(nx), nis=0.0, F_out=np.eye(nx),
                    x_prior=z.copy())
    c0, c1 = count
    with np.errstate(all="ignore"):
        if c0 == 0:
            xm, Pm, F = np.array(x_start, dtype=np.float64), np.diag(p0), np.eye(nx)
        else:
            xm, F = predict(np.asarray(est_x, dtype=np.float64), np.asarray(u, dtype=np.float64))
            M = (F @ np.asarray(est_P, dtype=np.float64)) @ F.T
            Pm = 0.5 * (M + M.T) + np.diag(q)
        bad = par_bad or not np.isfinite(u).all() or any(prior_bad(v, False) for v in xm) or \
            any(prior_bad(Pm[a, b], a == b) for a in range(nx) for b in range(nx))
        resets = 0
        if bad:
            xm, Pm, resets, c0 = z.copy(), np.diag(p0), 1, 0
        xm = np.array(xm, dtype=np.float64)
        xm[0] = rebase(xm[0], z[0], L, measured(r[0]))
        x, Pn, innov, nis = seq_update(xm, Pm, z, r)
        if any(post_bad(v, False) for v in x) or any(post_bad(Pn[a, b], a == b) for a in range(nx) for b in range(nx)):
            resets += 1; c0 = 0
            x, Pn, innov, nis = seq_update(z, np.diag(p0), z, r)
    return dict(est_x=x, est_P=Pn, count=(c0 + 1, c1 + resets), x0_est=x.copy(), innov=innov, nis=nis, F_out=F, x_prior=xm)
