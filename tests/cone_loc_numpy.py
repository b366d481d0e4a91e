"""Numpy restatement of the closed loop's cone-based localisation (include/fsaempc.h, fsaempc_cl_cone_sense_batch_device and
fsaempc_cl_estimate_cones_batch_device), sharing no code with csrc/cl_cone_loc.h / .hip or csrc/cl_sensors.hip: range and bearing of a cone,
the view test, the draws of a cone with the generator of tests/latency_numpy.py, the selection, the two rows of an observation on floats
(operation for operation) and on the dual numbers of tests/dual_numpy.py (so the rows are checked against the derivative of the very
formulas), the row-by-row update over own and cone rows, the joint update it must equal, and one period of one car on the rules of
tests/estimator_numpy.py and tests/sensors_numpy.py.  tests/test_cone_loc_cpu.py holds the header, built for the host under the
sanitizers, to the float64 functions bit for bit; the GPU tests compare the kernels against sense() and period().

A map is a pair (left (K_l, 2), right (K_r, 2)); cone g is left[g] for g < K_l and right[g - K_l] after that."""
import math

import numpy as np

import estimator_numpy as en
import latency_numpy as lt
import sensors_numpy as sn
from dual_numpy import Dual

OBS_MAX = 16     # FSAEMPC_CONE_OBS_MAX
INF = float("inf")
F = np.float64


def cone_at(left, right, g):
    left, right = np.asarray(left, dtype=F).reshape(-1, 2), np.asarray(right, dtype=F).reshape(-1, 2)
    return left[g] if g < len(left) else right[g - len(left)]


def count(left, right):
    return len(np.asarray(left).reshape(-1, 2)) + len(np.asarray(right).reshape(-1, 2))


# ---- the sensor ----
def polar(cx, cy, X, Y, psi):
    """(rho, beta) of the point (cx, cy) from the pose (X, Y, psi)"""
    dx, dy = F(cx) - F(X), F(cy) - F(Y)
    a, b = dx * dx, dy * dy
    return np.sqrt(a + b), sn.angdiff(psi, F(math.atan2(dy, dx)))


def in_view(rho, beta, r_min, r_max, fov):
    return bool(rho >= r_min and rho <= r_max and abs(beta) <= F(fov) / 2)


def observe1(x, sigma, z):
    """cll_observe: x + sigma z where sigma > 0 and finite, a copy everywhere else"""
    if not (sigma > 0.0 and sigma < INF):
        return F(x)
    e = F(sigma) * F(z)
    return F(x) + e


def detect(seed, cid, step, g, rho, beta, sigma_rho, sigma_beta, p_detect):
    """(detected, rho_m, beta_m) of cone g for car id `cid` in period `step`"""
    w = lt.words(seed, cid, step, 2 + g)
    z = lt.normals(w)
    u = (w[2] + 0.5) * 2.0 ** -32
    return bool(u < p_detect), observe1(rho, sigma_rho, z[0]), sn.angdiff(0.0, observe1(beta, sigma_beta, z[1]))


def select(rho, cand, k_max):
    """the min(count, k_max) candidates smallest by (rho, g), in that order -> (ids, seen)"""
    c = sorted((F(rho[g]), g) for g in range(len(rho)) if cand[g])
    return [g for _, g in c[:k_max]], len(c)


def sense_car(left, right, pose, cid, step, *, r_min, r_max, fov, sigma, p_detect, k_max, seed, finished=False):
    """One car.  dict: n, seen, ids (k_max,) with -1 past the count, z (k_max, 2) with 0 past it, and cand: [(g, rho, beta)] of every
    candidate (in view and detected), for the tests' margins."""
    ids, z = np.full(k_max, -1, dtype=np.int32), np.zeros((k_max, 2))
    if finished:
        return dict(n=0, seen=0, ids=ids, z=z, cand=[])
    K = count(left, right)
    rho, beta, cand, noisy = np.zeros(K), np.zeros(K), np.zeros(K, dtype=bool), {}
    with np.errstate(all="ignore"):
        for g in range(K):
            cx, cy = cone_at(left, right, g)
            rho[g], beta[g] = polar(cx, cy, pose[0], pose[1], pose[2])
            if not in_view(rho[g], beta[g], r_min, r_max, fov):
                continue
            det, rm, bm = detect(seed, cid, step, g, rho[g], beta[g], sigma[0], sigma[1], p_detect)
            cand[g] = det
            noisy[g] = (rm, bm)
    kept, seen = select(rho, cand, k_max)
    for k, g in enumerate(kept):
        ids[k] = g
        z[k] = noisy[g]
    return dict(n=len(kept), seen=seen, ids=ids, z=z, cand=[(g, rho[g], beta[g]) for g in range(K) if cand[g]])


def sense(left, right, cart, id0, step, finished=None, **kw):
    """The batch: left / right (K, 2) shared or (B, K, 2) per car.  dict of arrays n, seen (B,), ids (B, k_max), z (B, k_max, 2); cand a list."""
    left, right = np.asarray(left, dtype=F), np.asarray(right, dtype=F)
    out = [sense_car(left[b] if left.ndim == 3 else left, right[b] if right.ndim == 3 else right, cart[b], id0 + b, step,
                     finished=bool(finished is not None and finished[b] != 0), **kw) for b in range(len(cart))]
    return dict(n=np.array([o["n"] for o in out], dtype=np.int32), seen=np.array([o["seen"] for o in out], dtype=np.int32),
                ids=np.stack([o["ids"] for o in out]), z=np.stack([o["z"] for o in out]), cand=[o["cand"] for o in out])


# ---- the rows ----
def rows(h0, h1, h2, Hr, mx, my, rho_m, beta_m):
    """The two rows of one observation at the linearisation point, operation for operation -> (G (2, 3), nu0 (2,), rho_hat)"""
    Hr = np.asarray(Hr, dtype=F)
    with np.errstate(all="ignore"):
        dx, dy = F(mx) - F(h0), F(my) - F(h1)
        a, b = dx * dx, dy * dy
        q2 = a + b
        rho_hat = np.sqrt(q2)
        beta_hat = sn.angdiff(h2, F(math.atan2(dy, dx)))
        g = [[-dx / rho_hat, -dy / rho_hat, F(0.0)], [dy / q2, -dx / q2, F(-1.0)]]
        G = np.zeros((2, 3))
        for i in range(2):
            for c in range(3):
                acc = F(0.0)
                for k in range(3):
                    acc = acc + g[i][k] * Hr[k, c]
                G[i, c] = acc
        nu0 = np.array([F(rho_m) - rho_hat, sn.angdiff(beta_hat, beta_m)])
    return G, nu0, rho_hat


def composite(track, x, mx, my):
    """x -> (rho, beta) of the map cone (mx, my) from the pose h(x), on a list of floats or of Duals (the bearing's value is wrapped,
    its derivative is that of atan2(dy, dx) - h2)"""
    hv = sn.h(track, x)
    dx, dy = mx - hv[0], my - hv[1]
    rho = sn.dsqrt(dx * dx + dy * dy)
    ang = sn.datan2(dy, dx)
    if isinstance(ang, Dual):
        return rho, Dual(sn.angdiff(hv[2].v, ang.v), ang.d - hv[2].d)
    return rho, sn.angdiff(hv[2], ang)


def composite_values(track, x, mx, my):
    with np.errstate(all="ignore"):
        r, b = composite(track, [F(v) for v in x], F(mx), F(my))
    return np.array([r, b], dtype=F)


def composite_jacobian(track, x, mx, my):
    """d(rho, beta)/dx by dual numbers through h and the polar formulas: (2, nx)"""
    n = len(x)
    J = np.zeros((2, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            r, b = composite(track, [Dual(F(x[k]), F(1.0 if k == j else 0.0)) for k in range(n)], F(mx), F(my))
            J[:, j] = [r.d, b.d]
    return J


# ---- the update ----
def cone_list(left, right, n, ids, z):
    """The observations of one car as the update reads them: [(id, (mx, my) or None for an id outside the map, rho_m, beta_m)]"""
    K = count(left, right)
    out = []
    for k in range(int(n)):
        g = int(ids[k])
        out.append((g, tuple(cone_at(left, right, g)) if 0 <= g < K else None, F(z[k][0]), F(z[k][1])))
    return out


def row_update(x_prior, P, y, r, h0, H, cones, r_cone, k_max=OBS_MAX):
    """The EKF update linearised once at the prior (h0 = h(x-), H = dh/dx(x-)), processed row by row: the own rows of
    sensors_numpy.row_update, then per observation its range row and its bearing row.  cones: cone_list().  Returns a dict x, P, innov,
    nis, cone_innov (k_max, 2), rows, G (k_max, 2, 3)."""
    xm = np.array(x_prior, dtype=F); x = xm.copy(); P = np.array(P, dtype=F)
    nx = x.size
    innov, nis, used = np.zeros(nx), F(0.0), 0
    cone_innov, Gout = np.zeros((k_max, 2)), np.zeros((k_max, 2, 3))
    with np.errstate(all="ignore"):
        nu0 = sn.innovation0(y, h0)
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
            used += 1
        Hr = np.asarray(H, dtype=F)[:3, :3]
        for k, (g, pos, zr, zb) in enumerate(cones[:k_max]):
            if pos is None:
                continue
            G, n0, rho_hat = rows(h0[0], h0[1], h0[2], Hr, pos[0], pos[1], zr, zb)
            for i in range(2):
                if not (rho_hat > 0.0) or not en.measured(r_cone[i]):
                    continue
                hx = F(0.0)
                for q in range(3):
                    hx = hx + G[i, q] * (x[q] - xm[q])
                c = np.zeros(nx)
                for a in range(nx):
                    acc = F(0.0)
                    for q in range(3):
                        acc = acc + P[a, q] * G[i, q]
                    c[a] = acc
                hc = F(0.0)
                for q in range(3):
                    hc = hc + G[i, q] * c[q]
                nu, s = n0[i] - hx, hc + F(r_cone[i])
                if not (s > 0.0):
                    continue
                cone_innov[k, i] = nu
                Gout[k, i] = G[i]
                nis = nis + nu * nu / s
                x = x + c * nu / s
                P = P - np.outer(c, c) / s
                used += 1
    return dict(x=x, P=P, innov=innov, nis=float(nis), cone_innov=cone_innov, rows=used, G=Gout)


def stacked(x_prior, y, r, h0, H, cones, r_cone):
    """The rows a joint update stacks: (Hs, nu, R diagonal) over the measured own rows and the applicable cone rows"""
    nx = len(x_prior)
    Hs, nu, R = [], [], []
    nu0 = sn.innovation0(y, h0)
    for i in range(nx):
        if en.measured(r[i]):
            Hs.append(np.asarray(H[i], dtype=F)); nu.append(nu0[i]); R.append(r[i])
    Hr = np.asarray(H, dtype=F)[:3, :3]
    for g, pos, zr, zb in cones:
        if pos is None:
            continue
        G, n0, rho_hat = rows(h0[0], h0[1], h0[2], Hr, pos[0], pos[1], zr, zb)
        for i in range(2):
            if rho_hat > 0.0 and en.measured(r_cone[i]):
                row = np.zeros(nx); row[:3] = G[i]
                Hs.append(row); nu.append(n0[i]); R.append(r_cone[i])
    return np.array(Hs).reshape(-1, nx), np.array(nu), np.array(R)


def joint_update(x_prior, P, y, r, h0, H, cones, r_cone):
    """The textbook update on the stacked own and cone rows: K = P H' (H P H' + R)^-1.  Returns (x, P, nis)."""
    x = np.array(x_prior, dtype=F); P = np.array(P, dtype=F)
    Hs, nu, R = stacked(x, y, r, h0, H, cones, r_cone)
    if not len(nu):
        return x, P, 0.0
    S = Hs @ P @ Hs.T + np.diag(R)
    K = np.linalg.solve(S, Hs @ P).T
    return x + K @ nu, P - K @ Hs @ P, float(nu @ np.linalg.solve(S, nu))


def period(est_x, est_P, count_, y, x_proj, u, finished, q, r, p0, L, predict, lin, cones, r_cone, k_max=OBS_MAX, par_bad=False):
    """One period of one car: sensors_numpy.period with the cone rows in both runs of the update.  predict(x, u) -> (x-, F);
    lin(x) -> (h(x), H(x)).  Returns its dict plus cone_innov, rows and G."""
    nx = len(y)
    y = np.asarray(y, dtype=F); xq = np.asarray(x_proj, dtype=F)
    q = np.asarray(q, dtype=F); r = np.asarray(r, dtype=F); p0 = np.asarray(p0, dtype=F)
    if finished:
        return dict(est_x=np.array(est_x), est_P=np.array(est_P), count=tuple(count_), x0_est=xq.copy(), innov=np.zeros(nx), nis=0.0, F_out=np.eye(nx),
                    x_prior=xq.copy(), H_out=np.eye(nx), cone_innov=np.zeros((k_max, 2)), rows=0, G=np.zeros((k_max, 2, 3)))
    c0, c1 = count_
    with np.errstate(all="ignore"):
        if c0 == 0:
            xm, Pm, Fm = xq.copy(), np.diag(p0), np.eye(nx)
        else:
            xm, Fm = predict(np.asarray(est_x, dtype=F), np.asarray(u, dtype=F))
            M = (Fm @ np.asarray(est_P, dtype=F)) @ Fm.T
            Pm = 0.5 * (M + M.T) + np.diag(q)
        bad = par_bad or not np.isfinite(u).all() or any(en.prior_bad(v, False) for v in xm) or \
            any(en.prior_bad(Pm[a, b], a == b) for a in range(nx) for b in range(nx))
        resets = 0
        if bad:
            xm, Pm, resets, c0 = xq.copy(), np.diag(p0), 1, 0
        xm = np.array(xm, dtype=F)
        xm[0] = en.rebase(xm[0], xq[0], L, True)
        h0, H = lin(xm)
        o = row_update(xm, Pm, y, r, h0, H, cones, r_cone, k_max)
        if any(en.post_bad(v, False) for v in o["x"]) or any(en.post_bad(o["P"][a, b], a == b) for a in range(nx) for b in range(nx)):
            resets += 1; c0 = 0
            h0, H = lin(xq)
            o = row_update(xq, np.diag(p0), y, r, h0, H, cones, r_cone, k_max)
    return dict(est_x=o["x"], est_P=o["P"], count=(c0 + 1, c1 + resets), x0_est=o["x"].copy(), innov=o["innov"], nis=o["nis"], F_out=Fm, x_prior=xm,
                H_out=H, cone_innov=o["cone_innov"], rows=o["rows"], G=o["G"])
