"""Numpy statement of the minimum-time racing line of DESIGN.md 6o (csrc/minlap.h, csrc/minlap.hip), operation for operation: the
profile of raceline_numpy.line_profile on a line with the bookkeeping the reverse sweep needs, the adjoint of that profile (the two
passes undone in reverse order, then curvature, length and heading offset per cell, then the basis), one iteration with the oracle's
qp_solve for the candidate steps, and the loop."""
import numpy as np

import plan_numpy as pn
import raceline_numpy as rn

RHO_DEFAULT = (1e4, 3e3, 1e3, 300.0, 100.0, 30.0, 10.0, 3.0)
MINLAP_MAX_NS = 1024
WON_FWD, WON_BWD = 1, 2


def a_x(model, cst, grip, A_lat, v, K):
    """(a_x, d a_x / d v, d a_x / d K): plan_numpy.a_x with the slope of the polygon edge; zero partials where U_ACC_MAX or y = 1 is
    the active branch."""
    if model == 0:
        return grip * cst["U_ACC_MAX"], 0.0, 0.0
    y0 = v * v * K / A_lat
    y = min(y0, 1.0)
    j = 0 if y <= pn.POLY_S[1] else (1 if y <= pn.POLY_S[2] else 2)
    c0, c1, s0, s1 = pn.POLY_C[j], pn.POLY_C[j + 1], pn.POLY_S[j], pn.POLY_S[j + 1]
    X = c0 + (c1 - c0) * (y - s0) / (s1 - s0)
    val = grip * cst["ELL_LONG"] * X
    dv = dK = 0.0
    if val < cst["U_ACC_MAX"] and y0 < 1.0:
        slope = grip * cst["ELL_LONG"] * ((c1 - c0) / (s1 - s0))
        dv = slope * (2.0 * v * K / A_lat)
        dK = slope * (v * v / A_lat)
    return min(cst["U_ACC_MAX"], val), dv, dK


def lap_gradient(model, k, L, c, v_cap=20.0, grip=1.0, par=None, margin=None, want_pairs=False):
    """T, grad (N_c,) and the arrays of the forward run.  k (N_s,): curvature of the centre line at the cells, c (N_c,): control points.
    A plan that line_profile makes NaN: T = NaN, grad NaN.  want_pairs: also the two sides of every branch decision, as lists of
    (a, b) pairs per kind of decision (for the vetting of the GPU fixtures): "pass" the min of the two passes, "k" |k| against 1e-12,
    "cap" sqrt(A_lat / K) against v_cap, "edge" the polygon edges and U_ACC_MAX of the longitudinal limit, "y1" its y against 1."""
    k = np.asarray(k, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    N_s, N_c = k.size, c.size
    ds, h = L / N_s, L / N_c
    cst = pn.constants(par)
    nan = dict(T=np.nan, grad=np.full(N_c, np.nan), t=np.full(N_s, np.nan))
    if margin is not None and not ((rn.N_MAX_DEFAULT if par is None else float(par[pn.IDX["N_MAX"]])) - margin > 0):
        return nan
    n, nd = rn.offsets(c, N_s)
    nd = nd / h
    a = 1.0 - n * k
    if not (a >= 0.1).all():
        return nan
    r = np.sqrt(a * a + nd * nd)
    mu = np.arctan(nd / a)
    dl = ds * r
    m = k + (np.roll(mu, -1) - np.roll(mu, 1)) / (2.0 * ds)
    kl = m / r
    A_lat = pn.a_lat(model, cst, grip)
    K = np.maximum(np.abs(kl), 1e-12)
    slat = np.sqrt(A_lat / K)
    vlat = np.minimum(v_cap, slat)
    i0 = int(np.argmin(vlat))
    pairs = dict(k=[(float(abs(x)), 1e-12) for x in kl], cap=[(float(x), v_cap) for x in slat], edge=[], y1=[])
    pairs["pass"] = []
    v = vlat.copy()
    won = np.zeros(N_s, dtype=np.int64)

    def edge_pairs(vp, Kp):
        if model == 1:
            y0 = vp * vp * Kp / A_lat
            pairs["edge"].extend([(y0, 0.5), (y0, pn.POLY_S[2])])
            pairs["y1"].append((y0, 1.0))
            if y0 < 1.0:
                pairs["edge"].append((a_x(1, dict(cst, U_ACC_MAX=np.inf), grip, A_lat, vp, Kp)[0], cst["U_ACC_MAX"]))

    for j in range(1, N_s + 1):
        i = (i0 + j) % N_s; p = (i0 + j - 1) % N_s
        cand = np.sqrt(v[p] * v[p] + 2.0 * a_x(model, cst, grip, A_lat, v[p], K[p])[0] * dl[p])
        pairs["pass"].append((float(v[i]), float(cand))); edge_pairs(v[p], K[p])
        won[i] = WON_FWD if cand < v[i] else 0
        v[i] = min(v[i], cand)
    vf = v.copy()
    for j in range(1, N_s + 1):
        i = (i0 - j) % N_s; nx = (i0 - j + 1) % N_s
        cand = np.sqrt(v[nx] * v[nx] + 2.0 * a_x(model, cst, grip, A_lat, v[nx], K[nx])[0] * dl[i])
        pairs["pass"].append((float(v[i]), float(cand))); edge_pairs(v[nx], K[nx])
        if cand < v[i]:
            won[i] |= WON_BWD
        v[i] = min(v[i], cand)
    t = dl / v
    # ---- the reverse sweep ----
    vbar = -dl / (v * v)
    dlbar = 1.0 / v
    Kbar = np.zeros(N_s)
    i = i0
    for j in range(N_s, 0, -1):                      # the backward pass, last step first: step j set cell (i0 - j) mod N_s
        nx = (i + 1) % N_s
        if won[i] & WON_BWD:
            vn = vf[nx] if j == 1 else v[nx]
            ax, dv, dK = a_x(model, cst, grip, A_lat, vn, K[nx])
            qbar = vbar[i] / (2.0 * v[i])
            vbar[i] = 0.0
            vbar[nx] += qbar * (2.0 * vn + 2.0 * dl[i] * dv)
            Kbar[nx] += qbar * (2.0 * dl[i] * dK)
            dlbar[i] += qbar * (2.0 * ax)
        i = nx
    i = i0
    for j in range(N_s, 0, -1):                      # the forward pass: step j set cell (i0 + j) mod N_s
        p = (i - 1) % N_s
        if won[i] & WON_FWD:
            vp = vlat[i0] if j == 1 else vf[p]
            ax, dv, dK = a_x(model, cst, grip, A_lat, vp, K[p])
            qbar = vbar[i] / (2.0 * vf[i])
            vbar[i] = 0.0
            vbar[p] += qbar * (2.0 * vp + 2.0 * dl[p] * dv)
            Kbar[p] += qbar * (2.0 * dl[p] * dK)
            dlbar[p] += qbar * (2.0 * ax)
        i = p
    capped = slat < v_cap
    Kbar = np.where(capped, Kbar + vbar * (-0.5 * slat / K), Kbar)
    kbar = np.where(np.abs(kl) > 1e-12, np.where(kl < 0.0, -Kbar, Kbar), 0.0)
    mbar = kbar / r
    rbar = -kbar * m / (r * r) + ds * dlbar
    mubar = (np.roll(mbar, 1) - np.roll(mbar, -1)) / (2.0 * ds)
    q = a * a + nd * nd
    abar = rbar * a / r - mubar * nd / q
    ndbar = (rbar * nd / r + mubar * a / q) / h
    nbar = -abar * k
    grad = np.zeros(N_c)
    for i in range(N_s):                             # every grad_j: its cells in ascending order
        jb, u = rn.basis(i, N_s, N_c)
        w, wd = rn.weights(u), rn.dweights(u)
        for kk in range(4):
            grad[(jb - 1 + kk) % N_c] += w[kk] * nbar[i] + wd[kk] * ndbar[i]
    out = dict(T=float(t.sum()), grad=grad, t=t, v=v, vf=vf, won=won, i0=i0, kl=kl, dl=dl, vlat=vlat)
    if want_pairs:
        out["pairs"] = pairs
    return out


def closest_call(pairs):
    """The smallest relative distance between the two sides of a branch decision (a list of pairs; inf for an empty list)."""
    if len(pairs) == 0:
        return np.inf
    p = np.asarray(pairs, dtype=np.float64)
    fin = np.isfinite(p).all(axis=1)
    p = p[fin]
    return float(np.min(np.abs(p[:, 0] - p[:, 1]) / np.maximum(np.abs(p[:, 0]), np.abs(p[:, 1]))))


def iterate(orc, model, k, L, H, c, grad, T, lo, hi, rho=RHO_DEFAULT, v_cap=20.0, grip=1.0, par=None, margin=None):
    """One iteration from c (with its T and grad): per rho the step of the bounds-only QP by the oracle, the clamped candidate, its lap
    and gradient; the least finite T among the solved candidates (first index on ties) replaces the incumbent if strictly smaller.
    Returns c, grad, T, the index taken (-1: stayed) and the candidates' (T, flag, c) lists."""
    N_c = c.size
    cands = []
    for rj in rho:
        d, f, flag, it, lam = orc.qp_solve(H, grad / rj, np.zeros((0, N_c)), lo - c, hi - c, np.zeros(0), np.zeros(0))
        cj = np.minimum(np.maximum(c + d, lo), hi)
        cands.append((lap_gradient(model, k, L, cj, v_cap, grip, par, margin), flag, cj))
    pick, best = -1, T
    if np.isfinite(T):
        for j, (res, flag, cj) in enumerate(cands):
            if flag == 0 and np.isfinite(res["T"]) and res["T"] < best:
                pick, best = j, res["T"]
    if pick >= 0:
        c, grad, T = cands[pick][2], cands[pick][0]["grad"], cands[pick][0]["T"]
    return c, grad, T, pick, cands


def loop(orc, model, k, L, H, c, lo, hi, iters, rho=RHO_DEFAULT, v_cap=20.0, grip=1.0, par=None, margin=None):
    """`iters` iterations from c.  Returns c, lap_hist (iters + 1,), step_hist (iters,)."""
    res = lap_gradient(model, k, L, c, v_cap, grip, par, margin)
    T, grad = res["T"], res["grad"]
    lap, step = [T], []
    for _ in range(iters):
        c, grad, T, pick, _c = iterate(orc, model, k, L, H, c, grad, T, lo, hi, rho, v_cap, grip, par, margin)
        lap.append(T); step.append(pick)
    return c, np.array(lap), np.array(step, dtype=np.int64)
