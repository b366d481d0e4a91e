"""Numpy statement of the minimum-curvature racing line of DESIGN.md 6j (csrc/raceline.h, csrc/raceline.hip), operation for
operation: the B-spline basis of the lateral offset, the second difference of the line's points per cell as a function of the
control points, H = 2 ds G'G and g = 2 ds G'd summed over the cells in ascending order, and the speed profile of 6i on a line
(plan_numpy.profile with the cell's own length and curvature)."""
import ctypes as C

import numpy as np

import plan_numpy as pn

N_MAX_DEFAULT = 0.75
LINE_MAX_NS = 2048
_CACHE = {}


def basis(i, N_s, N_c):
    q = int(i) * int(N_c)
    return q // N_s, float(q % N_s) / float(N_s)


def weights(u):
    m = 1.0 - u
    return np.array([m * m * m / 6.0, (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0, (-3.0 * u * u * u + 3.0 * u * u + 3.0 * u + 1.0) / 6.0,
                     u * u * u / 6.0])


def dweights(u):
    m = 1.0 - u
    return np.array([-3.0 * m * m / 6.0, (9.0 * u * u - 12.0 * u) / 6.0, (-9.0 * u * u + 6.0 * u + 3.0) / 6.0, 3.0 * u * u / 6.0])


def frames(orc, track, N_s):
    """(N_s, 4): centre point and unit left normal of the cells s_i = i ds (curvilinear_to_cartesian.m:16-23)."""
    L = orc.lib()
    L.orc_spline_d.restype = C.c_double
    ds = track.L / N_s
    out = np.zeros((N_s, 4))
    for i in range(N_s):
        s = C.c_double(float(i) * ds)
        dl = C.c_double(track.dl)
        x, y = L.orc_spline_val(track.c.xP, track.M, dl, s), L.orc_spline_val(track.c.yP, track.M, dl, s)
        tx, ty = -L.orc_spline_d(track.c.yP, track.M, dl, s), L.orc_spline_d(track.c.xP, track.M, dl, s)
        nrm = np.sqrt(tx * tx + ty * ty)
        out[i] = (x, y, tx / nrm, ty / nrm)
    return out


def cell(fr, i, N_s, N_c, ds):
    """base, gx (5,), gy (5,), dx, dy of cell i (rl_cell)."""
    cells = ((i - 1) % N_s, i, (i + 1) % N_s)
    gx, gy = np.zeros(5), np.zeros(5)
    j0 = 0
    for m, (ci, coef) in enumerate(zip(cells, (1.0, -2.0, 1.0))):
        j, u = basis(ci, N_s, N_c)
        w = weights(u)
        if m == 0:
            j0 = j
        o = (j - j0) % N_c
        assert o in (0, 1)
        for k in range(4):
            gx[o + k] += coef * fr[ci, 2] * w[k]
            gy[o + k] += coef * fr[ci, 3] * w[k]
    ds2 = ds * ds
    p, c, n = cells
    dx = (fr[n, 0] - 2.0 * fr[c, 0] + fr[p, 0]) / ds2
    dy = (fr[n, 1] - 2.0 * fr[c, 1] + fr[p, 1]) / ds2
    return (j0 - 1) % N_c, gx / ds2, gy / ds2, dx, dy


def qp_from_frames(fr, L, N_c):
    """H (N_c, N_c), g (N_c,) of the line QP from the frames of the cells: every entry a sum over the cells in ascending order."""
    N_s = fr.shape[0]
    ds = L / N_s
    acc = np.zeros((N_c, N_c))
    gacc = np.zeros(N_c)
    for i in range(N_s):
        base, gx, gy, dx, dy = cell(fr, i, N_s, N_c, ds)
        cols = (base + np.arange(5)) % N_c
        acc[np.ix_(cols, cols)] += np.outer(gx, gx) + np.outer(gy, gy)
        gacc[cols] += gx * dx + gy * dy
    return 2.0 * ds * acc, 2.0 * ds * gacc


def second_difference(fr, L, N_c):
    """G (2 N_s, N_c) and d (2 N_s,): the second difference of the line's points over ds^2 is G c + d (x rows, then y rows)."""
    N_s = fr.shape[0]
    ds = L / N_s
    G, d = np.zeros((2 * N_s, N_c)), np.zeros(2 * N_s)
    for i in range(N_s):
        base, gx, gy, dx, dy = cell(fr, i, N_s, N_c, ds)
        cols = (base + np.arange(5)) % N_c
        G[i, cols] += gx; G[N_s + i, cols] += gy
        d[i], d[N_s + i] = dx, dy
    return G, d


def qp(orc, track, N_s, N_c):
    """H, g of (track, N_s, N_c), computed once and left unchanged."""
    key = (track.name, track.L, N_s, N_c)
    if key not in _CACHE:
        H, g = qp_from_frames(frames(orc, track, N_s), track.L, N_c)
        H.setflags(write=False); g.setflags(write=False)
        _CACHE[key] = (H, g)
    return _CACHE[key]


def offsets(c, N_s):
    """n (N_s,), n' (N_s,) of the line with control points c at the cells."""
    c = np.asarray(c, dtype=np.float64)
    N_c = c.size
    n, nd = np.zeros(N_s), np.zeros(N_s)
    for i in range(N_s):
        j, u = basis(i, N_s, N_c)
        w, wd = weights(u), dweights(u)
        a = b = 0.0
        for k in range(4):
            ck = c[(j - 1 + k) % N_c]
            a += w[k] * ck; b += wd[k] * ck
        n[i], nd[i] = a, b
    return n, nd


def line_profile(model, k, L, c, v_cap=20.0, grip=1.0, par=None, margin=None):
    """plan_profile_kernel<.., LINE = true>: k (N_s,) curvature of the centre line at the cells, c (N_c,) control points.  Returns the dict of
    plan_numpy.profile plus n, mu, kl (the line's curvature), dl (the cells' lengths on the line).  margin: None (no width check) or
    the margin of Plan.raceline."""
    k = np.asarray(k, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    N_s, N_c = k.size, c.size
    ds, h = L / N_s, L / N_c
    cst = pn.constants(par)
    nan = dict(table=np.full((N_s, 8), np.nan), t=np.full(N_s, np.nan), ds=ds)
    if margin is not None and not ((N_MAX_DEFAULT if par is None else float(par[pn.IDX["N_MAX"]])) - margin > 0):
        return nan
    n, nd = offsets(c, N_s)
    nd = nd / h
    a = 1.0 - n * k
    if not (a >= 0.1).all():
        return nan
    r = np.sqrt(a * a + nd * nd)
    mu = np.arctan(nd / a)
    dl = ds * r
    kl = (k + (np.roll(mu, -1) - np.roll(mu, 1)) / (2.0 * ds)) / r
    A_lat = pn.a_lat(model, cst, grip)
    K = np.maximum(np.abs(kl), 1e-12)
    vlat = np.minimum(v_cap, np.sqrt(A_lat / K))
    i0 = int(np.argmin(vlat))
    v = vlat.copy()
    for j in range(1, N_s + 1):
        i = (i0 + j) % N_s; p = (i0 + j - 1) % N_s
        v[i] = min(v[i], np.sqrt(v[p] * v[p] + 2.0 * pn.a_x(model, cst, grip, A_lat, v[p], K[p]) * dl[p]))
    for j in range(1, N_s + 1):
        i = (i0 - j) % N_s; nx = (i0 - j + 1) % N_s
        v[i] = min(v[i], np.sqrt(v[nx] * v[nx] + 2.0 * pn.a_x(model, cst, grip, A_lat, v[nx], K[nx]) * dl[i]))
    vn = np.roll(v, -1)
    delta = np.arctan((cst["LR"] + cst["LF"]) * kl)
    t = dl / v
    table = np.zeros((N_s, 8))
    table[:, 0] = n
    table[:, 1] = mu
    table[:, 2] = v
    table[:, 4] = v * kl
    table[:, 5] = delta
    table[:, 6] = (vn * vn - v * v) / (2.0 * dl)
    table[:, 7] = (np.roll(delta, -1) - delta) / t
    return dict(table=table, t=t, ds=ds, v=v, vlat=vlat, K=K, k=k, kl=kl, dl=dl, n=n, mu=mu, i0=i0, A_lat=A_lat, c=cst)


def multipliers(H, g, lb, ub, x, tol=1e-7):
    """Multipliers of a bounds-only QP at x: the gradient on the variables that sit on a bound, zero elsewhere (any stationarity
    residual of a free variable stays visible to the KKT certificate)."""
    lam = H @ x + g
    at = (np.abs(x - lb) <= tol) | (np.abs(ub - x) <= tol)
    return np.where(at, lam, 0.0)
