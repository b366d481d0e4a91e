"""numpy restatement of the corridor-from-cones stage, written from include/fsaempc.h's description, and an
independent brute-force ray cast of the same edge.  Test infrastructure: it shares no code with the product.

The restatement: every cone is projected onto the track spline (nearest of 4M coarse samples, then Newton on the squared distance),
the kept cones are ordered by (s, input index), and per cell the normal line of the spline is cut with the chord between the two
cones that bracket the cell in s.  The ray cast uses neither the projection nor the order: it cuts the normal line with every chord
of the closed polyline in file order and keeps the nearest admissible hit."""
import numpy as np

NCONEINFO = 8
CONES_MAX = 512
CONES_MAX_M = 512


def spline3(P, dl, t):
    """value, first and second derivative of one Bezier spline table P (M, 4) at t (any shape); csrc/cl_frame.h spline3"""
    P = np.asarray(P, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    M = P.shape[0]
    per = dl * M
    with np.errstate(invalid="ignore"):
        r = t - np.floor(t / per) * per
        r = np.where(r < 0, r + per, r)
        r = np.where(r >= per, r - per, r)
        ok = (r >= 0) & (r < per)
        i = np.where(ok, np.floor(np.where(ok, r, 0.0) / dl), 0).astype(np.int64)
    i = np.clip(i, 0, M - 1)
    u = r / dl - i
    p0, p1, p2, p3 = P[i, 0], P[i, 1], P[i, 2], P[i, 3]
    w = 1 - u
    v = p0 * (w * w * w) + 3 * p1 * (w * w) * u + 3 * p2 * w * (u * u) + p3 * (u * u * u)
    d = (-3 * w * w * p0 + 3 * (3 * u * u - 4 * u + 1) * p1 + 3 * (2 * u - 3 * u * u) * p2 + 3 * u * u * p3) / dl
    dd = (6 * w * p0 + 6 * (3 * u - 2) * p1 + 6 * (1 - 3 * u) * p2 + 6 * u * p3) / (dl * dl)
    return v, d, dd


def frame(track, s):
    """(p, T, N): the spline point, the unit tangent and the unit left normal at s (any shape), each (..., 2)"""
    X, Xd, _ = spline3(track.xP, track.dl, s)
    Y, Yd, _ = spline3(track.yP, track.dl, s)
    nrm = np.sqrt(Xd * Xd + Yd * Yd)
    return np.stack([X, Y], -1), np.stack([Xd / nrm, Yd / nrm], -1), np.stack([-Yd / nrm, Xd / nrm], -1)


ABSENT, UNPROJECTED, STRAY, KEPT = 2, 3, 4, 0


def project(track, L, cones, reach):
    """Per cone of (K, 2): (status, s in [0, L), n).  status: KEPT, ABSENT (a non-finite coordinate), UNPROJECTED, STRAY (|n| > reach)."""
    cones = np.asarray(cones, dtype=np.float64).reshape(-1, 2)
    K, M, dl = cones.shape[0], track.M, track.dl
    status = np.full(K, KEPT, dtype=np.int64)
    s_out, n_out = np.full(K, np.nan), np.full(K, np.nan)
    sc = (np.arange(4 * M, dtype=np.float64) + 0.5) * dl / 4
    cx, _, _ = spline3(track.xP, dl, sc)
    cy, _, _ = spline3(track.yP, dl, sc)
    for k in range(K):
        x0, y0 = cones[k]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            status[k] = ABSENT
            continue
        dx, dy = cx - x0, cy - y0
        s = sc[int(np.argmin(dx * dx + dy * dy))]     # (argmin: the first minimum in ascending j)
        done = False
        with np.errstate(all="ignore"):
            for _ in range(30):
                X, Xd, Xdd = spline3(track.xP, dl, s)
                Y, Yd, Ydd = spline3(track.yP, dl, s)
                dist_d = 2 * (X - x0) * Xd + 2 * (Y - y0) * Yd
                dist_dd = 2 * (X - x0) * Xdd + 2 * Xd * Xd + 2 * (Y - y0) * Ydd + 2 * Yd * Yd
                if not dist_dd > 0:
                    break
                delta = dist_d / dist_dd
                if not np.isfinite(delta) or abs(delta) > dl:
                    break
                s = s - delta
                if not np.isfinite(s):
                    break
                if abs(delta) <= 1e-10:
                    done = True
                    break
        if not done:
            status[k] = UNPROJECTED
            continue
        X, Xd, _ = spline3(track.xP, dl, s)
        Y, Yd, _ = spline3(track.yP, dl, s)
        nrm = np.sqrt(Xd * Xd + Yd * Yd)
        n = (x0 - X) * (-Yd / nrm) + (y0 - Y) * (Xd / nrm)
        if not np.isfinite(n):
            status[k] = UNPROJECTED
            continue
        if abs(n) > reach:
            status[k] = STRAY
            continue
        r = s - np.floor(s / L) * L
        if not (r >= 0 and r < L):
            r = 0.0
        s_out[k], n_out[k] = r, n
    return status, s_out, n_out


def edge_table(track, L, cones, N_w, reach):
    """One side: (edge (N_w,), counts {kept, absent, unprojected, stray, off}) of the closed polyline through the kept cones in the
    order of (s, input index)."""
    cones = np.asarray(cones, dtype=np.float64).reshape(-1, 2)
    status, s, n = project(track, L, cones, reach)
    keep = np.flatnonzero(status == KEPT)
    order = keep[np.lexsort((keep, s[keep]))]
    cs, cn, c = s[order], n[order], cones[order]
    K = len(order)
    counts = {"kept": K, "absent": int((status == ABSENT).sum()), "unprojected": int((status == UNPROJECTED).sum()),
              "stray": int((status == STRAY).sum()), "off": 0}
    if K == 0:
        return np.full(N_w, np.nan), counts
    if K == 1:
        return np.full(N_w, cn[0]), counts
    ds = L / N_w
    si = np.arange(N_w, dtype=np.float64) * ds
    p, T, N = frame(track, si)
    j = np.searchsorted(cs, si, side="right") - 1          # the last kept cone with s_j <= s_i
    none = j < 0
    j = np.where(none, K - 1, j)
    j1 = np.where(j + 1 < K, j + 1, 0)
    sj = np.where(none, cs[j] - L, cs[j])
    sj1 = np.where(none, cs[j1], np.where(j + 1 < K, cs[j1], cs[j1] + L))
    cj, d = c[j], c[j1] - c[j]
    dT = d[:, 0] * T[:, 0] + d[:, 1] * T[:, 1]
    with np.errstate(all="ignore"):
        t_geo = ((p[:, 0] - cj[:, 0]) * T[:, 0] + (p[:, 1] - cj[:, 1]) * T[:, 1]) / dT
        t_arc = (si - sj) / (sj1 - sj)
        t = np.where(dT > 0, t_geo, t_arc)
        counts["off"] = int((~((t >= -1e-9) & (t <= 1 + 1e-9))).sum())
        t = np.fmin(np.fmax(t, 0.0), 1.0)
        edge = (cj[:, 0] + t * d[:, 0] - p[:, 0]) * N[:, 0] + (cj[:, 1] + t * d[:, 1] - p[:, 1]) * N[:, 1]
    return edge, counts


def info(n_lo, n_hi, cl, cr):
    """The FSAEMPC_NCONEINFO block of one corridor from its tables and the two sides' counts"""
    out = np.zeros(NCONEINFO)
    out[0], out[1] = cl["kept"], cr["kept"]
    out[2] = cl["absent"] + cr["absent"]
    out[3] = cl["unprojected"] + cr["unprojected"]
    out[4] = cl["stray"] + cr["stray"]
    out[5] = cl["off"] + cr["off"]
    with np.errstate(invalid="ignore"):
        out[6] = int((~(n_lo < n_hi)).sum())
    w = n_hi - n_lo
    out[7] = np.nan if np.isnan(w).any() else w.min()
    return out


def corridor_from_cones(track, L, left, right, N_w, margin=0.0, reach=5.0):
    """(n_lo, n_hi, info) of one corridor"""
    el, cl = edge_table(track, L, left, N_w, reach)
    er, cr = edge_table(track, L, right, N_w, reach)
    n_hi, n_lo = el - margin, er + margin
    return n_lo, n_hi, info(n_lo, n_hi, cl, cr)


def ray_cast(track, L, cones, N_w, side, reach):
    """The independent oracle for one side (side = +1 left, -1 right): per cell the normal line p_i + n N_i is cut with every chord
    c_a -> c_{a+1} of the closed polyline in FILE order; a hit counts with t in [0, 1], n of the side's sign, d . T_i > 0 and
    |n| < reach; the nearest wins.  Returns (edge (N_w,), hits per cell (N_w,))."""
    c = np.asarray(cones, dtype=np.float64).reshape(-1, 2)
    si = np.arange(N_w, dtype=np.float64) * (L / N_w)
    p, T, N = frame(track, si)
    a, d = c, np.roll(c, -1, axis=0) - c
    edge, hits = np.full(N_w, np.nan), np.zeros(N_w, dtype=np.int64)
    for i in range(N_w):
        dT = d @ T[i]
        with np.errstate(all="ignore"):
            t = ((p[i] - a) @ T[i]) / dT
            n = (a + t[:, None] * d - p[i]) @ N[i]
        ok = (dT > 0) & (t >= 0) & (t <= 1) & (side * n > 0) & (np.abs(n) < reach)
        hits[i] = int(ok.sum())
        if hits[i]:
            cand = n[ok]
            edge[i] = cand[int(np.argmin(np.abs(cand)))]
    return edge, hits


def linear_sn_edge(track, L, cones, N_w, reach):
    """The (s, n)-linear resampling the polyline form replaces (for the record of the difference)"""
    status, s, n = project(track, L, cones, reach)
    keep = np.flatnonzero(status == KEPT)
    order = keep[np.lexsort((keep, s[keep]))]
    cs, cn = s[order], n[order]
    si = np.arange(N_w, dtype=np.float64) * (L / N_w)
    return np.interp(si, np.concatenate([[cs[-1] - L], cs, [cs[0] + L]]), np.concatenate([[cn[-1]], cn, [cn[0]]]))
