"""numpy restatement of the s-varying track corridors, written from include/fsaempc.h's description: the lookup, the
track-row bounds of the MPC QP, the control-point bounds of the racing line and the lap report's track violation.  Test
infrastructure: it shares no code with the product."""
import numpy as np


def _cell(Nw, ds, s):
    """q = s / ds wrapped into [0, N_w): (finite?, i = floor(q), u = q - i)"""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = s / ds
        ok = np.isfinite(q)
        q = np.where(ok, q, 0.0)
        q = q - Nw * np.floor(q / Nw)
        q = np.where((q >= 0.0) & (q < Nw), q, 0.0)      # (the wrap's own rounding: the point N_w is the point 0)
    i = np.floor(q).astype(np.int64)
    return ok, i, q - i


def lookup(table, ds, s):
    """Periodic, piecewise-linear table (N_w,) with cell i at i ds, at s (any shape): t[i] + u (t[i + 1 mod N_w] - t[i]), in this form so
    that a constant table returns the constant exactly.  NaN where s is not finite."""
    table = np.asarray(table, dtype=np.float64)
    Nw = table.shape[0]
    ok, i, u = _cell(Nw, ds, s)
    a, b = table[i], table[(i + 1) % Nw]
    return np.where(ok, a + u * (b - a), np.nan)


def limits(n_lo, n_hi, ds, s):
    """(lo, hi) at s; NaN for both where s is not finite or one of the two cells read has not n_lo < n_hi."""
    n_lo, n_hi = np.asarray(n_lo, dtype=np.float64), np.asarray(n_hi, dtype=np.float64)
    Nw = n_lo.shape[0]
    ok, i, u = _cell(Nw, ds, s)
    valid = n_lo < n_hi
    good = ok & valid[i] & valid[(i + 1) % Nw]
    return np.where(good, lookup(n_lo, ds, s), np.nan), np.where(good, lookup(n_hi, ds, s), np.nan)


def row_bounds(n_lo, n_hi, ds, s_lin, pred_n):
    """The 2N track-row bounds of one instance: lbA[2N + k] = n_lo(s_k) - pred_n,k and ubA[3N + k] = n_hi(s_k) - pred_n,k."""
    lo, hi = limits(n_lo, n_hi, ds, s_lin)
    return lo - np.asarray(pred_n), hi - np.asarray(pred_n)


def touching_cells(j, N_s, N_c):
    """Cells of the plan whose basis touches control point j: floor(i N_c / N_s) in {j - 2, j - 1, j, j + 1}, cyclic."""
    first = (np.arange(N_s) * N_c) // N_s
    want = {(j + d) % N_c for d in (-2, -1, 0, 1)}
    return np.array([i for i in range(N_s) if int(first[i]) in want], dtype=np.int64)


def control_point_bounds(n_lo, n_hi, ds, L, N_s, N_c, margin):
    """(lb, ub) of (N_c,): lb_j = max (n_lo(s_i) + margin), ub_j = min (n_hi(s_i) - margin) over the touching cells, s_i = i L / N_s.
    A NaN limit in any touching cell makes both NaN."""
    s = np.arange(N_s, dtype=np.float64) * L / N_s
    lo, hi = limits(n_lo, n_hi, ds, s)
    lb, ub = np.zeros(N_c), np.zeros(N_c)
    for j in range(N_c):
        c = touching_cells(j, N_s, N_c)
        l, h = lo[c] + margin, hi[c] - margin
        if np.isnan(l).any() or np.isnan(h).any():
            lb[j] = ub[j] = np.nan
        else:
            lb[j], ub[j] = l.max(), h.min()
    return lb, ub


def violation(n_lo, n_hi, ds, s, n):
    """v = max(n - n_hi(s), n_lo(s) - n) where that is > 0, else 0 (NaN limits: 0)."""
    lo, hi = limits(n_lo, n_hi, ds, s)
    with np.errstate(invalid="ignore"):
        v = np.fmax(n - hi, lo - n)
        return np.where(v > 0.0, v, 0.0)
