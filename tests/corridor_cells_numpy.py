"""numpy restatement of the cell-wise corridor rows of the racing line, written from include/fsaempc.h's description:
the row of a cell (first column and the four B-spline weights), the matrix of the rows, the bounds of the rows from the corridor, and
the corridor the tests use.  Test infrastructure: it shares no code with the product; the corridor's lookup is tests/corridor_numpy.py."""
import numpy as np

import corridor_numpy as cn

FREE = 1e10       # the bound of a free control point: the filler of the LTV rows, beyond the solver's inf_bound


def row(i, N_s, N_c):
    """Cell i: q = i N_c / N_s in integers, j = floor(q), u = q - j; returns the first column (j - 1) mod N_c and the weights
    [(1 - u)^3, 3u^3 - 6u^2 + 4, -3u^3 + 3u^2 + 3u + 1, u^3] / 6 of the columns first .. first + 3 (cyclic)."""
    q = int(i) * int(N_c)
    j, u = q // N_s, float(q % N_s) / float(N_s)
    m = 1.0 - u
    w = np.array([m * m * m / 6.0, (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0, (-3.0 * u * u * u + 3.0 * u * u + 3.0 * u + 1.0) / 6.0,
                  u * u * u / 6.0])
    return (j - 1) % N_c, w


def matrix(N_s, N_c):
    """B (N_s, N_c): B[i, (first_i + m) mod N_c] = w_m(u_i), zero elsewhere.  The device's A is the column-major memory of B,
    that is B.T as a C-contiguous (N_c, N_s) array."""
    B = np.zeros((N_s, N_c))
    for i in range(N_s):
        first, w = row(i, N_s, N_c)
        for m in range(4):
            B[i, (first + m) % N_c] = w[m]
    return B


def apply(c, N_s):
    """B c with every row summed over its four columns in the order m = 0 .. 3 (the order of the line's own evaluation)."""
    c = np.asarray(c, dtype=np.float64)
    n = np.zeros(N_s)
    for i in range(N_s):
        first, w = row(i, N_s, c.size)
        a = 0.0
        for m in range(4):
            a += w[m] * c[(first + m) % c.size]
        n[i] = a
    return n


def row_bounds(n_lo, n_hi, ds, L, N_s, margin):
    """(lbA, ubA) of (N_s,): n_lo(s_i) + margin and n_hi(s_i) - margin at s_i = i L / N_s; NaN for both where the lookup is NaN or
    lbA < ubA does not hold."""
    s = np.arange(N_s, dtype=np.float64) * L / N_s
    lo, hi = cn.limits(n_lo, n_hi, ds, s)
    l, h = lo + margin, hi - margin
    with np.errstate(invalid="ignore"):
        bad = ~(l < h)
    return np.where(bad, np.nan, l), np.where(bad, np.nan, h)


def kappa_corridor(kappa, wide=1.5, narrow=0.75, limit=0.02):
    """The corridor of DESIGN.md 6l over the cells whose curvature is given: +-wide where |kappa| < limit, +-narrow elsewhere."""
    w = np.where(np.abs(np.asarray(kappa)) < limit, wide, narrow)
    return -w, w


def objective(H, g, c):
    return 0.5 * float(c @ H @ c) + float(g @ c)
