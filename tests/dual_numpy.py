"""Dtype-generic dual-number restatement of the exact NLP build (csrc/ltv_build_kernel.h with EXACT = true, csrc/nlp_model.h): a
plain-Python forward-mode dual number (value, derivative) over numpy scalars of a chosen dtype, np.float64 or np.longdouble, and on
it kappa(s) of the track's spline table (d tau / ds = 1 / dl inside a segment), the two curvilinear models with a 32-double
parameter block (index names of tests/param_numpy.py), psi_step for Euler / midpoint RK2 / classical RK4, the exact linearisation
(one pass per column of [x; u]) and the whole QP of steps 2-5 of the kernel assembled in that dtype.  The constraint rows are
param_numpy.rows evaluated on object arrays of dual numbers (numpy's ufuncs call the element's method of the same name), so the
row Jacobians are derivatives of the very formulas the other tests use, not hand Jacobians.  Nothing here imports the library under
test or the oracle: run at np.longdouble this file is the reference of tests/test_exact_build_gpu.py, and the gap between its
float64 and its long-double run (e64) is the error a correct double implementation makes."""
import json

import numpy as np

import param_numpy as pn

EULER, RK2, RK4 = 0, 1, 2
IDX = pn.IDX


def default_block(model):
    """The constants compiled into the kernels (csrc/mpc_params.h FixedPar; fsaempc_ltv_default_params)."""
    P = np.zeros(32)
    for name, v in dict(M=280, IZ=200, LF=0.8672, LR=0.6183, GRAV=9.81, PB=12.56, PC=1.38, PD=1.60, PE=-0.58, Q_S=5, Q_N=250, Q_MU=2000,
                        Q_TERMINAL=10, R_ACC=10, R_STEER=10, R_SOFT0=1e8, U_ACC_MAX=10, U_STEER_MAX=0.4, DELTA_MAX=0.4, N_MAX=0.75,
                        V_MIN=0, ALAT_MAX=5, SLIP_MAX=0.1, ELL_LONG=10.0, ELL_LAT=9.163, PID_KP_V=16000, PID_MAX_F=2800, PID_KP_D=80,
                        PID_MAX_DRATE=0.8).items():
        P[IDX[name]] = v
    if model == 1:
        P[IDX["R_SOFT1"]], P[IDX["R_SOFT2"]], P[IDX["R_SOFT3"]] = 1e6, 1e6, 1e4
    return P


class Dual:
    """(v, d): a value and its derivative along one seeded direction; v and d are numpy scalars of one dtype."""
    __slots__ = ("v", "d")
    __array_ufunc__ = None      # numpy scalars and arrays hand binary operations with a Dual over to the methods below

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + o, self.d)
    __radd__ = __add__

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - o, self.d)

    def __rsub__(self, o):
        return Dual(o - self.v, -self.d)

    def __mul__(self, o):
        return Dual(self.v * o.v, self.d * o.v + self.v * o.d) if isinstance(o, Dual) else Dual(self.v * o, self.d * o)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):
            q = self.v / o.v
            return Dual(q, (self.d - q * o.d) / o.v)
        return Dual(self.v / o, self.d / o)

    def __rtruediv__(self, o):
        q = o / self.v
        return Dual(q, -q * self.d / self.v)

    def __pow__(self, p):       # a constant exponent
        return Dual(self.v ** p, p * self.v ** (p - 1) * self.d)

    # the names numpy's ufuncs look up on the elements of an object array
    def sin(self):
        return Dual(np.sin(self.v), np.cos(self.v) * self.d)

    def cos(self):
        return Dual(np.cos(self.v), -np.sin(self.v) * self.d)

    def tan(self):
        t = np.tan(self.v)
        return Dual(t, (1 + t * t) * self.d)

    def arctan(self):
        return Dual(np.arctan(self.v), self.d / (1 + self.v * self.v))

    def exp(self):
        e = np.exp(self.v)
        return Dual(e, e * self.d)


def _fn(name):
    npf = getattr(np, name)
    return lambda a: getattr(a, name)() if isinstance(a, Dual) else npf(a)


sin, cos, tan, atan, exp = (_fn(n) for n in ("sin", "cos", "tan", "arctan", "exp"))


def val(a):
    return a.v if isinstance(a, Dual) else a


class Table:
    """The spline table of a track JSON: xP, yP (M x 4 control values per segment), dl (arc length of a segment)."""

    def __init__(self, xP, yP, dl):
        self.xP, self.yP, self.dl = np.asarray(xP, dtype=np.float64), np.asarray(yP, dtype=np.float64), float(dl)
        self.M = self.xP.shape[0]
        self.L = self.dl * self.M

    @staticmethod
    def load(path):
        with open(path) as f:
            d = json.load(f)
        assert len(d["xP"]) == d["M"]
        return Table(d["xP"], d["yP"], d["dl"])


def seg_lookup(tab, t):
    """Segment index and local parameter tau of arc length t (a scalar of the working dtype), MATLAB's mod() for the wrap."""
    T = type(t)
    dl, per = T(tab.dl), T(tab.dl) * tab.M
    r = t - np.floor(t / per) * per
    if r < 0:
        r = r + per
    if r >= per:
        r = r - per
    i = min(max(int(np.floor(r / dl)), 0), tab.M - 1)
    return i, r / dl - i


def kappa(tab, s):
    """Curvature of the centre line at arc length s (scalar or Dual)."""
    i, tau = seg_lookup(tab, val(s))
    dl = type(tau)(tab.dl)
    u = Dual(tau, s.d / dl) if isinstance(s, Dual) else tau
    x0, x1, x2, x3 = tab.xP[i]
    y0, y1, y2, y3 = tab.yP[i]
    b0, b1, b2, b3 = -3 * (1 - u) * (1 - u), 3 * (3 * u * u - 4 * u + 1), 3 * (2 * u - 3 * u * u), 3 * u * u
    c0, c1, c2, c3 = 6 * (1 - u), 6 * (3 * u - 2), 6 * (1 - 3 * u), 6 * u
    Xd, Yd = (b0 * x0 + b1 * x1 + b2 * x2 + b3 * x3) / dl, (b0 * y0 + b1 * y1 + b2 * y2 + b3 * y3) / dl
    Xdd, Ydd = (c0 * x0 + c1 * x1 + c2 * x2 + c3 * x3) / (dl * dl), (c0 * y0 + c1 * y1 + c2 * y2 + c3 * y3) / (dl * dl)
    return (Xd * Ydd - Xdd * Yd) / (Xd * Xd + Yd * Yd) ** 1.5


def _par(P, T, *names):
    return [T(P[IDX[n]]) for n in names]


def f_kin(P, tab, x, u):
    T = type(val(x[3]))
    lf, lr = _par(P, T, "LF", "LR")
    k = kappa(tab, x[0])
    beta = atan(lr / (lr + lf) * tan(x[4]))
    den = 1.0 / (1.0 - x[1] * k)
    sd = x[3] * cos(x[2] + beta) * den
    return [sd, x[3] * sin(x[2] + beta), x[3] * sin(beta) / lr - sd * k, u[0], u[1]]


def _pacejka(P, T, Fz, a):
    B, C, D, E = _par(P, T, "PB", "PC", "PD", "PE")
    return Fz * D * sin(C * atan(B * a - E * (B * a - atan(B * a))))


def f_dyn(P, tab, x, u):
    T = type(val(x[3]))
    m, iz, lf, lr, grav = _par(P, T, "M", "IZ", "LF", "LR", "GRAV")
    n, mu, xd, yd, thd, delta = x[1], x[2], x[3], x[4], x[5], x[6]
    Fx = u[0] * m
    xh = xd + 5 * exp(-xd / 5)
    k = kappa(tab, x[0])
    den = 1.0 / (1.0 - n * k)
    af = delta - atan((yd + lf * thd) / xh)
    ar = -atan((yd - lr * thd) / xh)
    Fcf, Fcr = _pacejka(P, T, m * grav * lr / (lr + lf), af), _pacejka(P, T, m * grav * lf / (lr + lf), ar)
    sd = (xd * cos(mu) - yd * sin(mu)) * den
    return [sd, xd * sin(mu) + yd * cos(mu), thd - sd * k,
            (Fx - Fcf * sin(delta) + m * yd * thd) / m,
            (Fcr + Fcf * cos(delta) - m * xd * thd) / m,
            (lf * Fcf * cos(delta) - lr * Fcr) / iz, u[1]]


def f_model(P, tab, model, x, u):
    return f_kin(P, tab, x, u) if model == 0 else f_dyn(P, tab, x, u)


def psi_step(P, tab, model, x, u, dt, integ):
    """One step x+ = Psi(x, u) of the NLP's rollout; x, u: lists of scalars or Duals."""
    f = lambda xx: f_model(P, tab, model, xx, u)
    nx = len(x)
    k1 = f(x)
    if integ == EULER:
        return [x[j] + dt * k1[j] for j in range(nx)]
    k2 = f([x[j] + k1[j] * dt / 2 for j in range(nx)])
    if integ == RK2:
        return [x[j] + dt * k2[j] for j in range(nx)]
    k3 = f([x[j] + k2[j] * dt / 2 for j in range(nx)])
    k4 = f([x[j] + k3[j] * dt for j in range(nx)])
    return [x[j] + dt * ((k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]) / 6) for j in range(nx)]


def _vec(a, T):
    return [T(v) for v in np.asarray(a).ravel()]


def rollout(P, tab, model, x0, u, dt, integ, dtype=np.float64):
    """x_1 .. x_N (N, nx) in dtype."""
    T = dtype
    x, X, dt = _vec(x0, T), [], T(dt)
    for k in range(np.shape(u)[0]):
        x = psi_step(P, tab, model, x, _vec(u[k], T), dt, integ)
        X.append(x)
    return np.array(X, dtype=T)


def linearise_exact(P, tab, model, x, u, dt, integ, dtype=np.float64):
    """(x+, Ad, Bd) of one step at (x, u): one dual pass of psi_step per column of [x; u]."""
    T = dtype
    xs, us, dt = _vec(x, T), _vec(u, T), T(dt)
    nx = len(xs)
    J = np.zeros((nx, nx + 2), dtype=T)
    for c in range(nx + 2):
        xd = [Dual(xs[j], T(1.0 if j == c else 0.0)) for j in range(nx)]
        ud = [Dual(us[j], T(1.0 if nx + j == c else 0.0)) for j in range(2)]
        xn = psi_step(P, tab, model, xd, ud, dt, integ)
        J[:, c] = [e.d for e in xn]
    return np.array([e.v for e in xn], dtype=T), J[:, :nx], J[:, nx:]


def row_step(model, N):
    """The step each constraint row belongs to (row order of param_numpy.rows)."""
    k = np.arange(N)
    if model == 0:
        return np.tile(k, 6)
    return np.concatenate([np.tile(k, 4), np.tile(np.repeat(k, 2), 2), np.repeat(k, 12)])


def rows_linearised(P, model, X, U, dtype=np.float64):
    """Values c (nC,), state Jacobians Cx (nC, nx) and input Jacobians Cu (nC, 2) of the rows at the states X (N, nx) they
    constrain and the inputs U (N, 2) of their steps: param_numpy.rows on object arrays of Duals, one pass per column."""
    T = dtype
    X, U = np.asarray(X, dtype=T), np.asarray(U, dtype=T)
    N, nx = X.shape
    Z = np.concatenate([X, U], axis=1)
    cols = []
    for c in range(nx + 2):
        D = np.empty(Z.shape, dtype=object)
        for k in range(N):
            for j in range(nx + 2):
                D[k, j] = Dual(Z[k, j], T(1.0 if j == c else 0.0))
        r = pn.rows(P, model, D[:, :nx], D[:, nx:])
        cols.append(np.array([e.d for e in r], dtype=T))
    J = np.stack(cols, axis=1)
    return np.array([e.v for e in r], dtype=T), J[:, :nx], J[:, nx:]


def slack_columns(model, N):
    """The slack block of A (nC, ns): +1 / -1 where a soft row carries its slack (the kinematic rows share one)."""
    k = np.arange(N)
    if model == 0:
        S = np.zeros((6 * N, 1))
        S[2 * N + k, 0], S[3 * N + k, 0], S[4 * N + k, 0], S[5 * N + k, 0] = 1, -1, 1, -1
        return S
    S = np.zeros((20 * N, 4))
    S[2 * N + k, 0], S[3 * N + k, 0] = 1, -1
    for q in range(2):
        S[4 * N + 2 * k + q, 1 + q], S[6 * N + 2 * k + q, 1 + q] = 1, -1
    S[8 * N:, 3] = -1
    return S


def exact_qp(tab, model, x0, u, x_ref, dt, integ, P=None, dtype=np.longdouble):
    """The exact QP of the NLP at u for one instance, every tensor in dtype and in the layout of SqpBatch.build_qp's per-instance
    slices: H (nV, nV), g, A (nV, nC), lb, ub, lbA, ubA, pred (N nx), Bt (nV, N nx), const; and Ad (N, nx, nx), Bd (N, nx, 2)."""
    T = dtype
    P = default_block(model) if P is None else np.asarray(P, dtype=np.float64)
    u, x_ref = np.asarray(u, dtype=np.float64), np.asarray(x_ref, dtype=np.float64)
    N, nx, ns = u.shape[0], len(x0), (1 if model == 0 else 4)
    R, nU, nV = nx * N, 2 * N, 2 * N + ns
    # the rollout, and the linearisation of step k at (x_{k-1}, u_k)
    Xs = np.zeros((N + 1, nx), dtype=T)
    Xs[0] = _vec(x0, T)
    Ad, Bd, dd = np.zeros((N, nx, nx), dtype=T), np.zeros((N, nx, 2), dtype=T), np.zeros((N, nx), dtype=T)
    uT = u.astype(T)
    for k in range(N):
        Xs[k + 1], Ad[k], Bd[k] = linearise_exact(P, tab, model, Xs[k], u[k], dt, integ, T)
        dd[k] = Xs[k + 1] - Ad[k] @ Xs[k] - Bd[k] @ uT[k]
    X = Xs[1:]
    # Phi(i,i) = Bd_i, Phi(j,i) = Ad_j Phi(j-1,i); aff_k = Ad_k aff_{k-1} + dd_k, aff_0 = x0
    Phi = np.zeros((N, nx, N, 2), dtype=T)
    for i in range(N):
        Phi[i, :, i, :] = Bd[i]
        for j in range(i + 1, N):
            Phi[j, :, i, :] = Ad[j] @ Phi[j - 1, :, i, :]
    Phi = Phi.reshape(R, nU)
    aff, cur = np.zeros((N, nx), dtype=T), Xs[0]
    for k in range(N):
        cur = Ad[k] @ cur + dd[k]
        aff[k] = cur
    # the rows, linearised at the rollout state they constrain: c + Cx (x - x_k) + Cu (u - u_k) with x = aff_k + Phi_k u
    c, Cx, Cu = rows_linearised(P, model, X, u, T)
    rs = row_step(model, N)
    nC = c.size
    Au = np.einsum("rj,rjc->rc", Cx, Phi.reshape(N, nx, nU)[rs])
    for j in range(2):
        Au[np.arange(nC), 2 * rs + j] += Cu[:, j]
    cst = c + np.einsum("rj,rj->r", Cx, (aff - X)[rs]) - np.einsum("rj,rj->r", Cu, uT[rs])
    lo, hi = pn.bounds(P, model, N)
    shift = lambda b: np.where(np.abs(b) == 1e10, b.astype(T), b.astype(T) - cst)    # (the reference's +-1e10 fillers stay as they are)
    A = np.concatenate([Au, slack_columns(model, N).astype(T)], axis=1)
    # the cost
    W = pn.weights(P, N, nx).astype(T).ravel()
    off = aff.ravel() - x_ref.astype(T).ravel()
    H = np.zeros((nV, nV), dtype=T)
    H[:nU, :nU] = 2 * (Phi.T @ (W[:, None] * Phi) + np.diag(pn.r_diag(P, N).astype(T)))
    g = np.concatenate([2 * (Phi.T @ (W * off)), pn.r_soft(P, model).astype(T)])
    lim = np.tile(_par(P, T, "U_ACC_MAX", "U_STEER_MAX"), N)
    Bt = np.zeros((nV, R), dtype=T)
    Bt[:nU] = Phi.T
    return dict(H=H, g=g, A=np.ascontiguousarray(A.T), lb=np.concatenate([-lim, np.zeros(ns, dtype=T)]),
                ub=np.concatenate([lim, np.full(ns, np.inf, dtype=T)]), lbA=shift(lo), ubA=shift(hi),
                pred=X.ravel().copy(), Bt=Bt, const=np.sum(W * off * off), Ad=Ad, Bd=Bd)


QP_KEYS = ("pred", "Bt", "A", "lbA", "ubA", "lb", "ub", "H", "g", "const")


def gap(a, b):
    """Entry-wise max |a - b| over the max-norm of b (an all-zero b: the absolute gap); the infinite and +-1e10 filler pattern must
    be identical."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.longdouble)), np.atleast_1d(np.asarray(b, dtype=np.longdouble))
    fill = ~np.isfinite(b) | (np.abs(b) == 1e10)
    assert np.array_equal(~np.isfinite(a) | (np.abs(a) == 1e10), fill), "filler pattern differs"
    assert np.array_equal(a[fill], b[fill]), "filler entries differ"
    if fill.all():
        return 0.0
    scale = np.max(np.abs(b[~fill]))
    return float(np.max(np.abs(a[~fill] - b[~fill])) / (scale if scale > 0 else 1.0))
