"""Numpy statement of the NLP of the batched SQP (DESIGN.md "Nonlinear MPC: batched SQP"), built on the oracle's model f
(oracle.f_model): rollout under Euler / midpoint RK2 / classical RK4, the constraint rows of the LTV build in nonlinear form
(mpc/ltv/*_state_constraints.m, kinematic_tyre_linearise_constraints.m, dynamic_slip_ / dynamic_tyre_linearise_constraints.m), the
objective of generate_qp.m with the weights of ltvmpc_*.m:32-35, slack reset and l1 merit.  Per instance: x0 (nx,), u (N, 2),
x_ref (N, nx); states X (N, nx) = x_1 .. x_N."""
import numpy as np

LR, LF = 0.6183, 0.8672
QW = np.array([5.0, 250.0, 2000.0])
EULER, RK2, RK4 = 0, 1, 2


def default_integrator(model):
    return RK2 if model == 0 else RK4


def psi(orc, model, track, x, u, dt, integ):
    f = lambda xx: orc.f_model(model, track, xx, u)
    k1 = f(x)
    if integ == EULER:
        return x + dt * k1
    if integ == RK2:
        return x + dt * f(x + k1 * dt / 2)
    k2 = f(x + k1 * dt / 2)
    k3 = f(x + k2 * dt / 2)
    k4 = f(x + k3 * dt)
    return x + dt * ((k1 + 2 * k2 + 2 * k3 + k4) / 6)


def rollout(orc, model, track, x0, u, dt, integ):
    x = np.asarray(x0, dtype=np.float64)
    X = []
    for k in range(u.shape[0]):
        x = psi(orc, model, track, x, u[k], dt, integ)
        X.append(x)
    return np.array(X)


def _ellipse():
    j = np.arange(12)
    th0 = 2 * np.pi * j / 12
    th1 = np.where(j + 1 == 12, 2 * np.pi, 2 * np.pi * (j + 1) / 12)
    ac0, al0 = 9.163 * np.sin(th0), 10.0 * np.cos(th0)
    return ac0, al0, 9.163 * np.sin(th1) - ac0, 10.0 * np.cos(th1) - al0


def _slip(X):
    xh = X[:, 3] + 5 * np.exp(-X[:, 3] / 5)
    ar = -np.arctan((X[:, 4] - LR * X[:, 5]) / xh)
    af = X[:, 6] - np.arctan((X[:, 4] + LF * X[:, 5]) / xh)
    return ar, af


def _fcr(ar):
    PB, PC, PD, PE = 12.56, 1.38, 1.60, -0.58
    Fzr = 280 * 9.81 * LF / (LR + LF)
    return Fzr * PD * np.sin(PC * np.arctan(PB * ar - PE * (PB * ar - np.arctan(PB * ar))))


def rows(model, X, U):
    """The nC constraint rows of the build in nonlinear form, without their slack terms, row order of the QP's A."""
    N = X.shape[0]
    v, d, n = X[:, 3], X[:, -1], X[:, 1]
    out = [v, d, n, n]
    if model == 0:
        g = X[:, 3] ** 2 * X[:, 4] / (LR + LF)
        out += [g, g]
    else:
        ar, af = _slip(X)
        sl = np.stack([ar, af], 1).ravel()
        out += [sl, sl]
        ac0, al0, dac, dal = _ellipse()
        c = (U[:, 0:1] - al0[None]) * dac[None] - (_fcr(ar)[:, None] / 280 - ac0[None]) * dal[None]
        out.append(c.ravel())
    r = np.concatenate(out)
    assert r.size == (6 if model == 0 else 20) * N
    return r


def slack_min(model, X, U):
    s0 = max(0.0, np.max(np.abs(X[:, 1]) - 0.75))
    if model == 0:
        return np.array([max(s0, np.max(np.abs(X[:, 3] ** 2 * X[:, 4] / (LR + LF)) - 5))])
    ar, af = _slip(X)
    ac0, al0, dac, dal = _ellipse()
    c = (U[:, 0:1] - al0[None]) * dac[None] - (_fcr(ar)[:, None] / 280 - ac0[None]) * dal[None]
    return np.maximum(np.array([s0, np.max(np.abs(ar)) - 0.1, np.max(np.abs(af)) - 0.1, np.max(c)]), 0.0)


def r_soft(model):
    return np.array([1e8]) if model == 0 else np.array([1e8, 1e6, 1e6, 1e4])


def hard_violation(X):
    """(l1 sum, max) of the hard rows v_k >= 0, |delta_k| <= 0.4."""
    h = np.concatenate([np.maximum(0, -X[:, 3]), np.maximum(0, np.abs(X[:, -1]) - 0.4)])
    return float(h.sum()), float(h.max())


def weights(N, nx):
    W = np.zeros((N, nx))
    W[:, :3] = QW
    W[-1] *= 10
    return W


def objective(model, X, U, s, x_ref):
    W = weights(*X.shape)
    return float(np.sum(W * (X - x_ref) ** 2) + 10 * np.sum(U ** 2) + np.dot(r_soft(model), s))


def merit(model, X, U, s, x_ref, rho):
    return objective(model, X, U, s, x_ref) + rho * hard_violation(X)[0]
