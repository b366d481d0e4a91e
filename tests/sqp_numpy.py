"""Numpy restatement of the SQP's line search (csrc/sqp.hip; DESIGN.md 6e "Sweep"), in fp64 on top of tests/nlp_numpy.py: evaluate()
is what the kernels' nlp_eval does at one trial point, sweep() is one call of sqp_linesearch_kernel for one instance -- penalty update,
Armijo test of every trial, winner, status, step_norm and merit -- and it returns every trial's signed margin and the set of outcomes a
correct kernel may give when a decision lies within the suite's objective tolerance.  fd_build() / cpu_loop() imitate the whole loop on
the CPU (central-difference build of the exact QP, the oracle's QP solve): test infrastructure for vetting the case table, and no
reference for the device's QP."""
from collections import namedtuple

import numpy as np

import nlp_numpy as nn

U_MAX = np.array([10.0, 0.4])     # input boxes (ltvmpc_*.m:28-29)
RUNNING = 3                       # the kernels' code of an instance still running; never returned (the last sweep makes it 1)
TAU = 1e-8                        # a decision within TAU (1 + |phi0|) may fall either way: five times the two-sided 1e-9 the suite
                                  # allows between the device objective and numpy's (test_sqp_converges_to_kkt_points)

Problem = namedtuple("Problem", "orc model track x0 x_ref dt integ")          # one instance: x0 (nx,), x_ref (N, nx)
Point = namedtuple("Point", "J viol vmax s u X")                              # evaluate()'s result: u (N, 2), X (N, nx), s (ns,)
Opts = namedtuple("Opts", "trials armijo tol_step tol_feas sweep max_sweeps")
Qp = namedtuple("Qp", "z fval qconst flag iter lam")                          # one QP result: z (nV,), lam (nV + nC,)


def evaluate(P, u_c, z_u, alpha, s_trial):
    """The point u = clip(u_c + alpha (z_u - u_c)) into the input boxes, X = its rollout, s = max(s_trial, s_min(X, u), 0): objective J,
    l1 sum and max of the hard violation, s, u, X."""
    u_c, z_u = np.asarray(u_c, dtype=np.float64).reshape(-1, 2), np.asarray(z_u, dtype=np.float64).reshape(-1, 2)
    u = np.clip(u_c + alpha * (z_u - u_c), -U_MAX, U_MAX)
    X = nn.rollout(P.orc, P.model, P.track, P.x0, u, P.dt, P.integ)
    s = np.maximum(np.maximum(np.asarray(s_trial, dtype=np.float64), nn.slack_min(P.model, X, u)), 0.0)
    v1, vm = nn.hard_violation(X)
    return Point(nn.objective(P.model, X, u, s, P.x_ref), v1, vm, s, u, X)


def admissible(margins, tau):
    """The outcomes (winner l, or None for "no trial accepted") a correct line search may give when every Armijo decision with
    |margin| <= tau may fall either way: l is admissible iff m_l >= -tau and every l' < l has m_l' <= tau; None iff every m_l <= tau.
    A NaN margin is a rejected trial, whatever tau."""
    out = []
    for l, m in enumerate(margins):
        if m >= -tau:                       # (False for NaN)
            out.append(l)
        if m > tau:                         # accepted beyond doubt: nothing after it can win
            return out
    return out + [None]


def sweep(state, qp, opts, P):
    """One line search.  state = (u, s, rho, J, viol) of the instance before the sweep (J, viol: objective and l1 hard violation of
    (u, s)), qp = Qp of the exact QP at u, opts = Opts.  Returns a dict: rho (updated), phi0, pred, step_norm, margins (trials,),
    tau, winner (lowest accepted l or None), admissible (list), and outcomes {l or None: dict(u, s, X, J, viol, vmax, status, sweeps,
    merit)} for every admissible outcome and the winner."""
    u, s, rho, J, viol = state
    u, s = np.asarray(u, dtype=np.float64).reshape(-1, 2), np.asarray(s, dtype=np.float64)
    N, ns = u.shape[0], s.size
    nV = 2 * N + ns
    z_u, z_s = qp.z[:2 * N].reshape(N, 2), qp.z[2 * N:nV]
    dn = float(np.max(np.abs(z_u - u)))
    un = float(np.max(np.abs(u)))
    lm = float(np.max(np.abs(qp.lam[nV:nV + 2 * N])))          # rows 0 .. 2N-1 of the QP: v_k >= 0, |delta_k| <= 0.4
    rho = max(rho, 1.1 * lm + 1e-6)
    phi0 = J + rho * viol
    pred = max(J - (qp.fval + qp.qconst) + rho * viol, 0.0)
    here = evaluate(P, u, u, 0.0, s)                           # the point the instance keeps when no trial wins
    trial, margins = [], []
    if qp.flag == 0:
        for l in range(opts.trials):
            a = 2.0 ** -l
            e = evaluate(P, u, z_u, a, s + a * (z_s - s))
            trial.append(e)
            margins.append(phi0 - opts.armijo * a * pred - (e.J + rho * e.viol))
    margins = np.array(margins, dtype=np.float64)
    tau = TAU * (1.0 + abs(phi0))
    acc = [l for l, m in enumerate(margins) if m >= 0]          # (False for NaN)
    winner = acc[0] if acc else None
    small = dn <= opts.tol_step * (1.0 + un)

    def outcome(l):
        e = here if l is None else trial[l]
        Jn, vn = (J, viol) if l is None else (e.J, e.viol)      # (the kernel keeps its stored J / viol when nothing is accepted)
        if qp.flag != 0:
            status = -2 if qp.flag == -2 else -1
        else:
            done = small and e.vmax <= opts.tol_feas
            status = 0 if done else (RUNNING if l is not None else 2)
        if status == RUNNING and opts.sweep + 1 >= opts.max_sweeps:
            status = 1
        return dict(u=e.u, s=e.s if l is not None else s, X=e.X, J=Jn, viol=vn, vmax=e.vmax, status=status, sweeps=opts.sweep + 1,
                    merit=Jn + rho * vn)

    adm = admissible(margins, tau) if qp.flag == 0 else [None]
    return dict(rho=rho, phi0=phi0, pred=pred, step_norm=dn, margins=margins, tau=tau, winner=winner, admissible=adm,
                outcomes={l: outcome(l) for l in set(adm) | {winner}})


# ---- the whole loop on the CPU: vets tests/sqp_cases.py without a GPU ----

def _slack_cols(model, N):
    """(nC, ns) slack part of A: +1 on the rows bounded below, -1 on those bounded above (oracle/ltv_oracle_build.c, *_state_constraints.m)."""
    ns, nC = (1, 6 * N) if model == 0 else (4, 20 * N)
    S = np.zeros((nC, ns))
    S[2 * N:3 * N, 0], S[3 * N:4 * N, 0] = 1.0, -1.0
    if model == 0:
        S[4 * N:5 * N, 0], S[5 * N:6 * N, 0] = 1.0, -1.0
    else:
        for q in (0, 1):
            S[4 * N + q:6 * N:2, 1 + q], S[6 * N + q:8 * N:2, 1 + q] = 1.0, -1.0
        S[8 * N:, 3] = -1.0
    return S


def row_bounds(model, N):
    inf = np.inf
    rep = lambda v, n: np.full(n, v)
    lo = [rep(0, N), rep(-0.4, N), rep(-0.75, N), rep(-inf, N)]
    hi = [rep(inf, N), rep(0.4, N), rep(inf, N), rep(0.75, N)]
    if model == 0:
        lo += [rep(-5, N), rep(-inf, N)]; hi += [rep(inf, N), rep(5, N)]
    else:
        lo += [rep(-0.1, 2 * N), rep(-inf, 2 * N), rep(-inf, 12 * N)]; hi += [rep(inf, 2 * N), rep(0.1, 2 * N), rep(0, 12 * N)]
    return np.concatenate(lo), np.concatenate(hi)


def fd_build(P, u, h=1e-5):
    """The exact QP of the NLP at u by central differences of the rollout and of the rows (what test_exact_build_matches_numpy compares
    the device build with): dict(H, g, A (nC, nV), lb, ub, lbA, ubA, const).  Column j restarts the rollout at step j // 2."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    N = u.shape[0]
    X = nn.rollout(P.orc, P.model, P.track, P.x0, u, P.dt, P.integ)
    nx = X.shape[1]
    S = _slack_cols(P.model, N)
    nC, ns = S.shape
    nV = 2 * N + ns
    Phi, Au = np.zeros((nx * N, 2 * N)), np.zeros((nC, 2 * N))
    for j in range(2 * N):
        k = j // 2
        side = []
        for sg in (1.0, -1.0):
            up = u.copy(); up.flat[j] += sg * h
            Xp = X.copy()
            Xp[k:] = nn.rollout(P.orc, P.model, P.track, P.x0 if k == 0 else X[k - 1], up[k:], P.dt, P.integ)
            side.append((Xp, nn.rows(P.model, Xp, up)))
        Phi[:, j] = ((side[0][0] - side[1][0]) / (2 * h)).ravel()
        Au[:, j] = (side[0][1] - side[1][1]) / (2 * h)
    W = nn.weights(N, nx).ravel()
    ul = u.ravel()
    off = X.ravel() - Phi @ ul - P.x_ref.ravel()
    H = np.zeros((nV, nV))
    H[:2 * N, :2 * N] = 2 * (Phi.T @ (W[:, None] * Phi) + 10 * np.eye(2 * N))
    g = np.concatenate([2 * Phi.T @ (W * off), nn.r_soft(P.model)])
    lin0 = nn.rows(P.model, X, u) - Au @ ul
    lo, hi = row_bounds(P.model, N)
    return dict(H=H, g=g, A=np.hstack([Au, S]), lb=np.concatenate([np.tile(-U_MAX, N), np.zeros(ns)]),
                ub=np.concatenate([np.tile(U_MAX, N), np.full(ns, np.inf)]), lbA=lo - lin0, ubA=hi - lin0, const=float(np.sum(W * off ** 2)))


def cpu_loop(P, u_init, sweeps, trials=8, armijo=1e-4, tol_step=1e-6, tol_feas=1e-6, rho0=1.0):
    """The SQP of one instance on the CPU: init as sqp_init_kernel, then per sweep fd_build, the oracle's qp_solve (cold: the oracle
    takes no starting point) and sweep().  Returns dict(init=Point, clipped, records=[sweep()'s dict + start (J, viol, s) + lam_hard],
    status, u, s)."""
    u_init = np.asarray(u_init, dtype=np.float64).reshape(-1, 2)
    N = u_init.shape[0]
    ns = 1 if P.model == 0 else 4
    nV = 2 * N + ns
    init = evaluate(P, u_init, u_init, 0.0, np.zeros(ns))
    u, s, rho, J, viol = init.u, init.s, rho0, init.J, init.viol
    status, recs = RUNNING, []
    for k in range(sweeps):
        q = fd_build(P, u)
        z, fval, flag, it, lam = P.orc.qp_solve(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"])
        r = sweep((u, s, rho, J, viol), Qp(z, fval, q["const"], flag, it, lam), Opts(trials, armijo, tol_step, tol_feas, k, sweeps), P)
        r.update(start=(J, viol, s.copy()), lam_hard=float(np.max(np.abs(lam[nV:nV + 2 * N]))))
        recs.append(r)
        o = r["outcomes"][r["winner"]]
        u, s, rho, J, viol, status = o["u"], o["s"], r["rho"], o["J"], o["viol"], o["status"]
        if status != RUNNING:
            break
    return dict(init=init, clipped=bool(np.any(init.u != u_init)), records=recs, status=status, u=u, s=s)
