"""Dense numpy adjoint of the QP solve on a fixed working set (the statement the VJP kernel of csrc/qp_sens.hip is tested against).

On a working set W (encoding of kkt_numpy.working_set: -1 lower, 0 inactive, +1 upper; n + m entries) the solution map of
vertex_from_working_set is: free variables F and the multipliers of the working rows solve one linear system, the pinned variables sit
on their bounds.  Its adjoint for a cotangent xbar of x (and fbar of fval = 1/2 x'Hx + g'x) solves, with A^ = [A_W; unit rows of the
pinned bounds],

    H w + A^' mu = xbar + fbar (H x + g),    A^ w = 0,

and gives gbar = -w + fbar x, bbar = mu on each working side, Hbar = -(w x' + x w')/2 + fbar x x'/2, Abar_r = lam_r w' - mu_r x'.
Same algebra as vertex_from_working_set (free/pinned split, equilibration; LU with refinement, least squares if singular); layout of one QP: H (n,n),
A (m,n) as mathematical matrices."""
import numpy as np


def working_set_rule(lb, ub, lbA, ubA, x, A, lam, inf_bound=1e9):
    """The solver's refinement rule: a side is in the working set iff its multiplier has the side's sign and exceeds the side's slack."""
    lam = np.asarray(lam, dtype=np.float64)
    n = len(x)
    v = np.concatenate([x, np.asarray(A).reshape(-1, n) @ x])
    lo = np.concatenate([lb, lbA])
    hi = np.concatenate([ub, ubA])
    act_lo = (lo > -inf_bound) & (lam > 0) & (lam > np.abs(v - lo))
    act_hi = ~act_lo & (hi < inf_bound) & (lam < 0) & (-lam > np.abs(hi - v))
    return np.where(act_lo, -1, np.where(act_hi, 1, 0))


def adjoint(H, g, A, x, lam, ws, xbar, fbar=0.0):
    """VJP of one QP's solution map on the working set ws.  Returns dict(g, lb, ub, lbA, ubA, H, A, w, mu)."""
    H, g, x, lam, xbar = (np.asarray(a, dtype=np.float64) for a in (H, g, x, lam, xbar))
    n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    m = A.shape[0]
    ws = np.asarray(ws)
    wb, wc = ws[:n], ws[n:]
    Pv, Fv, W = np.nonzero(wb)[0], np.nonzero(wb == 0)[0], np.nonzero(wc)[0]
    r = xbar + fbar * (H @ x + g)
    Aw = A[np.ix_(W, Fv)]
    hd = np.diag(H)[Fv]
    colmax = np.abs(Aw).max(axis=0) if len(W) else np.ones(len(Fv))
    cs = np.where(hd > 1e-12, 1.0 / np.sqrt(np.maximum(hd, 1e-300)), 1.0 / np.maximum(colmax, 1e-300))
    Aws = Aw * cs[None, :]
    rs = 1.0 / np.maximum(np.abs(Aws).max(axis=1), 1e-300) if len(W) else np.zeros(0)
    Aws = Aws * rs[:, None]
    nf, k = len(Fv), len(W)
    K = np.block([[H[np.ix_(Fv, Fv)] * cs[:, None] * cs[None, :], Aws.T], [Aws, np.zeros((k, k))]])
    rhs = np.concatenate([r[Fv] * cs, np.zeros(k)])
    try:   # LU with refinement where the working rows are independent (the least-squares fall-back truncates at rcond)
        sol = np.linalg.solve(K, rhs)
        for _ in range(3):
            sol = sol + np.linalg.solve(K, rhs - K @ sol)
    except np.linalg.LinAlgError:
        sol = np.linalg.lstsq(K, rhs, rcond=1e-13)[0]
        for _ in range(2):
            sol = sol + np.linalg.lstsq(K, rhs - K @ sol, rcond=1e-13)[0]
    w = np.zeros(n)
    w[Fv] = sol[:nf] * cs
    muA = np.zeros(m)
    muA[W] = sol[nf:] * rs
    mub = np.zeros(n)
    mub[Pv] = (r - H @ w - A.T @ muA)[Pv]
    out = dict(w=w, mu=np.concatenate([mub, muA]), cond=float(np.linalg.cond(K)) if K.size else 1.0)
    out["g"] = -w + fbar * x
    out["lb"] = np.where(wb < 0, mub, 0.0)
    out["ub"] = np.where(wb > 0, mub, 0.0)
    out["lbA"] = np.where(wc < 0, muA, 0.0)
    out["ubA"] = np.where(wc > 0, muA, 0.0)
    out["H"] = -0.5 * (np.outer(w, x) + np.outer(x, w)) + 0.5 * fbar * np.outer(x, x)
    act = wc != 0
    out["A"] = np.where(act[:, None], np.outer(lam[n:], w) - np.outer(muA, x), 0.0)
    return out
