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


def adjoint(H, g, A, x, lam, ws, xbar, fbar=0.0, lstsq=False):
    """VJP of one QP's solution map on the working set ws.  Returns dict(g, lb, ub, lbA, ubA, H, A, w, mu, cond).  lstsq: the
    least-squares solution (for dependent working rows: w is unique, mu is the minimum-norm one of the equilibrated system); cond
    is then taken over the singular values that the least-squares solve keeps."""
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
        if lstsq:
            raise np.linalg.LinAlgError
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
    if lstsq and K.size:
        sv = np.linalg.svd(K, compute_uv=False)
        out["cond"] = float(sv[0] / sv[sv > 1e-13 * sv[0]].min())
    out["g"] = -w + fbar * x
    out["lb"] = np.where(wb < 0, mub, 0.0)
    out["ub"] = np.where(wb > 0, mub, 0.0)
    out["lbA"] = np.where(wc < 0, muA, 0.0)
    out["ubA"] = np.where(wc > 0, muA, 0.0)
    out["H"] = -0.5 * (np.outer(w, x) + np.outer(x, w)) + 0.5 * fbar * np.outer(x, x)
    act = wc != 0
    out["A"] = np.where(act[:, None], np.outer(lam[n:], w) - np.outer(muA, x), 0.0)
    return out


def conditions(H, A, ws):
    """What the VJP needs of a working set: dict(nF, nW, rank, cond) -- free variables, working rows, the rank of the working rows
    restricted to the free columns (equilibrated as in adjoint(); singular values above 1e-10 of the largest count) and the
    condition number of the equilibrated KKT matrix."""
    H = np.asarray(H, dtype=np.float64)
    n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    ws = np.asarray(ws)
    Fv, W = np.nonzero(ws[:n] == 0)[0], np.nonzero(ws[n:])[0]
    if len(Fv) == 0:   # a full vertex (or more): nothing to solve
        return dict(nF=0, nW=len(W), rank=0, cond=1.0)
    Aw = A[np.ix_(W, Fv)]
    hd = np.diag(H)[Fv]
    colmax = np.abs(Aw).max(axis=0) if len(W) else np.ones(len(Fv))
    cs = np.where(hd > 1e-12, 1.0 / np.sqrt(np.maximum(hd, 1e-300)), 1.0 / np.maximum(colmax, 1e-300))
    Aws = Aw * cs[None, :]
    rs = 1.0 / np.maximum(np.abs(Aws).max(axis=1), 1e-300) if len(W) else np.zeros(0)
    Aws = Aws * rs[:, None]
    k = len(W)
    K = np.block([[H[np.ix_(Fv, Fv)] * cs[:, None] * cs[None, :], Aws.T], [Aws, np.zeros((k, k))]])
    rank = 0
    if k and len(Fv):
        sv = np.linalg.svd(Aws, compute_uv=False)
        rank = int((sv > 1e-10 * sv[0]).sum()) if sv[0] > 0 else 0
    return dict(nF=len(Fv), nW=k, rank=rank, cond=float(np.linalg.cond(K)) if K.size else 1.0)


def compare(got, ref, H, g, A, x, lam, xbar, fbar=0.0):
    """Outputs of the VJP kernel for one instance and one cotangent column against a reference `ref` (adjoint()'s dict, or a closed
    form with the same keys).  got: key -> array for the keys to compare, in the device layout (H (n, n), A (n, m) = the memory of
    the column-major m x n matrix).  Returns (worst error / tolerance, (key, size of the reference, cond)).

    The tolerance is 1e-9 of the largest entry where the equilibrated KKT system is moderately conditioned; beyond that both
    solutions carry cond * eps, and the pinned multipliers (stationarity rows r - H w - A'mu) carry eps times the size of the terms
    that cancel in them; Hbar and Abar multiply that error by x and lambda (outer products)."""
    H, g, x, lam, xbar = (np.asarray(a, dtype=np.float64) for a in (H, g, x, lam, xbar))
    n = len(x)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    eps = np.finfo(float).eps
    rr = xbar + fbar * (H @ x + g)
    terms = np.max(np.abs(rr) + np.abs(H) @ np.abs(ref["w"]) + np.abs(A).T @ np.abs(ref["mu"][n:]))
    sol = max(np.abs(ref["w"]).max(), np.abs(ref["mu"]).max())
    worst, where = 0.0, None
    for key in got:
        want = ref[key].T if key == "A" else ref[key]
        amp = max(1.0, np.abs(x).max()) * (max(1.0, np.abs(lam).max()) if key == "A" else 1.0) if key in ("H", "A") else 1.0
        tol = max(1e-9 * max(1.0, np.abs(want).max() if want.size else 0.0), amp * max(10 * eps * ref["cond"] * sol, 100 * eps * terms))
        e = (np.abs(got[key] - want).max() if want.size else 0.0) / tol
        if e > worst or where is None:
            worst, where = max(worst, e), (key, float(np.abs(want).max()) if want.size else 0.0, ref["cond"])
    return worst, where


def residual(got, H, g, A, x, xbar, fbar=0.0):
    """Residual of the unscaled adjoint system at the (w, mu) that the kernel's outputs gbar, lb + ub, lbA + ubA imply, relative to
    the sizes of its terms (w relative to xbar / |H|, since w vanishes on a full vertex): max of the stationarity residual, A_W w on
    the rows with a multiplier and w on the pinned variables.  Returns (max, (stationarity, rows, pinned))."""
    H, g, x, xbar = (np.asarray(a, dtype=np.float64) for a in (H, g, x, xbar))
    n = len(x)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    w = -(got["g"] - fbar * x)
    mub = got["lb"] + got["ub"]
    muA = got["lbA"] + got["ubA"]
    rr = xbar + fbar * (H @ x + g)
    Hw, Atm = H @ w, A.T @ muA
    r1 = rr - Hw - mub - Atm
    sc1 = max(np.abs(rr).max(), np.abs(Hw).max(), np.abs(Atm).max(), np.abs(mub).max(), 1e-300)
    act = muA != 0
    wsc = max(np.abs(w).max(), np.abs(rr).max() / np.abs(H).max())
    r2 = np.abs(A[act] @ w).max() / (np.abs(A[act]).max() * wsc) if act.any() else 0.0
    r3 = np.abs(w[mub != 0]).max() / wsc if (mub != 0).any() else 0.0
    e1 = np.abs(r1).max() / sc1
    return max(e1, r2, r3), (e1, r2, r3)
