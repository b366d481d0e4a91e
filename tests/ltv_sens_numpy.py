"""Dense float64 restatement of the VJP of the LTV-MPC step in x0 and x_ref (the statement fsaempc_ltv_step_vjp_batch_device --
ltv_vjp_pre_kernel, the QP VJP kernel, ltv_vjp_chain_kernel of csrc/ltv_build.hip -- is tested against).

With x_lin and u_lin fixed the step is: build (x0, x_ref) -> (pred, g, lbA, ubA, const; H, A, lb, ub, Bt do not move), solve the QP
for z = [u_opt; slack], x_opt = pred + Bt z, fval = fval_qp + const.  Its VJP is therefore

    zbar = [ubar; sbar] + Bt' xbar,
    (gbar, lbAbar, ubAbar) = the QP's adjoint on the working set of the solver's rule (sens_numpy.adjoint, fbar folded in),
    x0bar  = J_pred' xbar + J_g' gbar + J_lbA' lbAbar + J_ubA' ubAbar + fbar J_const    (the J in x0),
    xrefbar likewise with the J in x_ref (J_pred = 0 there).

Nothing here knows how the build depends on x0 and x_ref: the Jacobians are central differences of a build callable with a unit
step.  The build is affine in both arguments and const is quadratic, so these differences are exact up to rounding; an infinite
bound (|.| >= 1e9 or inf) has a zero derivative.  Layout: batches as the oracle and the device hold them (H (B, nV, nV), A (B, nV, nC)
= the memory of the column-major nC x nV matrix, Bt (B, nV, nx N) = that of the column-major nx N x nV matrix, vectors (B, *))."""
import numpy as np

import sens_numpy as sn

EPS = np.finfo(float).eps
INF_BOUND = 1e9
MOVING = ("pred", "g", "lbA", "ubA", "const")


def build_jacobians(build, x0, x_ref):
    """build(x0 (B, nx), x_ref (B, R)) -> dict with the keys of MOVING (numpy; const (B,)).  Returns dict(x0=..., x_ref=...), each
    dict(J={key: (B, n_arg, n_key)}, T={key: (B, n_arg, n_key)}): J the central differences (q+ - q-) / 2 at a unit step, T the
    size (|q+| + |q-|) / 2 of the two numbers each J entry is the difference of -- 100 eps T bounds the rounding the differencing
    leaves in J (the builds themselves are a few eps accurate relative to their entries' terms)."""
    out = {}
    for arg, base in (("x0", x0), ("x_ref", x_ref)):
        n = base.shape[1]
        J, T = {}, {}
        for j in range(n):
            e = np.zeros_like(base)
            e[:, j] = 1.0
            qp, qm = (build(x0 + s * e, x_ref) if arg == "x0" else build(x0, x_ref + s * e) for s in (1.0, -1.0))
            for key in MOVING:
                a, b = (np.asarray(q[key], dtype=np.float64).reshape(len(base), -1) for q in (qp, qm))
                fin = (np.abs(a) < INF_BOUND) & (np.abs(b) < INF_BOUND)
                with np.errstate(invalid="ignore"):
                    d, t = np.where(fin, 0.5 * (a - b), 0.0), np.where(fin, 0.5 * (np.abs(a) + np.abs(b)), 0.0)
                if key not in J:
                    J[key] = np.zeros((len(base), n, d.shape[1]))
                    T[key] = np.zeros((len(base), n, d.shape[1]))
                J[key][:, j], T[key][:, j] = d, t
        out[arg] = dict(J=J, T=T)
    return out


def key_tolerances(ref, H, g, A, x, xbar, fbar=0.0, keys=("g", "lbA", "ubA")):
    """The tolerance sens_numpy.compare grants each of `keys` of the QP VJP for one instance and column (its amp is 1 for these
    keys): max(1e-9 max(1, |ref|_inf), 10 eps cond |solution|_inf, 100 eps |terms of the pinned stationarity rows|_inf).  Restated
    because compare only returns the ratio; tests/test_ltv_sens_cpu.py pins the two to each other."""
    H, g, x, xbar = (np.asarray(a, dtype=np.float64) for a in (H, g, x, xbar))
    n = len(x)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    rr = xbar + fbar * (H @ x + g)
    terms = np.max(np.abs(rr) + np.abs(H) @ np.abs(ref["w"]) + np.abs(A).T @ np.abs(ref["mu"][n:]))
    sol = max(np.abs(ref["w"]).max(), np.abs(ref["mu"]).max())
    floor = max(10 * EPS * ref["cond"] * sol, 100 * EPS * terms)
    return {key: max(1e-9 * max(1.0, np.abs(ref[key]).max() if ref[key].size else 0.0), floor) for key in keys}


def working_sets(q, z, lam):
    """The working set of the solver's rule per instance (n + m entries: -1 lower, 0 inactive, +1 upper)."""
    return [sn.working_set_rule(q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b], z[b], q["A"][b].T, lam[b]) for b in range(len(z))]


def step_vjp(q, jac, z, lam, cot, ns, only=None):
    """VJP of the step for the instances of `only` (default: all).  q: one build's outputs (H, g, A, lb, ub, lbA, ubA, Bt); jac:
    build_jacobians at the same (x0, x_ref); z (B, nV) = [u_opt; slack] and lam (B, nV + nC): the forward's results; cot: dict(ubar
    (B, k, 2N), xbar (B, k, R), sbar (B, k, ns), fbar (B, k)), None = 0; ns: the number of slack variables (nV = 2N + ns).

    Returns dict(x0 (B, k, nx), x_ref (B, k, R), tol_x0, tol_x_ref (same shapes), adj: {(b, c): sens_numpy.adjoint's dict}, ws: {b:
    working set}); instances outside `only` keep zeros.  The tolerance of an output entry: the tolerances of gbar, lbAbar, ubAbar
    (key_tolerances), each times the sum of the absolute Jacobian entries that multiply that key in the entry, plus 100 eps times
    the sum of the absolute terms of the entry -- a term being a cotangent entry times the (|q+| + |q-|) / 2 of its Jacobian entry."""
    B, nV = q["g"].shape
    given = [v for v in cot.values() if v is not None]
    k = given[0].shape[1]
    zero = lambda n: np.zeros((B, k, n))
    ubar = cot["ubar"] if cot.get("ubar") is not None else zero(nV - ns)
    sbar = cot["sbar"] if cot.get("sbar") is not None else zero(ns)
    R = q["Bt"].shape[2]
    xbar = cot["xbar"] if cot.get("xbar") is not None else zero(R)
    fbar = cot["fbar"] if cot.get("fbar") is not None else np.zeros((B, k))
    out = {a: np.zeros((B, k, jac[a]["J"]["g"].shape[1])) for a in ("x0", "x_ref")}
    tol = {a: np.zeros_like(out[a]) for a in out}
    adj, wss = {}, {}
    for b in (range(B) if only is None else only):
        Hb, Ab = q["H"][b].T, q["A"][b].T
        ws = sn.working_set_rule(q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b], z[b], Ab, lam[b])
        wss[b] = ws
        for c in range(k):
            zbar = np.concatenate([ubar[b, c], sbar[b, c]]) + q["Bt"][b] @ xbar[b, c]
            ad = sn.adjoint(Hb, q["g"][b], Ab, z[b], lam[b], ws, zbar, fbar[b, c])
            adj[(b, c)] = ad
            kt = key_tolerances(ad, Hb, q["g"][b], Ab, z[b], zbar, fbar[b, c])
            bars = dict(pred=xbar[b, c], g=ad["g"], lbA=ad["lbA"], ubA=ad["ubA"], const=np.array([fbar[b, c]]))
            for a in out:
                J, T = jac[a]["J"], jac[a]["T"]
                out[a][b, c] = sum(J[key][b] @ bars[key] for key in MOVING)
                tol[a][b, c] = sum(kt[key] * np.abs(J[key][b]).sum(axis=1) for key in kt) \
                    + 100 * EPS * sum(T[key][b] @ np.abs(bars[key]) for key in MOVING)
    return dict(x0=out["x0"], x_ref=out["x_ref"], tol_x0=tol["x0"], tol_x_ref=tol["x_ref"], adj=adj, ws=wss)


def row_cotangent(res, b, c=0):
    """lbAbar + ubAbar of instance b, column c: what the chain multiplies each row's coefficients by."""
    ad = res["adj"][(b, c)]
    return ad["lbA"] + ad["ubA"]
