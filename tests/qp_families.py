"""Generic QP families off the LTV-MPC shapes (numpy only), for tests of the batched QP solve and of the CPU oracle.

    min 1/2 x'Hx + x'g   s.t.  lb <= x <= ub,  lbA <= A x <= ubA

make(family, nV, nC, inst) returns H (nV, nV), g, A (nC, nV), lb, ub, lbA, ubA as mathematical matrices plus `x_star` (the closed-form
minimiser, None where there is none) and `lam_star` (its multipliers, nV + nC entries in the solver's convention
H x + g - lam_b - A' lam_A = 0, None where there is no x_star); stack() puts a list of them into the device layout of the C ABI
(H (B, nV, nV), A (B, nV, nC) = per-instance column-major nC x nV, vectors (B, *)).  Everything is deterministic: the matrices are
seeded by (family, nV, nC, ha_inst), the vectors by (family, nV, nC, inst); ha_inst defaults to inst, and instances that name the
same ha_inst share H and A.

H is symmetric positive definite with eigenvalues log-spaced over 1 .. 1e3 in a random orthogonal basis.  Every QP is feasible by
construction around a random point xs: bounds xs +- 1, row ranges A xs +- U(0.1, 1), unless the family says otherwise.

  F  nothing active: every bound and row side infinite, written as a mix of +-inf and the reference's +-1e10 fillers; x* = -H^-1 g.
  E  equalities: bounds infinite, the first min(nC, nV / 2) rows have lbA = ubA, the rest are free; x* from the dense KKT system.
  R  row structure: row r is dense up to a random last column and zero behind it, in random order (the prep kernel's sort by last
     column tile has work to do); row 1 is all zero with range [-1, 1]; row 2 touches only the last variable (a border column wherever
     there is a border); row 4 is a copy of row 3 with its scale and range; rows are scaled by 10^U(-4, 4) and their ranges with them
     (A xs +- scale U(0.01, 0.3)); every third lbA and every third ubA (offset 1) is infinite, every second ub; variable 3 is fixed.
  S  slack column: the last variable has a zero row and column in H, cost 1e6, lb = 0, ub = inf, and enters every third row with
     coefficient -1; rows are upper-bounded only; the soft rows have ubA = A xs + U(-0.5, 1), so some of them need s > 0.
  V  R without the duplicate (for the sensitivities, which need independent working rows): every array is R's except row 4, which
     is a row of its own kind -- dense up to a random last column, its own scale 10^U(-4, 4), lbA = A xs - scale U(0.01, 0.3) and no
     upper side, as the pattern of R gives row 4 -- drawn from streams of its own, so that R does not move.  Not in FAMILIES:
     the tests of the forward solve do not run it.
"""
import numpy as np

FAMILIES = ("F", "E", "R", "S")
# (nV, nC); (21, 60) and (24, 200) carry the row / column signature of the kinematic / dynamic LTV-MPC QPs (nC = 3 (nV - 1) resp.
# 10 (nV - 4)) and so get the solver's dummy-padded layout; the others avoid it on purpose
SHAPES = [(15, 3), (16, 16), (18, 7), (35, 50), (52, 70), (66, 33), (96, 130), (116, 40), (117, 30), (130, 65), (147, 257), (180, 64),
          (21, 60), (24, 200)]
SHAPES_F_ONLY = [(20, 0)]
# shapes for the tests of the VJP kernel (csrc/qp_sens.hip): those of SHAPES at which the working rows of V come out independent, plus
# both sides of the switch of its factor from LDS to the workspace slot (np = 128: nV = 128 | 129), the next tile (144 | 145) and
# FSAEMPC_MAX_NV; (16, 16) and (96, 130) have nV a multiple of 16 (no identity padding), F there has no working row at all
VJP_SHAPES = [(15, 3), (16, 16), (18, 7), (35, 50), (66, 33), (96, 130), (116, 40), (117, 30), (130, 65), (180, 64),
              (128, 40), (129, 40), (144, 30), (145, 30), (196, 50)]
# first instance of the 8 that the VJP tests take, where it is not 0: with the CPU oracle as the forward, V (16, 16) instance 2,
# (66, 33) instance 5 and (96, 130) instance 1 come back as interior-point iterates (refinement not accepted), and the working set
# that the rule reads off such an iterate is not a vertex's (tests/test_sens_shapes_cpu.py asserts the conditions on the 8 taken)
VJP_FIRST = {("V", 16, 16): 3, ("V", 66, 33): 6, ("V", 96, 130): 2}
FILLER = 1e10          # the reference writes "no bound" as +-1e10 (ltvmpc_*.m); the solvers treat |bound| >= 1e9 as infinite
KEYS = ("H", "g", "A", "lb", "ub", "lbA", "ubA")


def shapes(family):
    return SHAPES + (SHAPES_F_ONLY if family == "F" else [])


def _rng(family, nV, nC, inst, stream):
    return np.random.default_rng([20260, (FAMILIES + ("V",)).index(family), nV, nC, inst, stream])


def _spd(rng, n):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    H = (Q * np.logspace(0.0, 3.0, n)) @ Q.T
    return 0.5 * (H + H.T)


def _no_bound(k, sign):
    """k entries of "no bound" on the given side: +-inf and the +-1e10 filler in turn."""
    return sign * np.where(np.arange(k) % 2 == 0, np.inf, FILLER)


def make(family, nV, nC, inst, ha_inst=None):
    if family == "V":
        q = make("R", nV, nC, inst, ha_inst)
        q["family"] = "V"
        if nC > 4:
            rm = _rng("V", nV, nC, inst if ha_inst is None else ha_inst, 0)
            rv = _rng("V", nV, nC, inst, 1)
            xs = _rng("R", nV, nC, inst, 1).standard_normal(nV)   # the feasible point of R: the first draw of its vector stream
            row = rm.standard_normal(nV)
            row[np.arange(nV) > rm.integers(0, nV)] = 0.0
            scale = 10.0 ** rm.uniform(-4.0, 4.0)
            q["A"][4] = scale * row
            q["lbA"][4], q["ubA"][4] = q["A"][4] @ xs - scale * rv.uniform(0.01, 0.3), np.inf
        return q
    rm = _rng(family, nV, nC, inst if ha_inst is None else ha_inst, 0)   # matrices
    rv = _rng(family, nV, nC, inst, 1)                                   # vectors
    x_star = lam_star = None
    if family == "S":
        H = np.zeros((nV, nV)); H[:nV - 1, :nV - 1] = _spd(rm, nV - 1)
    else:
        H = _spd(rm, nV)
    A = rm.standard_normal((nC, nV))
    xs = rv.standard_normal(nV)
    g = 10.0 * rv.standard_normal(nV)
    if family == "F":
        lb, ub = _no_bound(nV, -1.0), _no_bound(nV, 1.0)
        lbA, ubA = _no_bound(nC, -1.0)[::-1].copy(), _no_bound(nC, 1.0)
        x_star = -np.linalg.solve(H, g)
        lam_star = np.zeros(nV + nC)
    elif family == "E":
        lb, ub = _no_bound(nV, -1.0), _no_bound(nV, 1.0)
        lbA, ubA = _no_bound(nC, -1.0), _no_bound(nC, 1.0)[::-1].copy()
        k = min(nC, nV // 2)
        b = A[:k] @ xs
        lbA[:k] = b; ubA[:k] = b
        K = np.block([[H, -A[:k].T], [A[:k], np.zeros((k, k))]])
        rhs = np.concatenate([-g, b])
        sol = np.linalg.solve(K, rhs)
        sol += np.linalg.solve(K, rhs - K @ sol)
        x_star = sol[:nV]
        lam_star = np.zeros(nV + nC)
        lam_star[nV:nV + k] = sol[nV:]
    elif family == "R":
        last = rm.integers(0, nV, nC)
        A[np.arange(nV)[None, :] > last[:, None]] = 0.0
        scale = 10.0 ** rm.uniform(-4.0, 4.0, nC)
        if nC > 1:
            A[1] = 0.0
        if nC > 2:
            A[2] = 0.0; A[2, nV - 1] = 1.0 + rm.uniform()
        A *= scale[:, None]
        if nC > 4:
            A[4] = A[3]; scale[4] = scale[3]
        lbA = A @ xs - scale * rv.uniform(0.01, 0.3, nC)
        ubA = A @ xs + scale * rv.uniform(0.01, 0.3, nC)
        lbA[0::3] = -np.inf; ubA[1::3] = np.inf
        if nC > 1:
            lbA[1], ubA[1] = -1.0, 1.0
        if nC > 4:
            lbA[4], ubA[4] = lbA[3], ubA[3]
        lb, ub = xs - 1.0, xs + 1.0
        ub[::2] = np.inf
        lb[3] = ub[3] = xs[3]
    elif family == "S":
        xs[nV - 1] = 0.0
        g[nV - 1] = 1e6
        soft = np.arange(nC) % 3 == 0
        A[:, nV - 1] = np.where(soft, -1.0, 0.0)
        lbA = np.full(nC, -np.inf)
        ubA = A @ xs + np.where(soft, rv.uniform(-0.5, 1.0, nC), rv.uniform(0.1, 1.0, nC))
        lb, ub = xs - 1.0, xs + 1.0
        lb[nV - 1], ub[nV - 1] = 0.0, np.inf
    else:
        raise ValueError(family)
    return dict(H=H, g=g, A=A, lb=lb, ub=ub, lbA=lbA, ubA=ubA, x_star=x_star, lam_star=lam_star, family=family)


def make_infeasible(nV, nC, inst):
    """Family R with the duplicate rows 3 and 4 given disjoint ranges: A_3 x <= u and A_3 x >= u + |u| + scale."""
    q = make("R", nV, nC, inst)
    assert nC > 4 and np.array_equal(q["A"][3], q["A"][4])
    u = q["ubA"][3]
    q["lbA"][4], q["ubA"][4] = u + abs(u) + np.abs(q["A"][3]).max(), np.inf
    return q


def stack(qps, shared_HA=False):
    """Device layout of a batch.  With shared_HA H and A are given once ((nV, nV) / (nV, nC)): all instances must hold the same."""
    out = {k: np.ascontiguousarray(np.stack([q[k] for q in qps])) for k in ("g", "lb", "ub", "lbA", "ubA")}
    if shared_HA:
        assert all(np.array_equal(q["H"], qps[0]["H"]) and np.array_equal(q["A"], qps[0]["A"]) for q in qps)
        out["H"] = np.ascontiguousarray(qps[0]["H"].T); out["A"] = np.ascontiguousarray(qps[0]["A"].T)
    else:
        out["H"] = np.ascontiguousarray(np.stack([q["H"].T for q in qps]))
        out["A"] = np.ascontiguousarray(np.stack([q["A"].T for q in qps]))
    if all(q.get("x_star") is not None for q in qps):
        out["x_star"] = np.stack([q["x_star"] for q in qps])
        out["lam_star"] = np.stack([q["lam_star"] for q in qps])
    return out


def batch(family, nV, nC, B, first=0):
    return stack([make(family, nV, nC, first + i) for i in range(B)])


def vjp_first(family, nV, nC):
    return VJP_FIRST.get((family, nV, nC), 0)


def vjp_batch(family, nV, nC, B):
    """The batch that the VJP tests take of (family, nV, nC): B instances from vjp_first() on."""
    return batch(family, nV, nC, B, first=vjp_first(family, nV, nC))
