"""The cases the CPU and the GPU tests of the cell-wise corridor rows share: the shapes, the corridors, and the oracle's
solution of each line QP, computed once per case and left unchanged."""
import numpy as np

import corridor_cells_numpy as ccn
import corridor_numpy as cn
import plan_numpy as pn
import raceline_numpy as rn

MARGIN = 0.25
N_MAX = 0.75
# (N_s, N_c) -> why the shape is there
SHAPES = {
    (16, 8): "both minima",
    (40, 8): "nC = 10 (nV - 4): the signature of the dynamic LTV QPs",
    (48, 17): "nC = 3 (nV - 1): the signature of the kinematic LTV QPs, border 1",
    (40, 20): "border 4",
    (64, 16): "no border",
    (224, 112): "seven column tiles: the largest shape of the one-wavefront kernel",
    (226, 113): "eight column tiles: the smallest shape of the workgroup kernel",
    (232, 116): "the largest one-wavefront shape of an LTV QP (here eight tiles: no border is split off)",
    (234, 117): "the smallest workgroup shape of an LTV QP",
    (392, 196): "FSAEMPC_MAX_NV: twelve tiles and the last four control points as the border",
    (500, 100): "the workload",
}
BLOCKED_CPU = [(16, 8), (64, 16), (96, 48), (256, 128), (392, 196)]
BLOCKED_GPU = [(64, 16), (96, 48)]      # (a subset of BLOCKED_CPU)
_KAPPA, _SOL = {}, {}


def kappa(orc, otr, N_s):
    key = (otr.name, otr.L, N_s)
    if key not in _KAPPA:
        k = pn.kappa_cells(orc, otr, N_s); k.setflags(write=False)
        _KAPPA[key] = k
    return _KAPPA[key]


def corridor(orc, otr, N_s, kind):
    """(n_lo, n_hi) of N_w = N_s cells.  "kappa": +-1.5 m where |kappa| < 0.02, +-0.75 m elsewhere; "constant": +-0.75 m; "blocked": the
    kappa corridor with n_lo = 0.1 over max(1, N_s / 10) cells from cell N_s / 4 on (the centre line is outside it there)."""
    if kind == "constant":
        return np.full(N_s, -N_MAX), np.full(N_s, N_MAX)
    lo, hi = ccn.kappa_corridor(kappa(orc, otr, N_s))
    if kind == "blocked":
        lo = lo.copy(); lo[blocked_cells(N_s)] = 0.1
    return lo, hi


def blocked_cells(N_s):
    return slice(N_s // 4, N_s // 4 + max(1, N_s // 10))


def oracle_cells(orc, otr, N_s, N_c, kind):
    """The oracle on (H, g, B, -+1e10, lbA, ubA): dict(x, fval, flag, iter, lam, polished, H, g, B, lbA, ubA, n)."""
    key = (otr.name, otr.L, N_s, N_c, kind, "cells")
    if key not in _SOL:
        H, g = rn.qp(orc, otr, N_s, N_c)
        lo, hi = corridor(orc, otr, N_s, kind)
        lbA, ubA = ccn.row_bounds(lo, hi, otr.L / N_s, otr.L, N_s, MARGIN)
        B = ccn.matrix(N_s, N_c)
        free = np.full(N_c, ccn.FREE)
        r = orc.qp_solve_batch_aux(H[None], g[None], np.ascontiguousarray(B.T)[None], -free[None], free[None], lbA[None], ubA[None])
        sol = dict(x=r["x"][0], fval=float(r["fval"][0]), flag=int(r["exitflag"][0]), iter=int(r["iter"][0]), lam=r["lam"][0],
                   polished=int(r["polished"][0]), H=H, g=g, B=B, lbA=lbA, ubA=ubA, n=ccn.apply(r["x"][0], N_s))
        for v in sol.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SOL[key] = sol
    return _SOL[key]


def oracle_points(orc, otr, N_s, N_c, kind):
    """The oracle on the point-box form of the same corridor (tests/corridor_numpy.py::control_point_bounds): dict(x, fval, flag, n)."""
    key = (otr.name, otr.L, N_s, N_c, kind, "points")
    if key not in _SOL:
        H, g = rn.qp(orc, otr, N_s, N_c)
        lo, hi = corridor(orc, otr, N_s, kind)
        lb, ub = cn.control_point_bounds(lo, hi, otr.L / N_s, otr.L, N_s, N_c, MARGIN)
        x, f, flag, it, lam = orc.qp_solve(H, g, np.zeros((0, N_c)), lb, ub, np.zeros(0), np.zeros(0))
        x.setflags(write=False)
        _SOL[key] = dict(x=x, fval=f, flag=flag, n=ccn.apply(x, N_s))
    return _SOL[key]
