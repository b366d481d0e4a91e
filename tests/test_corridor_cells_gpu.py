"""GPU tests of the cell-wise corridor rows of the racing line: the rows (1), the solve of every shape against the
oracle (2), what the form gains over the point boxes (3), a blocked side (4), a pinched plan in a batch (5), the profile and the
multipliers (6) and the default path (7).  The numpy side is tests/corridor_cells_numpy.py, the cases and the oracle's solutions
tests/corridor_cells_cases.py (shared with tests/test_corridor_cells_cpu.py, which shows the oracle solves everything asked here).
fsg2019, margin 0.25 and the kappa corridor (+-1.5 m where |kappa| < 0.02, +-0.75 m elsewhere) at N_w = N_s unless stated."""
import ctypes as C

import numpy as np
import pytest
from conftest import relerr

import corridor_cells_cases as cases
import corridor_cells_numpy as ccn
import raceline_numpy as rn
from kkt_numpy import kkt_certificate

pytestmark = pytest.mark.gpu

MARGIN = cases.MARGIN
ROW_TOL = 1e-14         # tests/test_corridor_gpu.py on the control-point boxes
BUILD_TOL = 1e-9        # tests/test_raceline_gpu.py on table and t
KKT_TOL = 1e-6          # the tolerances of tests/test_gpu_parity.py
FVAL_TOL = 1e-6
X_TOL = 5e-3
X_TOL_VERTEX = 1e-6
ON_ROW = 1e-9           # a cell counts as inside its limits up to this (tests/test_corridor_gpu.py, test D)


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def tr(fm):
    return fm.Track.load("fsg2019")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _host(torch, *ts):
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in ts]


def _outputs(torch, plan):
    return dict(zip(("line", "flag", "table", "t"), _host(torch, plan.line, plan.line_flag, plan.table, plan.t)))


def _qp(fm, torch, tr, cor, N_s, N_c, n_plans):
    """the QP the cells path solves, as the device makes it: H, g, A (N_c, N_s), lbA, ubA on the host"""
    H, g = fm.raceline_qp(tr, N_s, N_c)
    A, lbA, ubA = cor.line_rows(N_s, N_c, MARGIN, n_plans=n_plans)
    return _host(torch, H, g, A, lbA, ubA)


def _certificate(H, g, A, lbA, ubA, line, row_lambda):
    P, N_c = line.shape
    free = np.full((P, N_c), ccn.FREE)
    lam = np.concatenate([np.zeros((P, N_c)), row_lambda], axis=1)           # (free control points carry no multiplier)
    rep = lambda a: np.broadcast_to(a, (P,) + a.shape)
    return kkt_certificate(rep(H), rep(g), rep(A), -free, free, lbA, ubA, line, lam)


def smooth_tables(L, N_w):
    """a corridor that is no constant anywhere: n_hi = 0.75 + 0.75 sin^2(3 pi s / L), n_lo = -(0.75 + 0.5 sin^2(2 pi s / L + 0.7))"""
    s = np.arange(N_w) * L / N_w
    return -(0.75 + 0.5 * np.sin(2 * np.pi * s / L + 0.7) ** 2), 0.75 + 0.75 * np.sin(3 * np.pi * s / L) ** 2


# ---- 1. the rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_s,N_c", [(16, 8), (48, 17), (64, 16), (333, 41), (500, 100)])
def test_1_matrix_is_the_restatement_bit_for_bit(fm, torch_, tr, N_s, N_c):
    """Straight through the C entry into buffers filled with NaN beforehand: every element is written."""
    torch = torch_
    cor = fm.Corridor.constant(tr.L, 0.75)
    A = torch.full((N_c, N_s), float("nan"), dtype=torch.float64, device="cuda")
    lbA, ubA = torch.full((3, N_s), float("nan"), dtype=torch.float64, device="cuda"), torch.full((3, N_s), float("nan"), dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert fm.lib().fsaempc_corridor_line_rows_device(cor.ref(), C.c_double(tr.L), 3, N_s, N_c, C.c_double(MARGIN), P(A), P(lbA), P(ubA), None) == 0
    A, lbA, ubA = _host(torch, A, lbA, ubA)
    assert _same_bits(A, np.ascontiguousarray(ccn.matrix(N_s, N_c).T))
    assert np.array_equal(lbA, np.full((3, N_s), -0.5)) and np.array_equal(ubA, np.full((3, N_s), 0.5))     # (a constant table: the constant exactly)
    A2 = _host(torch, cor.line_rows(N_s, N_c, MARGIN)[0])[0]
    assert _same_bits(A2, A)


@pytest.mark.parametrize("N_w", [32, 50, 64, 200])
def test_1_row_bounds_against_the_lookup(fm, torch_, tr, N_w):
    """N_s = 64.  N_w = 64: every lookup exactly on a cell; 32: every other one, the last half way into the last cell (the wrap to
    cell 0); 50 and 200: N_w no divisor or multiple of N_s, 50 with the last lookup in the last cell.  Shared and one per plan;
    a plan with a pinched cell has NaN in both bounds of the rows that read it and nowhere else."""
    torch = torch_
    L, N_s, N_c = tr.L, 64, 16
    lo, hi = smooth_tables(L, N_w)
    ds = L / N_w
    s = np.arange(N_s) * L / N_s
    assert int(np.floor(s[-1] / ds)) == N_w - 1 or N_w in (64, 200)
    wl, wu = ccn.row_bounds(lo, hi, ds, L, N_s, MARGIN)
    A, lbA, ubA = _host(torch, *fm.Corridor.from_table(lo, hi, L).line_rows(N_s, N_c, MARGIN))
    assert lbA.shape == (1, N_s) and np.isfinite(wl).all()
    assert np.abs(lbA[0] - wl).max() <= ROW_TOL and np.abs(ubA[0] - wu).max() <= ROW_TOL, (np.abs(lbA[0] - wl).max(), np.abs(ubA[0] - wu).max())
    shared3 = _host(torch, *fm.Corridor.from_table(lo, hi, L).line_rows(N_s, N_c, MARGIN, n_plans=3))
    assert _same_bits(shared3[1], np.tile(lbA, (3, 1))) and _same_bits(shared3[2], np.tile(ubA, (3, 1))) and _same_bits(shared3[0], A)
    # one corridor per plan: plan 1 wider, plan 2 pinched (n_hi = n_lo + 0.4 < 2 margin in one cell of the table)
    tl, th = np.tile(lo, (3, 1)), np.tile(hi, (3, 1))
    th[1] += 0.05
    pinch = 25                                                     # (cell 25 of every table is read by a row: 25 = i N_w / 64 for an integer i)
    assert (25 * N_s) % N_w == 0
    th[2, pinch] = tl[2, pinch] + 0.4
    A3, lbA3, ubA3 = _host(torch, *fm.Corridor.from_table(tl, th, L).line_rows(N_s, N_c, MARGIN))
    assert _same_bits(A3, A) and _same_bits(lbA3[0], lbA[0]) and _same_bits(ubA3[0], ubA[0])
    for p in (1, 2):
        wl, wu = ccn.row_bounds(tl[p], th[p], ds, L, N_s, MARGIN)
        assert np.array_equal(np.isnan(lbA3[p]), np.isnan(wl)) and np.array_equal(np.isnan(ubA3[p]), np.isnan(wl)) and np.array_equal(np.isnan(wl), np.isnan(wu))
        ok = np.isfinite(wl)
        assert np.abs(lbA3[p][ok] - wl[ok]).max() <= ROW_TOL and np.abs(ubA3[p][ok] - wu[ok]).max() <= ROW_TOL
        assert (~ok).sum() == 0 if p == 1 else 1 <= (~ok).sum() < N_s // 4, (p, (~ok).sum())


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_s,N_c", list(cases.SHAPES))
def test_2_solve_against_the_oracle(fm, torch_, orc, otrack, tr, N_s, N_c):
    """Small shapes solve two plans (the kappa corridor and the constant band, one corridor per plan), the others one."""
    torch = torch_
    L = tr.L
    kinds = ("kappa", "constant") if N_c <= 20 else ("kappa",)
    tabs = [cases.corridor(orc, otrack, N_s, k) for k in kinds]
    cor = fm.Corridor.from_table(np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), L)
    P = len(kinds)
    plan = fm.Plan.raceline(fm.KINEMATIC, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor, rows="cells", want_row_lambda=True)
    assert plan.P == P
    line, flag, lam = _host(torch, plan.line, plan.line_flag, plan.row_lambda)
    H, g, A, lbA, ubA = _qp(fm, torch, tr, cor, N_s, N_c, P)
    # the same QP through the general entry: its iteration count and whether it ends on the refined vertex
    free = torch.full((P, N_c), ccn.FREE, dtype=torch.float64, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n_slack = 4 if N_c > 192 else 0                                        # (the slack count the cells path gives the solve)
    gen = fm.qp_solve_batch_device(dev(H)[None], dev(np.tile(g, (P, 1))), dev(A)[None], -free, free, dev(lbA), dev(ubA), shared_HA=True, want_aux=True,
                                   n_slack=n_slack)
    gx, gflag, giter, gpol = _host(torch, gen["x"], gen["exitflag"], gen["iter"], gen["polished"])
    lay = fm.qp_layout(N_c, N_s, n_slack)
    print("(%d, %d) %s: %s, flags %s, iterations %s, polished %s" % (N_s, N_c, cases.SHAPES[(N_s, N_c)], lay, flag.tolist(), giter.tolist(), gpol.tolist()))
    assert flag.tolist() == [0] * P, (flag, giter)
    assert np.array_equal(gflag, flag) and np.abs(gx - line).max() <= 1e-12, np.abs(gx - line).max()
    cert = _certificate(H, g, A, lbA, ubA, line, lam)
    print("  certificate %s" % {k: float(np.max(v)) for k, v in cert.items() if k != "fval"})
    assert cert["max"].max() <= KKT_TOL, cert
    for p, kind in enumerate(kinds):
        ref = cases.oracle_cells(orc, otrack, N_s, N_c, kind)
        assert ref["flag"] == 0
        f = ccn.objective(H, g, line[p])
        ferr = abs(f - ref["fval"]) / abs(ref["fval"])
        both = gpol[p] > 0 and ref["polished"] > 0
        xerr = np.abs(line[p] - ref["x"]).max() / max(1.0, np.abs(ref["x"]).max())
        print("  plan %d (%s): f %.6f, oracle %.6f (rel %.2e), |c - oracle| rel %.2e, both at the vertex %s, max |n| %.3f"
              % (p, kind, f, ref["fval"], ferr, xerr, both, np.abs(ccn.apply(line[p], N_s)).max()))
        assert ferr <= FVAL_TOL, (kind, f, ref["fval"])
        assert xerr <= (X_TOL_VERTEX if both else X_TOL), (kind, xerr, both)


# ---- 3. the feature does something -------------------------------------------------------------------------------------------------
def test_3_cell_rows_use_the_wide_cells(fm, torch_, orc, otrack, tr):
    torch = torch_
    L, N_s, N_c = tr.L, 64, 16
    H, g = _host(torch, *fm.raceline_qp(tr, N_s, N_c))
    w = cases.N_MAX - MARGIN
    res = {}
    for kind in ("kappa", "constant"):
        cor = fm.Corridor.from_table(*cases.corridor(orc, otrack, N_s, kind), L)
        for rows in ("cells", "points"):
            plan = fm.Plan.raceline(fm.DYNAMIC, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor, rows=rows)
            o = _outputs(torch, plan)
            assert o["flag"].tolist() == [0] and np.isfinite(o["table"]).all()
            res[kind, rows] = (o["table"][0, :, 0], ccn.objective(H, g, o["line"][0]), o["line"][0])
            print("%s, %s: f %.5f, max |n| %.3f, max |c| %.3f, lap %.3f s" % (kind, rows, res[kind, rows][1], np.abs(res[kind, rows][0]).max(),
                                                                             np.abs(o["line"][0]).max(), o["t"].sum()))
    n_c, f_c, _ = res["kappa", "cells"]
    n_p, f_p, _ = res["kappa", "points"]
    assert np.abs(n_p).max() <= w + ON_ROW
    assert np.abs(n_c).max() > w                                   # the oracle: 0.556
    assert f_c < f_p - 1e-3 * abs(f_p)                             # the oracle: -0.12399 against -0.10892
    n_c, f_c, _ = res["constant", "cells"]
    n_p, f_p, _ = res["constant", "points"]
    assert np.abs(n_c).max() <= w + ON_ROW and f_c <= f_p          # the oracle: -0.12282 against -0.10892


# ---- 4. a blocked side -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_s,N_c", cases.BLOCKED_GPU)
def test_4_blocked_side(fm, torch_, orc, otrack, tr, N_s, N_c):
    """n_lo = 0.1 over N_s / 10 cells: the centre line is outside the corridor, and there is no fallback to it."""
    torch = torch_
    lo, hi = cases.corridor(orc, otrack, N_s, "blocked")
    plan = fm.Plan.raceline(fm.KINEMATIC, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=fm.Corridor.from_table(lo, hi, tr.L), rows="cells")
    o = _outputs(torch, plan)
    n = o["table"][0, :, 0]
    stretch = cases.blocked_cells(N_s)
    print("blocked (%d, %d): flag %s, n in the stretch %s" % (N_s, N_c, o["flag"].tolist(), np.round(n[stretch], 6).tolist()))
    assert o["flag"].tolist() == [0]
    assert (n[stretch] >= 0.35 - ON_ROW).all(), n[stretch]
    assert np.isfinite(o["table"]).all() and np.isfinite(o["t"]).all() and np.isfinite(o["line"]).all()
    ref = cases.oracle_cells(orc, otrack, N_s, N_c, "blocked")
    assert np.abs(o["line"][0] - ref["x"]).max() <= X_TOL * max(1.0, np.abs(ref["x"]).max())


# ---- 5. a pinched plan in a batch --------------------------------------------------------------------------------------------------
def test_5_pinched_plan_fails_alone(fm, torch_, orc, otrack, tr):
    torch = torch_
    L, N_s, N_c = tr.L, 64, 16
    lo, hi = cases.corridor(orc, otrack, N_s, "kappa")
    tl = np.stack([lo, lo - 0.1, lo, lo - 0.2])
    th = np.stack([hi, hi + 0.1, hi, hi + 0.2])
    th[2, 21] = tl[2, 21] + 2 * MARGIN                             # plan 2: one cell with n_hi - n_lo <= 2 margin
    keep = [0, 1, 3]
    four = fm.Plan.raceline(fm.DYNAMIC, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=fm.Corridor.from_table(tl, th, L), rows="cells", want_row_lambda=True)
    three = fm.Plan.raceline(fm.DYNAMIC, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=fm.Corridor.from_table(tl[keep], th[keep], L), rows="cells",
                             want_row_lambda=True)
    a, b = _outputs(torch, four), _outputs(torch, three)
    a["row_lambda"], b["row_lambda"] = _host(torch, four.row_lambda, three.row_lambda)
    assert four.P == 4 and three.P == 3
    assert a["flag"].tolist() == [0, 0, -1, 0] and b["flag"].tolist() == [0, 0, 0]
    for k in ("line", "table", "t"):
        assert np.isnan(a[k][2]).all(), k
    for k in ("line", "flag", "table", "t", "row_lambda"):
        assert _same_bits(a[k][keep], b[k]), k
    assert np.isfinite(b["table"]).all()
    # the same QPs through the general entry: plan 2 is answered before the first iteration
    H, g, A, lbA, ubA = _qp(fm, torch, tr, four._corridor, N_s, N_c, 4)
    assert np.isnan(lbA[2, 21]) and np.isnan(ubA[2, 21]) and np.isfinite(np.delete(lbA, 2, axis=0)).all()
    free = torch.full((4, N_c), ccn.FREE, dtype=torch.float64, device="cuda")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    gen = fm.qp_solve_batch_device(dev(H)[None], dev(np.tile(g, (4, 1))), dev(A)[None], -free, free, dev(lbA), dev(ubA), shared_HA=True, n_slack=0)
    gflag, giter = _host(torch, gen["exitflag"], gen["iter"])
    assert gflag.tolist() == [0, 0, -1, 0] and giter[2] == 0 and (np.delete(giter, 2) > 0).all(), (gflag, giter)


# ---- 6. the profile and the multipliers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1])
def test_6_profile_and_multipliers(fm, torch_, orc, otrack, tr, model):
    torch = torch_
    L, N_s, N_c = tr.L, 64, 16
    cor = fm.Corridor.from_table(*cases.corridor(orc, otrack, N_s, "kappa"), L)
    with_lam = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor, rows="cells", want_row_lambda=True)
    without = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor, rows="cells")
    a, b = _outputs(torch, with_lam), _outputs(torch, without)
    lam = _host(torch, with_lam.row_lambda)[0]
    assert without.row_lambda is None and lam.shape == (1, N_s)
    for k in ("line", "flag", "table", "t"):
        assert _same_bits(a[k], b[k]), k
    assert a["flag"].tolist() == [0]
    ref = rn.line_profile(model, cases.kappa(orc, otrack, N_s), otrack.L, a["line"][0], 20.0, 1.0)
    for col in range(8):
        assert relerr(a["table"][0][:, col], ref["table"][:, col]) <= BUILD_TOL, (model, "column", col, relerr(a["table"][0][:, col], ref["table"][:, col]))
    assert relerr(a["t"][0], ref["t"]) <= BUILD_TOL, (model, "t")
    # multipliers: non-zero only where the cell sits on its limit, with the sign of the side (the certificate's complementarity and sign)
    H, g, A, lbA, ubA = _qp(fm, torch, tr, cor, N_s, N_c, 1)
    cert = _certificate(H, g, A, lbA, ubA, a["line"], lam)
    assert cert["max"][0] <= KKT_TOL, cert
    n = a["table"][0, :, 0]
    on_lo, on_hi = np.abs(n - lbA[0]) <= 1e-6, np.abs(ubA[0] - n) <= 1e-6
    print("model %d: %d cells on n_lo, %d on n_hi, %d multipliers non-zero, %d above 1e-3" % (model, on_lo.sum(), on_hi.sum(), np.count_nonzero(lam[0]),
                                                                                              (np.abs(lam[0]) > 1e-3).sum()))
    big = np.abs(lam[0]) > 1e-3                                    # (complementarity <= 1e-6 puts these within 1e-3 of their limit)
    assert big.sum() >= 1 and (np.where(lam[0] > 0, n - lbA[0], ubA[0] - n)[big] <= 1e-3).all()


# ---- 7. the default path -----------------------------------------------------------------------------------------------------------
def test_7_default_path_is_the_point_form(fm, torch_, orc, otrack, tr):
    torch = torch_
    L, N_s, N_c = tr.L, 64, 16
    cor = fm.Corridor.from_table(*cases.corridor(orc, otrack, N_s, "kappa"), L)
    for model in (0, 1):
        default = _outputs(torch, fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor))
        points = _outputs(torch, fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN, corridor=cor, rows="points"))
        # fsaempc_plan_raceline_batch_device_c itself
        xP, yP = tr.device(torch.device("cuda:0"))
        P = lambda t: C.c_void_p(t.data_ptr())
        sp = fm._lib.Spline(tr.M, tr.dl, P(xP), P(yP))
        need = fm.lib().fsaempc_plan_raceline_workspace_bytes(1, N_c)
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
        line, table, t = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((1, N_c), (1, N_s, 8), (1, N_s)))
        flag = torch.empty(1, dtype=torch.int32, device="cuda")
        opts = fm.default_opts()
        rc = fm.lib().fsaempc_plan_raceline_batch_device_c(model, C.byref(sp), C.c_double(L), None, cor.ref(), 1, N_s, N_c, C.c_double(MARGIN), C.c_double(20.0),
                                                           C.c_double(1.0), C.byref(opts), P(line), P(flag), P(table), P(t), P(ws), C.c_longlong(ws.numel() * 8), None)
        assert rc == 0, fm.lib().fsaempc_last_error()
        direct = dict(zip(("line", "flag", "table", "t"), _host(torch, line, flag, table, t)))
        for k in ("line", "flag", "table", "t"):
            assert _same_bits(default[k], points[k]) and _same_bits(default[k], direct[k]), (model, k)
        assert default["flag"].tolist() == [0]
        # and without a corridor rows="points" is Plan.raceline as it always was
        plain = _outputs(torch, fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN))
        plain_p = _outputs(torch, fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=MARGIN, rows="points"))
        for k in ("line", "flag", "table", "t"):
            assert _same_bits(plain[k], plain_p[k]), (model, k)
