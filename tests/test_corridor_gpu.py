"""GPU tests of the s-varying track corridors: the track rows of the LTV build (A), the fused step (B), the closed loop
and its lap report (C), the racing line (D) and the refusals of the C entries.  The numpy side is tests/corridor_numpy.py; tolerances
are the project's own (tests/test_gpu_parity.py, tests/test_raceline_gpu.py, tests/test_lap_report_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
from conftest import relerr

import corridor_numpy as cn
import lap_numpy as ln
import raceline_numpy as rn
from kkt_numpy import kkt_certificate

pytestmark = pytest.mark.gpu

DT, SEED, B = 0.05, 31, 16
BUILD_TOL = 1e-9        # the project's construction tolerance
KKT_TOL = 1e-6          # the tolerances of tests/test_gpu_parity.py
FVAL_TOL = 1e-6
X_TOL = 5e-3
X_TOL_VERTEX = 1e-6
LINE_TOL = 1e-6         # tests/test_raceline_gpu.py
N_W = 200
QP = ("H", "g", "A", "lb", "ub", "lbA", "ubA")
QP_KEYS = QP + ("pred", "Bt", "const")
STEP_KEYS = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")
I = ln.IDX


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _np(torch, d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _inputs(torch, inp):
    x0, xl, ul, xr = inp
    return _dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul)


def corridor_tables(L, cap=0.1):
    """The corridor of tests A and B: 200 cells, n_hi = min(0.75 + 0.75 sin^2(3 pi s / L), cap), n_lo = -(0.75 + 0.5 sin^2(2 pi s / L + 0.7));
    cap = None: no cap."""
    s = np.arange(N_W) * L / N_W
    hi = 0.75 + 0.75 * np.sin(3 * np.pi * s / L) ** 2
    if cap is not None:
        hi = np.minimum(hi, cap)
    lo = -(0.75 + 0.5 * np.sin(2 * np.pi * s / L + 0.7) ** 2)
    return lo, hi


def lookup_case_instances(fm, model, N, L):
    """instances(model, N, 0.05, L, 31, range(16)) with the s column of the first four linearisation points rewritten to the lookup's
    cases: exactly on a cell, in the last cell (the wrap to cell 0), negative, past L."""
    x0, xl, ul, xr = fm.instances(model, N, DT, L, SEED, range(B))
    xl = xl.copy()
    ds = L / N_W
    k = np.arange(N)
    xl[0, :, 0] = (37 + k) * ds
    xl[1, :, 0] = (N_W - 1) * ds + ds * (0.05 + 0.9 * k / N)
    xl[2, :, 0] = xl[2, :, 0] - 2 * L
    xl[3, :, 0] = xl[3, :, 0] + L
    assert (xl[2, :, 0] < 0).all() and (xl[3, :, 0] > L).all()
    return x0, xl, ul, xr


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- A. the build ------------------------------------------------------------------------------------------------------------------
SHAPES_A = [(0, 5, None, False), (1, 5, None, False), (0, 8, [1, 2, 5], True)]


@pytest.mark.parametrize("model,N,lens,with_block", SHAPES_A)
def test_a_track_rows_of_the_build(fm, torch_, orc, otrack, tr, model, N, lens, with_block):
    torch = torch_
    L = tr.L
    inp = lookup_case_instances(fm, model, N, L)
    x0, xl, ul, xr = inp
    P = fm.default_params(model) if with_block else None
    lo, hi = corridor_tables(L)
    ds = L / N_W
    base = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens).build_qp(*_inputs(torch, inp)))
    tables = {"shared": (lo, hi), "per instance": (np.tile(lo, (B, 1)), np.tile(hi, (B, 1)) + 0.01 * np.arange(B)[:, None])}
    # the oracle's rows for every shape: move blocking leaves the rows' bounds as they are (tests/block_numpy.py::block_qp), and the
    # parameter block of the third shape holds the defaults the oracle has compiled in
    oq = orc.build_qp_batch(model, otrack, N, DT, x0, xr, xl, ul)
    for name, (tl, th) in tables.items():
        cor = fm.Corridor.from_table(tl, th, L)
        assert cor.P == (1 if name == "shared" else B)
        q = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens, corridor=cor).build_qp(*_inputs(torch, inp)))
        rows_l, rows_u = slice(2 * N, 3 * N), slice(3 * N, 4 * N)
        for k in QP_KEYS:
            a, b = q[k].copy(), base[k].copy()
            if k == "lbA":
                a[:, rows_l] = 0; b[:, rows_l] = 0
            if k == "ubA":
                a[:, rows_u] = 0; b[:, rows_u] = 0
            assert _same_bits(a, b), (name, k)                                  # everything else: the bits of the _b / _p build
        pred_n = q["pred"].reshape(B, N, -1)[:, :, 1]
        for b in range(B):
            bl, bh = (tl, th) if name == "shared" else (tl[b], th[b])
            wl, wu = cn.row_bounds(bl, bh, ds, xl[b, :, 0], pred_n[b])
            el, eu = np.abs(q["lbA"][b, rows_l] - wl).max(), np.abs(q["ubA"][b, rows_u] - wu).max()
            assert el <= BUILD_TOL and eu <= BUILD_TOL, (name, b, el, eu)
            l_, h_ = cn.limits(bl, bh, ds, xl[b, :, 0])      # the oracle's rows are +-0.75 - pred: move them to the corridor's limits
            el, eu = np.abs(q["lbA"][b, rows_l] - (oq["lbA"][b, rows_l] + 0.75 + l_)).max(), np.abs(q["ubA"][b, rows_u] - (oq["ubA"][b, rows_u] - 0.75 + h_)).max()
            assert el <= BUILD_TOL and eu <= BUILD_TOL, (name, "oracle", b, el, eu)
        assert (q["ubA"][:, rows_l] == 1e10).all() and (q["lbA"][:, rows_u] == -1e10).all()      # the fillers of the other sides stay
        assert np.abs(q["ubA"][:, rows_u] - base["ubA"][:, rows_u]).max() > 0.5                     # (the corridor is not the constant one)
    # a constant corridor +-0.75: the bits of the build without one, in every output
    q = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens, corridor=fm.Corridor.constant(L, 0.75)).build_qp(*_inputs(torch, inp)))
    for k in QP_KEYS:
        assert _same_bits(q[k], base[k]), ("constant", k)
    # A NaN s in step 2 of one instance.  The build itself carries that NaN on (the step is linearised there, so pred is NaN from step 2 on):
    # outside the 2N rows the bits are those of the build without a corridor on the same input; inside them the two entries of step 2 are
    # NaN and the NaN pattern is the restatement's on the device's own pred; every other instance is finite.
    xl2 = xl.copy(); xl2[5, 2, 0] = np.nan
    inp2 = (x0, xl2, ul, xr)
    cor = fm.Corridor.from_table(lo, hi, L)
    qn = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens, corridor=cor).build_qp(*_inputs(torch, inp2)))
    bn_ = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens).build_qp(*_inputs(torch, inp2)))
    pred_n = qn["pred"].reshape(B, N, -1)[:, :, 1]
    for k, rows, side in (("lbA", slice(2 * N, 3 * N), 0), ("ubA", slice(3 * N, 4 * N), 1)):
        x, y = qn[k].copy(), bn_[k].copy()
        x[:, rows] = 0; y[:, rows] = 0
        assert _same_bits(x, y), k
        assert np.isnan(qn[k][5, rows][2])
        want = np.stack([cn.row_bounds(lo, hi, ds, xl2[b, :, 0], pred_n[b])[side] for b in range(B)])
        assert np.array_equal(np.isnan(qn[k][:, rows]), np.isnan(want)), k
        assert np.isfinite(np.delete(qn[k][:, rows], 5, axis=0)).all()
    for k in QP_KEYS:
        if k not in ("lbA", "ubA"):
            assert _same_bits(qn[k], bn_[k]), k
    # Cells where n_lo < n_hi does not hold (a table that did not go through Corridor.from_table's validation): NaN in the rows whose
    # lookup reads such a cell and nowhere else.  Instance 0 sits exactly on the cells 37 + k.
    lo_t, hi_t = _dev(torch, lo[None]), _dev(torch, hi[None])
    hi_t[0, 39] = lo_t[0, 39]
    hi_bad = hi.copy(); hi_bad[39] = lo[39]
    qb = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens, corridor=fm.Corridor(lo_t, hi_t, L)).build_qp(*_inputs(torch, inp)))
    pred_n = qb["pred"].reshape(B, N, -1)[:, :, 1]
    for k, rows, side in (("lbA", slice(2 * N, 3 * N), 0), ("ubA", slice(3 * N, 4 * N), 1)):
        want = np.stack([cn.row_bounds(lo, hi_bad, ds, xl[b, :, 0], pred_n[b])[side] for b in range(B)])
        assert np.array_equal(np.isnan(qb[k][:, rows]), np.isnan(want)), k
        assert 2 <= np.isnan(want[0]).sum() <= 3 and np.isnan(want[0, 1:3]).all(), want[0]
        fin = np.isfinite(want)
        assert np.abs(qb[k][:, rows][fin] - want[fin]).max() <= BUILD_TOL
        x, y = qb[k].copy(), base[k].copy()
        x[:, rows] = 0; y[:, rows] = 0
        assert _same_bits(x, y), k


# ---- B. the fused step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [(0, 10), (1, 10)])
def test_b_fused_step_in_the_corridor(fm, torch_, orc, otrack, tr, model, N):
    torch = torch_
    L = tr.L
    inp = lookup_case_instances(fm, model, N, L)
    x0, xl, ul, xr = inp
    ns = 1 if model == 0 else 4
    lo, hi = corridor_tables(L)
    ds = L / N_W
    cor = fm.Corridor.from_table(lo, hi, L)
    mpc = fm.LtvBatch(model, N, DT, tr, B, corridor=cor)
    q = _np(torch, mpc.build_qp(*_inputs(torch, inp)))
    out = _np(torch, mpc.step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    plain = _np(torch, fm.LtvBatch(model, N, DT, tr, B).step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    assert (out["exitflag"] == 0).all(), out["exitflag"]
    z = np.concatenate([out["u_opt"], out["slack"]], axis=1)
    c = kkt_certificate(*[q[k] for k in QP], z, out["lam"])
    print("corridor step", model, N, "certificate max", c["max"].max(), "iter mean", out["iter"].mean())
    assert c["max"].max() <= KKT_TOL, {k: float(np.max(c[k])) for k in ("stationarity", "primal", "sign", "complementarity")}
    # the oracle on its own QP with the restated bounds
    oq = orc.build_qp_batch(model, otrack, N, DT, x0, xr, xl, ul)
    l_, h_ = cn.limits(lo, hi, ds, xl[:, :, 0])
    lbA, ubA = oq["lbA"].copy(), oq["ubA"].copy()
    lbA[:, 2 * N:3 * N] = oq["lbA"][:, 2 * N:3 * N] + 0.75 + l_
    ubA[:, 3 * N:4 * N] = oq["ubA"][:, 3 * N:4 * N] - 0.75 + h_
    ref = orc.qp_solve_batch_aux(oq["H"], oq["g"], oq["A"], oq["lb"], oq["ub"], lbA, ubA)
    assert (ref["exitflag"] == 0).all(), ref["exitflag"]
    fo = ref["fval"] + oq["const"]
    ferr = np.abs(out["fval"] - fo) / np.maximum(1.0, np.abs(fo))
    both = (out["polished"] > 0) & (ref["polished"] > 0)
    uerr = np.abs(out["u_opt"] - ref["x"][:, : 2 * N]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"][:, : 2 * N]).max(axis=1))
    print("  fval err max %.3e, u err max %.3e, both at the vertex %d of %d" % (ferr.max(), uerr.max(), both.sum(), B))
    assert (ferr <= FVAL_TOL).all(), ferr
    assert (uerr <= np.where(both, X_TOL_VERTEX, X_TOL)).all(), (uerr, both)
    # the plan respects the left edge up to the track slack
    n_k = out["x_opt"].reshape(B, N, -1)[:, :, 1]
    assert (n_k <= h_ + out["slack"][:, :1] + 1e-6).all(), float((n_k - h_ - out["slack"][:, :1]).max())
    # the feature acts
    moved = np.abs(out["u_opt"] - plain["u_opt"]).max(axis=1) > 1e-3
    print("  instances moved by the corridor:", int(moved.sum()))
    assert moved.sum() >= 6, moved
    # the constant corridor is the step without one, bit for bit
    const = _np(torch, fm.LtvBatch(model, N, DT, tr, B, corridor=fm.Corridor.constant(L, 0.75)).step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    for k in STEP_KEYS + ("kkt", "polished", "lam"):
        assert _same_bits(const[k], plain[k]), k
    # per-instance corridors are isolated: changing car 3's table leaves every other car's outputs as they were
    tl, th = np.tile(lo, (B, 1)), np.tile(hi, (B, 1))
    a = _np(torch, fm.LtvBatch(model, N, DT, tr, B, corridor=fm.Corridor.from_table(tl, th, L)).step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    th2 = th.copy(); th2[3] = -0.5                                             # (left of where car 3 drives: its plan must move)
    b = _np(torch, fm.LtvBatch(model, N, DT, tr, B, corridor=fm.Corridor.from_table(tl, th2, L)).step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    others = np.delete(np.arange(B), 3)
    for k in STEP_KEYS:
        assert _same_bits(a[k][others], b[k][others]), k
        assert _same_bits(a[k], out[k]), k                                     # (and B copies of the table are the shared table)
    assert abs(a["fval"][3] - b["fval"][3]) > 1e-6 * max(1.0, abs(a["fval"][3]))   # (the inputs may sit on their bounds in both: the cost tells)


def test_b_nan_limit_fails_one_instance_only(fm, torch_, tr):
    """A NaN linearisation s gives NaN track rows for that instance: the solve answers -1 with iter = 0, the neighbours are unaffected."""
    torch = torch_
    model, N = 0, 10
    x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, SEED, range(B))
    lo, hi = corridor_tables(tr.L)
    mpc = fm.LtvBatch(model, N, DT, tr, B, corridor=fm.Corridor.from_table(lo, hi, tr.L))
    good = _np(torch, mpc.step(*_inputs(torch, (x0, xl, ul, xr))))
    xl2 = xl.copy(); xl2[5, 2, 0] = np.nan
    out = _np(torch, mpc.step(*_inputs(torch, (x0, xl2, ul, xr))))
    assert out["exitflag"][5] == -1 and out["iter"][5] == 0
    others = np.delete(np.arange(B), 5)
    for k in STEP_KEYS:
        assert _same_bits(out[k][others], good[k][others]), k


# ---- C. the closed loop and the report --------------------------------------------------------------------------------------------
def _pinched(L):
    """+-0.75 with n_hi = 0.1 over the first 40 m"""
    s = np.arange(N_W) * L / N_W
    hi = np.where(s < 40.0, 0.1, 0.75)
    return np.full(N_W, -0.75), hi


def _run(fm, torch, tr, model, N, cart, s0, v0, steps, **kw):
    """tests/test_lap_report_gpu.py::_run: the loop with the metrics kernel's inputs of every step read back at the end"""
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    keep = dict(x0=[], finished=[], flag=[], iter=[], fval=[], slack=[], a=[], cart=[])
    for t in range(steps):
        out = cl.step()
        for k, v in (("x0", cl.x0), ("finished", cl.finished), ("flag", out["exitflag"]), ("iter", out["iter"]), ("fval", out["fval"]),
                     ("slack", out["slack"]), ("a", cl.u_opt[:, 0, 0]), ("cart", cl.cart)):
            keep[k].append(v.clone())
    torch.cuda.synchronize(cl.device)
    h = {k: torch.stack(v).cpu().numpy() for k, v in keep.items()}
    h["slack"] = h["slack"].reshape(steps, cl.B, -1)
    return cl, h


def _records_in_corridor(h, lo, hi, ds):
    """tests/lap_numpy.py's records with the two track-violation slots restated against the corridor: the n list of a car is what
    main.m:101 collects (every step up to and including the one that ends the lap, none of a lost car's)."""
    want = ln.records(h, DT, 1e-6)
    T, nb = h["finished"].shape
    for b in range(nb):
        vs = []
        for t in range(T):
            fin = int(h["finished"][t, b])
            if fin == 2:
                break
            vs.append(float(cn.violation(lo, hi, ds, h["x0"][t, b, 0], h["x0"][t, b, 1])))
            if fin == 1:
                break
        vs = [v for v in vs if v > 0.0]
        want[b, I["N_VIOL_INT"]] = sum(v * DT for v in vs)
        want[b, I["N_VIOL_MAX"]] = max(vs) if vs else 0.0
    return want


@pytest.mark.parametrize("blocked", [False, True])
def test_c_closed_loop_and_report(fm, torch_, tr, otrack, blocked):
    """Kinematic N = 10, 16 cars, 30 steps.  The cars are the five of tests/lap_numpy.py tiled (s0 = 20 m but for the one near the end of the
    lap): "off-line" starts at n = 0.9 and "centre" on the centre line; inside the pinch (n_hi = 0.1 for s < 40) the off-line cars start
    0.8 m outside the corridor, so their N_VIOL_INT is positive and larger than against +-0.75."""
    torch = torch_
    cart, s0, v0, kind = ln.cars(otrack, B)
    lo, hi = _pinched(tr.L)
    ds = tr.L / N_W
    kw = dict(blocking=[1, 1, 2, 2, 4], reference=fm.Plan.profile(fm.KINEMATIC, tr, N_s=200)) if blocked else {}
    cor = fm.Corridor.from_table(lo, hi, tr.L)
    cl, h = _run(fm, torch, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True, corridor=cor, **kw)
    m = cl.metrics.cpu().numpy()
    print("C: worst deviation of a sum", ln.compare(m, _records_in_corridor(h, lo, hi, ds), 1e-10))
    for b in range(B):
        name = ln.CAR_NAMES[kind[b]]
        if name == "off-line":                             # the cars that start with n > 0.1 (tests/lap_numpy.py drives no corridor on the oracle)
            assert m[b, I["N_VIOL_INT"]] > 0, (b, name)
            assert m[b, I["N_VIOL_MAX"]] >= 0.79 and m[b, I["N_ABS_MAX"]] >= 0.89, b
        if name == "lost":
            assert m[b, I["STATUS"]] == 2 and m[b, I["N_VIOL_INT"]] == 0, b
    # without a corridor: the loop and the report as they are; the constant corridor gives the same bits
    none, h0 = _run(fm, torch, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True, **kw)
    const, h1 = _run(fm, torch, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True, corridor=fm.Corridor.constant(tr.L, 0.75), **kw)
    m0 = none.metrics.cpu().numpy()
    ln.compare(m0, ln.records(h0, DT, 1e-6), 1e-10)
    assert _same_bits(const.metrics.cpu().numpy(), m0)
    for k in h0:
        assert _same_bits(h0[k], h1[k]), k
    off = [b for b in range(B) if ln.CAR_NAMES[kind[b]] == "off-line"]
    assert (m[off, I["N_VIOL_INT"]] > m0[off, I["N_VIOL_INT"]]).all()


# ---- D. the racing line ------------------------------------------------------------------------------------------------------------
def _line_corridor(L):
    lo, hi = corridor_tables(L, cap=None)
    s = np.arange(N_W) * L / N_W
    hi = hi.copy(); hi[(s > 100.0) & (s < 115.0)] = 0.3
    return lo, hi


def test_d_racing_line_in_the_corridor(fm, torch_, orc, otrack, tr):
    torch = torch_
    L, N_s, N_c, margin = tr.L, 64, 16, 0.25
    lo, hi = _line_corridor(L)
    ds = L / N_W
    lb, ub = cn.control_point_bounds(lo, hi, ds, L, N_s, N_c, margin)
    assert (ub - lb).min() >= 0.55
    H, g = (a.cpu().numpy() for a in fm.raceline_qp(tr, N_s, N_c))
    xo, fo, flo, ito, lamo = orc.qp_solve(H, g, np.zeros((0, N_c)), lb, ub, np.zeros(0), np.zeros(0))
    assert flo == 0
    cor = fm.Corridor.from_table(lo, hi, L)
    s_cells = np.arange(N_s) * L / N_s
    l_, h_ = cn.limits(lo, hi, ds, s_cells)
    for model in (0, 1):
        plan = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=margin, corridor=cor)
        torch.cuda.synchronize()
        got_lb, got_ub = (v.cpu().numpy()[0] for v in cor.line_bounds(N_s, N_c, margin))    # the bounds the call hands to the solve
        assert np.abs(got_lb - lb).max() <= 1e-14 and np.abs(got_ub - ub).max() <= 1e-14, (np.abs(got_lb - lb).max(), np.abs(got_ub - ub).max())
        assert int(plan.line_flag[0]) == 0
        c = plan.line.cpu().numpy()[0]
        print("model %d: max |line - oracle| %.3e m, on a bound %d of %d" % (model, np.abs(c - xo).max(), int(((c <= lb + 1e-9) | (c >= ub - 1e-9)).sum()), N_c))
        assert np.abs(c - xo).max() <= LINE_TOL
        lam = rn.multipliers(H, g, got_lb, got_ub, c)
        cert = kkt_certificate(H[None], g[None], np.zeros((1, N_c, 0)), got_lb[None], got_ub[None], np.zeros((1, 0)), np.zeros((1, 0)), c[None], lam[None])
        assert cert["max"][0] <= KKT_TOL, cert
        n = plan.table.cpu().numpy()[0, :, 0]
        assert (n >= l_ + margin - 1e-9).all() and (n <= h_ - margin + 1e-9).all()
        # a constant corridor +-0.75 is Plan.raceline(margin = 0.25)
        a = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=margin)
        b = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=margin, corridor=fm.Corridor.constant(L, 0.75))
        torch.cuda.synchronize()
        for x, y in ((a.line, b.line), (a.table, b.table), (a.t, b.t)):
            assert _same_bits(x.cpu().numpy(), y.cpu().numpy())
        # two plans, the second one's corridor narrower than 2 margin in one cell: NaN throughout, plan 1 as in the one-plan run
        hi2 = hi.copy(); hi2[58:63] = lo[58:63] + 0.4                             # (five cells of the table: the plan's cell at s = 19 L / 64 reads two of them)
        assert np.isnan(cn.control_point_bounds(lo, hi2, ds, L, N_s, N_c, margin)[0]).sum() == 0 and \
            (np.subtract(*cn.control_point_bounds(lo, hi2, ds, L, N_s, N_c, margin)) >= 0).any()
        two = fm.Plan.raceline(model, tr, N_s=N_s, N_c=N_c, margin=margin, corridor=fm.Corridor.from_table(np.stack([lo, lo]), np.stack([hi, hi2]), L))
        torch.cuda.synchronize()
        assert two.P == 2
        for x, y in ((two.line, plan.line), (two.table, plan.table), (two.t, plan.t)):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            assert _same_bits(x[0], y[0]) and np.isnan(x[1]).all()
        # its QP is not solved (NaN bounds where a control point has no box: flag -1), and exactly those control points have no box
        assert two.line_flag.cpu().numpy().tolist() == [0, -1]
        lb2, ub2 = (v.cpu().numpy() for v in two._corridor.line_bounds(N_s, N_c, margin))
        wl2, wu2 = cn.control_point_bounds(lo, hi2, ds, L, N_s, N_c, margin)
        assert np.array_equal(lb2[0], got_lb) and np.array_equal(ub2[0], got_ub)
        assert np.array_equal(np.isnan(lb2[1]), wl2 >= wu2) and np.array_equal(np.isnan(ub2[1]), wl2 >= wu2) and 0 < (wl2 >= wu2).sum() < N_c
        ok = wl2 < wu2
        assert np.abs(lb2[1][ok] - wl2[ok]).max() <= 1e-14 and np.abs(ub2[1][ok] - wu2[ok]).max() <= 1e-14


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_corridors_are_refused_before_a_launch(fm, torch_, tr):
    """Every FSAEMPC_ERR_ARG case of every entry, straight through the C ABI with otherwise valid arguments and real buffers: the entry
    returns -1, fsaempc_last_error names the argument, and every output buffer, filled with a sentinel beforehand, is untouched."""
    torch = torch_
    model, N, nb = 0, 5, 4
    mpc = fm.LtvBatch(model, N, DT, tr, nb)
    nx, nV, nC = mpc.nx, mpc.nV, mpc.nC
    x0, xr, xl, ul = _inputs(torch, fm.instances(model, N, DT, tr.L, SEED, range(nb)))
    good = fm.Corridor.constant(tr.L, 0.75)
    ptr = good.c.n_lo
    SENT = -12345.0
    f64 = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device="cuda")
    i32 = lambda *shape: torch.full(shape, -777, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    L_ = fm.lib()
    need = L_.fsaempc_ltv_workspace_bytes(C.byref(mpc.desc))
    n_plans, N_s, N_c = 1, 64, 16
    need_line = L_.fsaempc_plan_raceline_workspace_bytes(n_plans, N_c)
    opts = fm.default_opts()
    cases = [((None, ptr, 2, 1.0), "n_lo"), ((ptr, None, 2, 1.0), "n_hi"), ((ptr, ptr, 1, 1.0), "N_w"), ((ptr, ptr, 2, 0.0), "ds"),
             ((ptr, ptr, 2, -1.0), "ds"), ((ptr, ptr, 2, float("nan")), "ds"), ((ptr, ptr, 2, float("inf")), "ds")]
    for (lo, hi, Nw, ds), word in cases:
        cor = fm._lib.CorridorTable(lo, hi, Nw, ds, 0)
        outs = dict(H=f64(nb, nV, nV), g=f64(nb, nV), A=f64(nb, nV, nC), lb=f64(nb, nV), ub=f64(nb, nV), lbA=f64(nb, nC), ubA=f64(nb, nC),
                    pred=f64(nb, N * nx), Bt=f64(nb, nV, N * nx), const=f64(nb),
                    u_opt=f64(nb, 2 * N), x_opt=f64(nb, N * nx), slack=f64(nb, 1), fval=f64(nb), ws=f64((need + 7) // 8),
                    metrics=f64(nb, 16), line=f64(n_plans, N_c), table=f64(n_plans, N_s, 8), t=f64(n_plans, N_s), ws_line=f64((need_line + 7) // 8),
                    blb=f64(n_plans, N_c), bub=f64(n_plans, N_c))
        ints = dict(exitflag=i32(nb), iter=i32(nb), flag=i32(n_plans))
        o = outs
        calls = {
            "build": lambda: L_.fsaempc_ltv_build_qp_batch_device_c(C.byref(mpc.desc), C.byref(mpc.sp), None, None, C.byref(cor), P(x0), P(xr), P(xl), P(ul),
                                                                    *[P(o[k]) for k in QP_KEYS], None),
            "step": lambda: L_.fsaempc_ltv_step_batch_device_c(C.byref(mpc.desc), C.byref(mpc.sp), None, None, C.byref(cor), P(x0), P(xr), P(xl), P(ul),
                                                               C.byref(opts), P(o["u_opt"]), P(o["x_opt"]), P(o["slack"]), P(o["fval"]), P(ints["exitflag"]),
                                                               P(ints["iter"]), None, None, P(o["ws"]), C.c_longlong(o["ws"].numel() * 8), None),
            "metrics": lambda: L_.fsaempc_cl_metrics_batch_device_c(model, N, DT, 1e-6, nb, None, C.byref(cor), P(x0), P(i32(nb)), P(i32(nb)), P(i32(nb)),
                                                                     P(f64(nb)), P(f64(nb, 1)), P(ul), P(f64(nb, 7)), P(o["metrics"]), None),
            "raceline": lambda: L_.fsaempc_plan_raceline_batch_device_c(model, C.byref(mpc.sp), C.c_double(tr.L), None, C.byref(cor), n_plans, N_s, N_c,
                                                                         0.25, 20.0, 1.0, C.byref(opts), P(o["line"]), P(ints["flag"]), P(o["table"]),
                                                                         P(o["t"]), P(o["ws_line"]), C.c_longlong(o["ws_line"].numel() * 8), None),
            "line bounds": lambda: L_.fsaempc_corridor_line_bounds_device(C.byref(cor), C.c_double(tr.L), n_plans, N_s, N_c, 0.25, P(o["blb"]), P(o["bub"]), None),
        }
        for name, call in calls.items():
            assert call() == -1, (name, word)
            msg = L_.fsaempc_last_error().decode()
            assert "corridor" in msg and word in msg, (name, word, msg)
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert bool((v == SENT).all()), (word, k)
        for k, v in ints.items():
            assert bool((v == -777).all()), (word, k)
    # the same calls with the good corridor go through: the sentinel check above can see a launch
    cor = good.c
    assert calls["build"]() == 0 and calls["line bounds"]() == 0
    torch.cuda.synchronize()
    assert not bool((outs["lbA"] == SENT).any()) and not bool((outs["blb"] == SENT).any())
