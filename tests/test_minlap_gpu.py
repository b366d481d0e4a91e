"""GPU tests of the minimum-time racing line: lap time and gradient of plan_line_lapgrad_kernel against the numpy
restatement (tests/minlap_numpy.py) on the fixtures tests/test_minlap_cpu.py vets, T against the line-profile entry's sum of t, the
isolation of a plan inside a batch and of NaN plans, one iteration and the loop of fsaempc_plan_minlap_batch_device against the
restated iteration with the oracle's solver, K = 0 against Plan.raceline bit for bit, corridor boxes, and the closed-loop wiring.

What "the lap of Plan.raceline, bitwise" means here: a Plan carries no lap time of its own, its lap is a sum of t that the caller
forms.  The loop test therefore compares lap_history[:, 0] bit for bit with Plan.lap_gradient on Plan.raceline's control points (the
same kernel on the same line) and to 1e-12 relative with the sum of Plan.raceline's t."""
import numpy as np
import pytest

import minlap_cases as mc
import minlap_numpy as mn
import raceline_numpy as rn

pytestmark = pytest.mark.gpu

BUILD_TOL = 1e-9      # the project's construction tolerance; test_minlap_cpu.py::test_gradient_conditioning: a 1e-13 input difference stays below 1e-11
SUM_TOL = 1e-12       # T against the sum of the line-profile entry's t: the rounding of two orders of one sum of N_s <= 500 terms
CAND_TOL = 1e-6       # candidates' T against the restatement's, relative: their lines come from two solvers
LINE_TOL = 1e-9       # m, the new line against the restatement's (two solvers on one QP; measured 1.4e-14 m, most control points end on the box)


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


def _tracks(fm, orc, name):
    return fm.Track.load(name), orc.Track.load(fm.tracks._HERE + "/tracks/%s.json" % name)


def _np(*a):
    out = tuple(x.cpu().numpy() for x in a)
    return out if len(out) > 1 else out[0]


def _bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", mc.GRAD_CASES, ids=str)
def test_lap_gradient_parity(fm, orc, case):
    name, model, N_s, N_c, v_cap, grip = case
    tr, otr = _tracks(fm, orc, name)
    c = np.array(mc.line(orc, otr, case))      # (a writable copy: the fixture's own array is read-only)
    ref = mc.restated(orc, otr, case)
    T, g = _np(*fm.Plan.lap_gradient(model, tr, c, N_s=N_s, v_cap=v_cap, grip=grip))
    T2, g2 = _np(*fm.Plan.lap_gradient(model, tr, c, N_s=N_s, v_cap=v_cap, grip=grip))
    assert T.shape == (1,) and g.shape == (1, N_c) and _bits(T, T2) and _bits(g, g2)          # the same bits on every call
    t = _np(fm.Plan.profile(model, tr, N_s=N_s, v_cap=v_cap, grip=grip, line=c).t)[0]
    eT, eS, eg = abs(T[0] - ref["T"]) / ref["T"], abs(T[0] - t.sum()) / t.sum(), np.abs(g[0] - ref["grad"]).max() / np.abs(ref["grad"]).max()
    print("T rel %.2e, against the profile's sum %.2e, grad rel %.2e (max |grad| %.3e)" % (eT, eS, eg, np.abs(ref["grad"]).max()))
    assert eT <= BUILD_TOL and eS <= SUM_TOL and eg <= BUILD_TOL


@pytest.mark.parametrize("model", [0, 1])
def test_lap_gradient_with_blocks_and_in_a_batch_of_70(fm, orc, model):
    """RtPar: one block per plan (and one shared block), grips 1 and 0.8; a plan alone and inside a batch of 70 has the same bits; a bad
    block and a line that folds over a corner are NaN and their neighbours do not notice."""
    tr, otr = _tracks(fm, orc, "fss2019")
    N_s, N_c = 130, 32
    k, c0 = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c)
    blocks = fm.param_draws(model, range(70), 77, 0.2)
    lines = c0[None] * np.linspace(0.3, 1.0, 70)[:, None]
    for grip in (1.0, 0.8):
        T, g = _np(*fm.Plan.lap_gradient(model, tr, lines[:3], N_s=N_s, grip=grip, params=blocks[:3]))
        for p in range(3):
            ref = mn.lap_gradient(model, k, otr.L, lines[p], 20.0, grip, blocks[p])
            assert abs(T[p] - ref["T"]) / ref["T"] <= BUILD_TOL and np.abs(g[p] - ref["grad"]).max() <= BUILD_TOL * np.abs(ref["grad"]).max(), (grip, p)
    T1, g1 = _np(*fm.Plan.lap_gradient(model, tr, lines[5], N_s=N_s, params=blocks[5]))                  # one shared block, one plan
    T70, g70 = _np(*fm.Plan.lap_gradient(model, tr, lines, N_s=N_s, params=blocks))
    assert T70.shape == (70,) and _bits(T1[0], T70[5]) and _bits(g1[0], g70[5])
    assert np.isfinite(T70).all() and np.unique(T70).size == 70
    bad_blocks, bad_lines = blocks.copy(), lines.copy()
    bad_blocks[7, fm.PARAM_INDEX["M"]] = -1.0
    bad_lines[64] = 0.95 / np.abs(k).max() * np.sign(k[np.argmax(np.abs(k))])                            # a = 0.05 in the tightest cell
    Tb, gb = _np(*fm.Plan.lap_gradient(model, tr, bad_lines, N_s=N_s, params=bad_blocks))
    keep = np.ones(70, dtype=bool); keep[[7, 64]] = False
    assert np.isnan(Tb[~keep]).all() and np.isnan(gb[~keep]).all()
    assert _bits(Tb[keep], T70[keep]) and _bits(gb[keep], g70[keep])


@pytest.mark.parametrize("case", mc.STEP_CASES, ids=str)
def test_one_iteration_against_the_restatement(fm, orc, case):
    """From the oracle's minimum-curvature line: every candidate's T (one call per rho with a ladder of one: J = 1), the index taken
    with the whole ladder, and the new line."""
    name, model, N_s, N_c, v_cap, grip = case
    tr, otr = _tracks(fm, orc, name)
    k, c = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c)
    H, g = rn.qp(orc, otr, N_s, N_c)
    ref = mc.restated(orc, otr, case)
    lo, hi = np.full(N_c, -mc.W), np.full(N_c, mc.W)
    c1, g1, T1, pick, cands = mn.iterate(orc, model, k, otr.L, H, c, ref["grad"], ref["T"], lo, hi, mn.RHO_DEFAULT, v_cap, grip)
    kw = dict(N_s=N_s, N_c=N_c, margin=mc.MARGIN, v_cap=v_cap, grip=grip, c_init=c)
    for j, rho in enumerate(mn.RHO_DEFAULT):
        one = fm.Plan.minlap(model, tr, iters=1, rho=(rho,), **kw)
        lap, step = _np(one.lap_history, one.step_history)
        assert step[0, 0] == 0 and abs(lap[0, 1] - cands[j][0]["T"]) / cands[j][0]["T"] <= CAND_TOL, (j, lap, cands[j][0]["T"])
    plan = fm.Plan.minlap(model, tr, iters=1, **kw)
    lap, step, line = _np(plan.lap_history, plan.step_history, plan.control_points)
    print("T %.6f -> %.6f, rho index %d, max |line - restatement| %.2e m" % (lap[0, 0], lap[0, 1], step[0, 0], np.abs(line[0] - c1).max()))
    assert abs(lap[0, 0] - ref["T"]) / ref["T"] <= BUILD_TOL
    assert step[0, 0] == pick and abs(lap[0, 1] - T1) / T1 <= CAND_TOL
    assert (line[0] >= lo).all() and (line[0] <= hi).all() and np.abs(line[0] - c1).max() <= LINE_TOL
    assert int(plan.line_flag[0]) == 0 and lap[0, 0] - lap[0, 1] >= 0.05


@pytest.mark.parametrize("case", mc.STEP_CASES, ids=str)
def test_the_loop(fm, orc, case):
    name, model, N_s, N_c, v_cap, grip = case
    tr, otr = _tracks(fm, orc, name)
    kw = dict(N_s=N_s, N_c=N_c, margin=mc.MARGIN, v_cap=v_cap, grip=grip)
    race = fm.Plan.raceline(model, tr, **kw)
    plan = fm.Plan.minlap(model, tr, iters=3, **kw)
    lap, step, line = _np(plan.lap_history, plan.step_history, plan.control_points)
    assert lap.shape == (1, 4) and step.shape == (1, 3) and (np.diff(lap[0]) <= 0).all() and lap[0, -1] < lap[0, 0]
    assert all((s >= 0) == (b < a) for s, a, b in zip(step[0], lap[0, :-1], lap[0, 1:])) and step.max() < len(mn.RHO_DEFAULT)
    T0 = _np(fm.Plan.lap_gradient(model, tr, race.line, N_s=N_s, v_cap=v_cap, grip=grip)[0])
    assert _bits(lap[:, 0], T0) and abs(lap[0, 0] - race.lap_time()[0]) <= SUM_TOL * lap[0, 0]
    assert _bits(_np(plan.line_flag), _np(race.line_flag)) and (np.abs(line) <= mc.W).all()
    own = fm.Plan.profile(model, tr, N_s=N_s, v_cap=v_cap, grip=grip, line=line)
    assert _bits(_np(plan.table), _np(own.table)) and _bits(_np(plan.t), _np(own.t))
    assert abs(_np(plan.t).sum() - lap[0, -1]) <= SUM_TOL * lap[0, -1]
    # the restated loop from the device's own start, with the oracle's solver: the same history while no selection ties
    H, g = rn.qp(orc, otr, N_s, N_c)
    c3, lap_n, step_n = mn.loop(orc, model, mc.kappa(orc, otr, N_s), otr.L, H, _np(race.line)[0], np.full(N_c, -mc.W), np.full(N_c, mc.W), 3, mn.RHO_DEFAULT, v_cap, grip)
    print("device %s %s, restated %s %s" % (lap[0], step[0], lap_n, step_n))
    assert np.abs(lap[0] - lap_n).max() <= CAND_TOL * lap_n[0]


@pytest.mark.parametrize("model", [0, 1])
def test_no_iterations_is_the_raceline_entry(fm, model):
    tr = fm.Track.load("fss2019")
    blocks = fm.param_draws(model, range(3), 77, 0.2)
    for kw in (dict(N_s=128, N_c=32), dict(N_s=37, N_c=9, grip=0.8), dict(N_s=130, N_c=32, params=blocks)):
        a, b = fm.Plan.raceline(model, tr, **kw), fm.Plan.minlap(model, tr, iters=0, **kw)
        for x, y in ((a.table, b.table), (a.t, b.t), (a.line, b.line), (a.line_flag, b.line_flag)):
            assert _bits(_np(x), _np(y)), kw
        assert tuple(b.lap_history.shape) == (a.P, 1) and tuple(b.step_history.shape) == (a.P, 0)
    c = 0.3 * np.sin(np.arange(32) * 0.7)
    a, b = fm.Plan.profile(model, tr, N_s=128, line=c), fm.Plan.minlap(model, tr, N_s=128, N_c=32, iters=0, c_init=c)
    assert _bits(_np(a.table), _np(b.table)) and _bits(_np(a.t), _np(b.t)) and _bits(_np(b.line)[0], c)


def test_per_plan_blocks_in_the_loop_are_isolated(fm):
    """Three plans with their own blocks (so their own widths, grips of the tyres and lap times) in one call and one by one: the same
    bits; a block that cannot describe a car is NaN and never moves."""
    tr = fm.Track.load("fss2019")
    model, N_s, N_c = fm.DYNAMIC, 128, 32
    blocks = fm.param_draws(model, range(4), 77, 0.2)
    blocks[3, fm.PARAM_INDEX["M"]] = -1.0
    kw = dict(N_s=N_s, N_c=N_c, iters=2, rho=(100.0, 10.0, 3.0), grip=0.9)
    allp = fm.Plan.minlap(model, tr, params=blocks, **kw)
    lap, step, line, t = _np(allp.lap_history, allp.step_history, allp.control_points, allp.t)
    assert np.isnan(lap[3]).all() and (step[3] == -1).all() and np.isnan(line[3]).all() and np.isnan(t[3]).all()
    for p in range(3):
        one = fm.Plan.minlap(model, tr, params=blocks[p], **kw)
        l1, s1, c1, t1 = _np(one.lap_history, one.step_history, one.control_points, one.t)
        assert _bits(l1[0], lap[p]) and _bits(s1[0], step[p]) and _bits(c1[0], line[p]) and _bits(t1[0], t[p]), p
        assert lap[p, -1] < lap[p, 0] and np.abs(line[p]).max() <= blocks[p, fm.PARAM_INDEX["N_MAX"]] - 0.25 + 1e-12
    assert np.unique(lap[:3, 0]).size == 3


def test_corridor_boxes_are_kept_cell_by_cell(fm, orc):
    """Plan.minlap(corridor=): the start is Plan.raceline(corridor=), every cell of the final line lies in the corridor less the margin
    (through the offsets of the control points), a corridor with no room is NaN and its neighbours are what they are alone."""
    tr, otr = _tracks(fm, orc, "fss2019")
    model, N_s, N_c, N_w, margin = fm.DYNAMIC, 128, 32, 64, 0.1
    s = np.arange(N_w) * tr.L / N_w
    n_lo = np.stack([-0.6 + 0.25 * np.sin(2 * np.pi * s / tr.L), -0.15 * np.ones(N_w), -0.5 - 0.2 * np.cos(4 * np.pi * s / tr.L)])
    n_hi = np.stack([0.7 + 0.2 * np.cos(2 * np.pi * s / tr.L), 0.04 * np.ones(N_w), 0.45 + 0.2 * np.sin(2 * np.pi * s / tr.L)])       # corridor 1: 0.19 wide < 2 margin
    cor = fm.Corridor.from_table(n_lo, n_hi, tr.L)
    kw = dict(N_s=N_s, N_c=N_c, margin=margin)
    race = fm.Plan.raceline(model, tr, corridor=cor, **kw)
    plan = fm.Plan.minlap(model, tr, corridor=cor, iters=2, **kw)
    lap, step, line, flag = _np(plan.lap_history, plan.step_history, plan.control_points, plan.line_flag)
    assert plan.P == 3 and flag[1] == -1 and np.isnan(lap[1]).all() and (step[1] == -1).all() and np.isnan(line[1]).all() and np.isnan(_np(plan.t)[1]).all()
    assert _bits(flag, _np(race.line_flag))
    T0 = _np(fm.Plan.lap_gradient(model, tr, _np(race.line)[[0, 2]], N_s=N_s)[0])
    assert _bits(lap[[0, 2], 0], T0)
    lo_d, hi_d = _np(plan._box[0], plan._box[1])
    for p in (0, 2):
        assert (np.diff(lap[p]) <= 0).all() and lap[p, -1] < lap[p, 0]
        assert (line[p] >= lo_d[p]).all() and (line[p] <= hi_d[p]).all()
        n = rn.offsets(line[p], N_s)[0]
        si = np.arange(N_s) * tr.L / N_s
        lo_i, hi_i = np.interp(si, np.append(s, tr.L), np.append(n_lo[p], n_lo[p][0])), np.interp(si, np.append(s, tr.L), np.append(n_hi[p], n_hi[p][0]))
        assert (n >= lo_i + margin - 1e-12).all() and (n <= hi_i - margin + 1e-12).all(), p
        alone = fm.Plan.minlap(model, tr, corridor=fm.Corridor.from_table(n_lo[p], n_hi[p], tr.L), iters=2, **kw)
        assert _bits(_np(alone.lap_history)[0], lap[p]) and _bits(_np(alone.control_points)[0], line[p]) and _bits(_np(alone.t)[0], _np(plan.t)[p])


def test_a_folding_start_never_moves_and_its_neighbours_do_not_notice(fm, orc):
    tr, otr = _tracks(fm, orc, "fss2019")
    model, N_s, N_c = fm.DYNAMIC, 128, 32
    k, c = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c)
    fold = np.full(N_c, 0.95 / np.abs(k).max() * np.sign(k[np.argmax(np.abs(k))]))
    kw = dict(N_s=N_s, N_c=N_c, iters=2, margin=mc.MARGIN)
    a = fm.Plan.minlap(model, tr, c_init=np.stack([c, fold, 0.5 * c]), **kw)
    b = fm.Plan.minlap(model, tr, c_init=np.stack([c, 0.7 * c, 0.5 * c]), **kw)
    la, sa, ca = _np(a.lap_history, a.step_history, a.control_points)
    lb, sb, cb = _np(b.lap_history, b.step_history, b.control_points)
    assert np.isnan(la[1]).all() and (sa[1] == -1).all() and np.isnan(ca[1]).all() and np.isnan(_np(a.table)[1]).all()
    for p in (0, 2):
        assert _bits(la[p], lb[p]) and _bits(sa[p], sb[p]) and _bits(ca[p], cb[p]) and _bits(_np(a.t)[p], _np(b.t)[p])
    assert np.isfinite(lb).all() and (lb[:, -1] < lb[:, 0]).all()


@pytest.mark.parametrize("model", [0, 1])
def test_monte_carlo_takes_the_plan(fm, model):
    """Wiring only: the result is a Plan like any other."""
    tr = fm.Track.load("fss2019")
    plan = fm.Plan.minlap(model, tr, N_s=128, N_c=32, iters=2)
    cl, fl, it, ac = fm.monte_carlo(model, 20, tr, 8, 5, reference=plan)
    assert fl.shape == (5, 8) and np.isfinite(_np(cl.cart)).all() and np.isfinite(_np(cl.x_ref)).all()


def test_refusals_come_before_any_launch(fm):
    import ctypes as C
    import torch
    L = fm.lib()
    tr = fm.Track.load("fss2019")
    xP, yP = tr.device(torch.device("cuda:0"))
    p = lambda a: C.c_void_p(a.data_ptr())
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    N_s, N_c, K, J = 64, 16, 2, 3
    seven = lambda n, dt=torch.float64: torch.full((n,), 7, dtype=dt, device="cuda")
    line, flag, table, tt, lap, step, T, grad = seven(N_c), seven(1, torch.int32), seven(N_s * 8), seven(N_s), seven(K + 1), seven(K, torch.int32), seven(1), seven(N_c)
    need = L.fsaempc_plan_minlap_workspace_bytes(1, N_c, J)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    rho = (C.c_double * J)(100.0, 10.0, 3.0)
    bad = (C.c_double * J)(100.0, -10.0, 3.0)
    lg = lambda ns=N_s, nc=N_c: L.fsaempc_plan_line_lapgrad_batch_device(1, C.byref(sp), C.c_double(tr.L), None, 1, ns, nc, p(line), 0, C.c_double(20.0), C.c_double(1.0),
                                                                         p(T), p(grad), None)
    ml = lambda ns=N_s, nc=N_c, k=K, r=rho, j=J, lo=None, wsb=need: L.fsaempc_plan_minlap_batch_device(
        1, C.byref(sp), C.c_double(tr.L), None, 1, ns, nc, C.c_double(0.25), C.c_double(20.0), C.c_double(1.0), None, k, r, j, None, lo, None, p(line), p(flag), p(table),
        p(tt), p(lap), p(step), p(ws), C.c_longlong(wsb), None)
    for kw in (dict(nc=7), dict(ns=2 * N_c - 1), dict(ns=1025, nc=100)):
        assert lg(**kw) == -1 and ml(**kw) == -1, kw
    assert ml(k=-1) == -1 and ml(j=0) == -1 and ml(j=17) == -1 and ml(r=bad) == -1 and ml(lo=p(line)) == -1 and ml(wsb=need - 64) == -5
    torch.cuda.synchronize()
    assert all(bool((a == 7).all()) for a in (line, flag, table, tt, lap, step, T, grad)) and not bool(ws.any())
    with pytest.raises(ValueError):
        fm.Plan.minlap(fm.DYNAMIC, tr, N_s=1025, N_c=100)
