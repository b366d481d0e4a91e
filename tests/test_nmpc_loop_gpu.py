"""GPU tests of the batched SQP as the controller of the closed loop: the shift and take-over entries and the SQP's
skip mask against the restatement (tests/nmpc_loop_numpy.py, pinned by tests/test_nmpc_loop_cpu.py) bit for bit, ClosedLoop(controller=
Nmpc) against the same sequence driven by hand, what the mode means (the kept plan is the rollout of the kept inputs from the state the
solve read), off is off, and the whole loop engaged.  B = 70 (more than one wavefront, not a multiple of 64), N = 10, fsg2019.

No test asserts a convergence rate: the status shares are measured (profiles/nmpc_loop), not fixed in advance."""
import ctypes as C

import numpy as np
import pytest

import lap_numpy as lpn
import latency_cases as lc
import nlp_numpy as nn
import nmpc_cases as nc
import nmpc_loop_numpy as nl

pytestmark = pytest.mark.gpu

DT, B, N = lc.DT, lc.B, lc.N
ROLL_TOL = 1e-10       # the rollout tolerance of the SQP tests, of max(1, |x|)
SQP_KEYS = ("u_opt", "x_opt", "slack", "fval", "status", "sweeps", "lambda", "qp_iter", "step_norm", "hard_viol", "merit")


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
def tracks(fm, orc):
    return fm.Track.load("fsg2019"), orc.Track.load(fm.tracks._HERE + "/tracks/fsg2019.json")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(torch, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _g(t):
    return t.cpu().numpy().copy()


# ---- 1 ----
@pytest.mark.parametrize("horizon", [1, 2, 10])
def test_shift_entry_matches_the_restatement(fm, torch_, horizon):
    torch = torch_
    rng = np.random.default_rng(3 + horizon)
    u = rng.standard_normal((B, horizon, 2))
    u[5, 0, 0] = -0.0; u[64, horizon - 1, 1] = np.nan; u[69, 0, 1] = np.inf     # copied as they are
    fin = (np.arange(B) % 3).astype(np.int32)                                   # 0, 1 and 2
    for shift in (0, 1):
        for finished in (fin, None):
            u_keep = _dev(torch, u)
            u_init = torch.full((B, horizon, 2), nc.SENTINEL, dtype=torch.float64, device="cuda")
            skip = torch.full((B,), 7, dtype=torch.int32, device="cuda")
            assert nc.shift_entry(fm.lib(), horizon, B, shift, u_keep, _dev(torch, finished), u_init, skip) == 0, fm.lib().fsaempc_last_error()
            torch.cuda.synchronize()
            assert _same_bits(_g(u_init), nl.shift(u, shift)), (shift, finished is None)
            assert np.array_equal(_g(skip), nl.skip(finished, B)), (shift, finished is None)
            assert _same_bits(_g(u_keep), u)
    # the Python wrapper is the same call
    u_init = torch.empty((B, horizon, 2), dtype=torch.float64, device="cuda"); skip = torch.empty(B, dtype=torch.int32, device="cuda")
    fm.nmpc_shift(_dev(torch, u), _dev(torch, fin), 1, u_init, skip)
    torch.cuda.synchronize()
    assert _same_bits(_g(u_init), nl.shift(u, 1)) and np.array_equal(_g(skip), nl.skip(fin, B))


# ---- 2 ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_accept_entry_matches_the_restatement(fm, torch_, model):
    torch = torch_
    nx = 5 if model == 0 else 7
    Lx, Lu = N * nx, 2 * N                                   # 50 or 70 (the lanes' second pass), 20
    rng = np.random.default_rng(11 + model)
    xn, un = rng.standard_normal((B, Lx)), rng.standard_normal((B, Lu))
    status = np.array([nl.STATUSES[b % 6] for b in range(B)], dtype=np.int32)      # every status, with finite and non-finite plans
    xn[0, 0] = np.nan                                        # entry 0, status 0
    xn[8, 0] = np.nan                                        # entry 0, status 2
    xn[13, Lx - 1] = -np.inf                                 # the last entry, status 1
    if model == 1:
        xn[19, 64] = np.nan; xn[31, 66] = np.nan             # entries the lanes reach in their second pass (status 1, 1)
    un[16, Lu - 1] = np.inf                                  # the last entry of u_new, status -2
    un[69, Lu - 1] = np.inf                                  # ... status -1
    un[33, 3] = np.nan                                       # status -1
    skip = np.zeros(B, dtype=np.int32); skip[[5, 20, 26, 65]] = [1, 2, 1, 1]
    xn[26, 7] = np.nan                                       # a skipped car with a non-finite new plan
    qp_iter = (100 + np.arange(B)).astype(np.int32)
    xk0, uk0 = rng.standard_normal((B, N, nx)), rng.standard_normal((B, N, 2))
    seen = set()
    for it_in, sk_in in ((qp_iter, skip), (None, skip), (qp_iter, None), (None, None)):
        x_keep, u_keep = _dev(torch, xk0), _dev(torch, uk0)
        ef = torch.full((B,), -99, dtype=torch.int32, device="cuda"); it = torch.full((B,), -99, dtype=torch.int32, device="cuda")
        rc = nc.accept_entry(fm.lib(), model, N, B, _dev(torch, xn), _dev(torch, un), _dev(torch, status), _dev(torch, it_in), _dev(torch, sk_in),
                             x_keep, u_keep, ef, it)
        assert rc == 0, fm.lib().fsaempc_last_error()
        torch.cuda.synchronize()
        xr, ur, efr, itr = nl.accept(xn, un, status, it_in, sk_in, xk0.reshape(B, Lx), uk0.reshape(B, Lu))
        tag = (it_in is None, sk_in is None)
        assert _same_bits(_g(x_keep).reshape(B, Lx), xr), tag
        assert _same_bits(_g(u_keep).reshape(B, Lu), ur), tag
        assert np.array_equal(_g(ef), efr) and np.array_equal(_g(it), itr), tag
        kept = _bits(xr) == _bits(xk0.reshape(B, Lx))
        seen |= {(int(s), bool(k)) for s, k in zip(status, kept.all(axis=1))}
    # (the table covers what it is meant to: a plan taken over and a plan kept under a good, a capped and a failed status)
    assert {(0, False), (0, True), (1, False), (1, True), (2, True), (2, False), (-1, True), (-1, False), (-2, True), (-2, False), (4, False), (4, True)} <= seen
    # the Python wrapper is the same call
    x_keep, u_keep = _dev(torch, xk0), _dev(torch, uk0)
    ef = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty(B, dtype=torch.int32, device="cuda")
    fm.nmpc_accept(model, N, _dev(torch, xn), _dev(torch, un), _dev(torch, status), _dev(torch, qp_iter), _dev(torch, skip), x_keep, u_keep, ef, it)
    torch.cuda.synchronize()
    xr, ur, efr, itr = nl.accept(xn, un, status, qp_iter, skip, xk0.reshape(B, Lx), uk0.reshape(B, Lu))
    assert _same_bits(_g(x_keep).reshape(B, Lx), xr) and _same_bits(_g(u_keep).reshape(B, Lu), ur) and np.array_equal(_g(ef), efr) and np.array_equal(_g(it), itr)


# ---- 3 ----
def _raw_p(fm, torch, sb, x0, xr, u0, max_sweeps):
    """fsaempc_sqp_batch_device_p, the entry without a mask, with the outputs of SqpBatch.solve."""
    Bn, Nn, nx = sb.batch, sb.N, sb.nx
    o = fm._lib.sqp_default_opts(max_sweeps=max_sweeps)
    need = fm.lib().fsaempc_sqp_workspace_bytes(C.byref(sb.desc))
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
    out = dict(u_opt=f64(Bn, 2 * Nn), x_opt=f64(Bn, nx * Nn), slack=f64(Bn, sb.ns), fval=f64(Bn), status=i32(Bn), sweeps=i32(Bn),
               **{"lambda": f64(Bn, sb.nV + sb.nC)}, qp_iter=i32(Bn), step_norm=f64(Bn), hard_viol=f64(Bn), merit=f64(Bn, max_sweeps))
    P = lambda t: C.c_void_p(t.data_ptr())
    aux = fm._lib.SqpAux(P(out["lambda"]), P(out["qp_iter"]), P(out["step_norm"]), P(out["hard_viol"]), P(out["merit"]))
    rc = fm.lib().fsaempc_sqp_batch_device_p(C.byref(sb.desc), C.byref(sb.sp), None, P(x0), P(xr), P(u0), C.byref(sb.opts), C.byref(o), P(out["u_opt"]),
                                             P(out["x_opt"]), P(out["slack"]), P(out["fval"]), P(out["status"]), P(out["sweeps"]), C.byref(aux), P(ws),
                                             C.c_longlong(ws.numel() * 8), None)
    assert rc == 0, fm.lib().fsaempc_last_error()
    return out


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_sqp_skip_mask(fm, torch_, orc, tracks, model):
    torch = torch_
    tr, otr = tracks
    sweeps = 3
    x0, _, _, xr = fm.instances(model, N, DT, tr.L, 31, range(B))
    rng = np.random.default_rng(17 + model)
    u0 = np.stack([rng.uniform(-2, 2, (B, N)), rng.uniform(-0.05, 0.05, (B, N))], axis=2)
    k, b = np.arange(N)[None, :], np.arange(B)[:, None]
    out_of_box = (np.arange(B) % 7 == 0)                     # 10 cars start outside the input box (3 of them masked below): init clamps
    u0[out_of_box, :, 0] = (12.0 * np.cos(k + b))[out_of_box]
    u0[out_of_box, :, 1] = (0.6 * np.sin(2 * k + b))[out_of_box]
    P = fm.default_params(model)
    lim = np.array([P[fm.PARAM_INDEX["U_ACC_MAX"]], P[fm.PARAM_INDEX["U_STEER_MAX"]]])
    clamped = np.minimum(np.maximum(u0, -lim), lim)
    assert (clamped != u0).any()
    sb = fm.SqpBatch(model, N, DT, tr, B)
    dx0, dxr, du0 = _dev(torch, x0), _dev(torch, xr), _dev(torch, u0)
    get = lambda o: {kk: _g(o[kk]) for kk in SQP_KEYS}
    base = get(_raw_p(fm, torch, sb, dx0, dxr, du0, sweeps))
    torch.cuda.synchronize()
    assert (base["sweeps"] >= 1).all() and set(np.unique(base["status"])) <= {0, 1, 2, -1, -2}
    # no mask, and a mask of zeros: the bits of the entry without one, on every output
    for mask in (None, torch.zeros(B, dtype=torch.int32, device="cuda")):
        got = get(sb.solve(dx0, dxr, du0, skip=mask, max_sweeps=sweeps))
        for kk in SQP_KEYS:
            assert np.array_equal(got[kk], base[kk], equal_nan=True), (kk, mask is None)
    # every third instance masked (1 and 2 both mean "skip")
    m = np.zeros(B, dtype=np.int32); m[::3] = 1; m[::6] = 2
    got = get(sb.solve(dx0, dxr, du0, skip=_dev(torch, m), max_sweeps=sweeps))
    on, off = m == 0, m != 0
    for kk in SQP_KEYS:
        assert np.array_equal(got[kk][on], base[kk][on], equal_nan=True), kk     # the others do not notice
    assert (got["status"][off] == 4).all() and (got["sweeps"][off] == 0).all() and (got["qp_iter"][off] == 0).all()
    assert _same_bits(got["u_opt"][off], clamped.reshape(B, 2 * N)[off])
    assert np.isnan(got["merit"][off]).all() and np.isnan(got["step_norm"][off]).all()
    worst = 0.0
    for i in np.flatnonzero(off):
        X = nn.rollout(orc, model, otr, x0[i], clamped[i], DT, nn.default_integrator(model)).ravel()
        worst = max(worst, float((np.abs(got["x_opt"][i] - X) / np.maximum(1.0, np.abs(X))).max()))
    print("skipped instances: x_opt against the rollout of the clamped u_init %.3e of max(1, |x|)" % worst)
    assert worst <= ROLL_TOL
    # everybody masked: nothing is built or solved
    got = get(sb.solve(dx0, dxr, du0, skip=torch.ones(B, dtype=torch.int32, device="cuda"), max_sweeps=sweeps))
    assert (got["qp_iter"] == 0).all() and (got["status"] == 4).all() and (got["sweeps"] == 0).all()
    assert _same_bits(got["u_opt"], clamped.reshape(B, 2 * N))


# ---- 4 ----
def _loop(fm, torch, tr, otr, model, starts=None, **kw):
    cart, s0, v0, _ = lpn.cars(otr, B, starts)
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    return cl


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_step_is_the_sequence_of_its_public_pieces(fm, torch_, tracks, model):
    """The five cars of the lap report tiled to B (one reaches the end of the track parameter inside the run, one is lost at once: the
    mask is in use)."""
    torch = torch_
    tr, otr = tracks
    ctl = fm.Nmpc(sweeps=2)
    a = _loop(fm, torch, tr, otr, model, controller=ctl)
    h = _loop(fm, torch, tr, otr, model, controller=ctl)
    assert a.sqp is not None and a.sqp.params is None and a.u_init.shape == (B, N, 2) and a.nmpc_skip.dtype == torch.int32
    masked = 0
    for k in range(4):
        out = a.step()
        h.pre()
        fm.nmpc_shift(h.u_opt, h.finished, 0 if k == 0 else 1, h.u_init, h.nmpc_skip)
        res = h.sqp.solve(h.x0, h.x_ref, h.u_init, skip=h.nmpc_skip, max_sweeps=2)
        ef = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty(B, dtype=torch.int32, device="cuda")
        fm.nmpc_accept(model, N, res["x_opt"], res["u_opt"], res["status"], res["qp_iter"], h.nmpc_skip, h.x_opt, h.u_opt, ef, it)
        h.plant(None)
        h.steps += 1
        torch.cuda.synchronize()
        for name in ("cart", "x_opt", "u_opt", "u_init"):
            assert _same_bits(_g(getattr(a, name)), _g(getattr(h, name))), (k, name)
        assert np.array_equal(_g(a.finished), _g(h.finished)) and np.array_equal(_g(out["exitflag"]), _g(ef)) and np.array_equal(_g(out["iter"]), _g(it)), k
        assert np.array_equal(_g(a.nmpc_status), _g(res["status"])) and np.array_equal(_g(out["status"]), _g(res["status"]))
        assert np.array_equal(_g(a.nmpc_skip), (_g(a.finished) != 0).astype(np.int32))
        assert set(out) >= {"x_opt", "u_opt", "slack", "fval", "exitflag", "iter", "status", "sweeps", "qp_iter", "step_norm", "hard_viol"}
        masked += int((_g(a.nmpc_status) == 4).sum())
    fin = _g(a.finished)
    assert masked > 0 and (fin == 0).any() and (fin == 2).any()


# ---- 5 ----
def _rollout_error(orc, otr, model, x0, x_opt, u_opt, cars):
    worst = 0.0
    for b in cars:
        X = nn.rollout(orc, model, otr, x0[b], u_opt[b], DT, nn.default_integrator(model))
        worst = max(worst, float((np.abs(x_opt[b] - X) / np.maximum(1.0, np.abs(X))).max()))
    return worst


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_kept_plan_is_the_rollout_of_the_kept_inputs(fm, torch_, orc, tracks, model):
    torch = torch_
    tr, otr = tracks
    P = fm.default_params(model)
    lim = np.array([P[fm.PARAM_INDEX["U_ACC_MAX"]], P[fm.PARAM_INDEX["U_STEER_MAX"]]])
    cl = _loop(fm, torch, tr, otr, model, controller=fm.Nmpc(sweeps=2))
    ltv = _loop(fm, torch, tr, otr, model)
    worst = worst_ltv = 0.0
    checked = 0
    prev_u = None
    for k in range(6):
        out = cl.step()
        ltv.step()
        torch.cuda.synchronize()
        fin, x0, x_opt, u_opt = _g(cl.finished), _g(cl.x0), _g(cl.x_opt), _g(cl.u_opt)
        res_ok = np.isfinite(_g(out["x_opt"])).all(axis=1) & np.isfinite(_g(out["u_opt"])).all(axis=1)
        cars = np.flatnonzero((fin == 0) & res_ok)
        checked += cars.size
        worst = max(worst, _rollout_error(orc, otr, model, x0, x_opt, u_opt, cars))
        assert (np.abs(u_opt[cars]) <= lim).all(), k
        if prev_u is not None:       # the start of this period's solve is the previous plan, one stage on
            assert _same_bits(_g(cl.u_init)[:, : N - 1], prev_u[:, 1:]) and _same_bits(_g(cl.u_init)[:, N - 1], prev_u[:, N - 1]), k
        else:
            assert _same_bits(_g(cl.u_init), np.tile(np.array([10.0, 0.0]), (B, N, 1)))        # the unshifted guess of main.m:47-55
        prev_u = u_opt
        lfin = _g(ltv.finished)
        worst_ltv = max(worst_ltv, _rollout_error(orc, otr, model, _g(ltv.x0), _g(ltv.x_opt), _g(ltv.u_opt), np.flatnonzero(lfin == 0)))
    print("kept plan against the rollout of the kept inputs, of max(1, |x|): NMPC %.3e over %d car-periods; the LTV controller's plan %.3e "
          "(a linearised prediction: not asserted)" % (worst, checked, worst_ltv))
    assert checked >= 6 * B // 2
    assert worst <= ROLL_TOL


# ---- 6 ----
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_off_is_off(fm, torch_, tracks, model):
    tr, _ = tracks
    plan = fm.Plan.profile(model, tr)

    def run(reference, **kw):
        cl = fm.monte_carlo(model, N, tr, B, 5, seed=11, reference=reference, **kw)[0]
        return cl, [t.cpu().numpy() for t in (cl.cart, cl.x_opt, cl.finished)]
    for reference in (None, plan):
        _, base = run(reference)
        cl, got = run(reference, controller=None)
        assert cl.sqp is None and cl.controller is None and cl.u_init is None and cl.nmpc_skip is None and cl.nmpc_status is None
        assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]) and np.array_equal(got[2], base[2])
    assert (base[2] == 0).any()
    # ... and on is on: the same run under the SQP is another run
    cl, got = run(plan, controller=fm.Nmpc(sweeps=1))
    assert cl.sqp is not None and not _same_bits(got[1], base[1])


# ---- 7 ----
def test_whole_loop_engaged(fm, torch_, tracks):
    """Dynamic model under the SQP with a plan reference, a parameter block per car, noise, one period of compensated delay, the
    estimator, the lap gate firing inside the run and the lap report: everything stays finite, nobody leaves the race, and the report's
    abnormal count is the count of recorded statuses other than 0 and 1."""
    torch = torch_
    tr, otr = tracks
    model, d, steps = fm.DYNAMIC, 1, 8
    sigma = np.array([0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005])
    plan = fm.Plan.profile(model, tr)
    Pb = fm.param_draws(model, np.arange(B), 77, 0.1)
    starts = [(otr.L - 3.0, 0.05 * i, 10.0) for i in range(-3, 4)]      # 3 m before the line at 10 m/s: the crossing falls inside the run
    cl = _loop(fm, torch, tr, otr, model, starts, controller=fm.Nmpc(sweeps=2), reference=plan, params=Pb,
               latency=fm.Latency(delay=d, compensate=True, sigma=sigma, seed=lc.SEED, id0=1000), estimator=fm.Estimator(0.1 * sigma ** 2), laps=2,
               metrics=True)
    assert cl.sqp.params is not None and cl.sqp.params.per_instance == 1
    status, driving = [], []
    for k in range(steps):
        out = cl.step()
        status.append(_g(out["status"])); driving.append(_g(cl.finished) == 0)
    torch.cuda.synchronize()
    status, driving = np.array(status), np.array(driving)
    print("statuses over %d car-periods: %s" % (status.size, dict(zip(*[v.tolist() for v in np.unique(status, return_counts=True)]))))
    for name in ("cart", "x_opt", "u_opt", "u_init", "x0", "x0_obs", "x0_est", "x0_mpc", "x_ref", "x_hist", "u_hist", "est_x", "est_P", "metrics", "lap_records"):
        assert np.isfinite(_g(getattr(cl, name))).all(), name
    assert (_g(cl.finished) == 0).all()                                  # no car lost, none at the end of its run
    assert (_g(cl.lap_state[:, fm.LAP_STATE_INDEX["DONE"]]) == 1).all()  # the gate fired for every car
    rep = cl.report()
    assert np.isfinite(rep.metrics).all() and np.isfinite(rep.lap_records).all() and np.isfinite(_g(cl.lap_times[:, 0])).all()
    abnormal = rep.lap_records[:, :, fm.METRIC_INDEX["ABNORMAL"]].sum()      # the closed lap's record plus the current one, per car
    want = int((driving & (status != 0) & (status != 1)).sum())
    assert abnormal == want, (abnormal, want)


# ---- 8 ----
def test_abi_refusals(fm):
    nc.check_abi_refusals("cuda")
