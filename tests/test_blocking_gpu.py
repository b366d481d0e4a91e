"""GPU tests of move blocking (held inputs): the blocked construction kernel against the numpy condensation of the
unblocked QP (tests/block_numpy.py), the trivial blocking against the unblocked path (bitwise), the fused blocked step against the
oracle on the condensed QP, the layout hint of the generic solve, the blocked closed loop, isolation and the refusals."""
import ctypes as C

import numpy as np
import pytest

import block_numpy as bn
from conftest import relerr
from kkt_numpy import kkt_certificate, vertex_from_working_set, working_set
from test_blocking_cpu import SHAPES

pytestmark = pytest.mark.gpu

DT, SEED = 0.05, 31
KKT_TOL = 1e-6          # the tolerances of tests/test_gpu_parity.py
FVAL_TOL = 1e-6
X_TOL = 5e-3
X_TOL_VERTEX = 1e-6
BUILD_TOL = 1e-9        # the project's construction tolerance (tests/test_gpu_parity.py::test_construction_parity)
QP = ("H", "g", "A", "lb", "ub", "lbA", "ubA")
QP_KEYS = QP + ("pred", "Bt", "const")
STEP_KEYS = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")


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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _np(torch, d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _tracks(fm, orc, name):
    return fm.Track.load(name), orc.Track.load(fm.tracks._HERE + "/tracks/%s.json" % name)


def _inputs(torch, inp):
    x0, xl, ul, xr = inp
    return _dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul)


# ---- 1. construction parity ----
@pytest.mark.parametrize("model,N,lens,track,_B", SHAPES)
def test_blocked_construction_against_the_condensed_oracle_build(fm, torch_, orc, model, N, lens, track, _B):
    torch = torch_
    tr, otr = _tracks(fm, orc, track)
    B, ns = 16, (1 if model == 0 else 4)
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    x0, xl, ul, xr = inp
    mpc = fm.LtvBatch(model, N, DT, tr, B, blocking=lens)
    assert mpc.n_blocks == len(lens) and mpc.nV == 2 * len(lens) + ns and mpc.block_of_step == list(bn.block_of_step(lens))
    q = _np(torch, mpc.build_qp(*_inputs(torch, inp)))
    E = bn.blocking_matrix(lens, ns)
    ref = orc.build_qp_batch(model, otr, N, DT, x0, xr, xl, ul, keep_prediction=True)
    refb = bn.block_qp(ref, E)
    for k in QP + ("const", "Bt"):
        err = relerr(q[k], refb[k])
        print("blocked build", model, N, k, err)
        assert err <= BUILD_TOL, (k, err)
    pred = np.einsum("bcr,bc->br", ref["A_bar"], x0) + ref["d_bar"]
    assert relerr(q["pred"], pred) <= BUILD_TOL


@pytest.mark.parametrize("model,N,lens,track,_B", SHAPES)
def test_blocked_construction_under_per_instance_parameters(fm, torch_, model, N, lens, track, _B):
    torch = torch_
    tr = fm.Track.load(track)
    B, ns = 16, (1 if model == 0 else 4)
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    P = fm.param_draws(model, range(B), SEED, 0.1)
    q = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens).build_qp(*_inputs(torch, inp)))
    full = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P).build_qp(*_inputs(torch, inp)))
    refb = bn.block_qp(full, bn.blocking_matrix(lens, ns))
    for k in QP_KEYS:
        err = relerr(q[k], refb[k])
        print("blocked build, parameters", model, N, k, err)
        assert err <= BUILD_TOL, (k, err)
    # an invalid block: NaN in g of that instance alone
    P[3, fm.PARAM_INDEX["M"]] = -1.0
    q = _np(torch, fm.LtvBatch(model, N, DT, tr, B, params=P, blocking=lens).build_qp(*_inputs(torch, inp)))
    assert np.isnan(q["g"][3]).all() and np.isfinite(np.delete(q["g"], 3, axis=0)).all()


# ---- 2. the trivial blocking is the unblocked path ----
@pytest.mark.parametrize("model,N", [(0, 40), (1, 60)])
def test_one_step_per_block_is_bitwise_the_unblocked_path(fm, torch_, model, N):
    torch = torch_
    tr = fm.Track.load("fsg2019")
    B = 16
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    a, b = fm.LtvBatch(model, N, DT, tr, B), fm.LtvBatch(model, N, DT, tr, B, blocking=[1] * N)
    assert b.nV == a.nV
    qa, qb = _np(torch, a.build_qp(*_inputs(torch, inp))), _np(torch, b.build_qp(*_inputs(torch, inp)))
    for k in QP_KEYS:
        assert np.array_equal(qa[k], qb[k], equal_nan=True), k
    sa = _np(torch, a.step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    sb = _np(torch, b.step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    for k in STEP_KEYS + ("kkt", "polished", "lam"):
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k


# ---- 3. step parity against the oracle ----
@pytest.mark.parametrize("model,N,lens,track,B", SHAPES)
def test_blocked_step_against_the_oracle(fm, torch_, orc, model, N, lens, track, B):
    """Largest deviations observed on the MI355X: DESIGN.md 6h."""
    torch = torch_
    tr, otr = _tracks(fm, orc, track)
    ns, M = (1 if model == 0 else 4), len(lens)
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    x0, xl, ul, xr = inp
    E = bn.blocking_matrix(lens, ns)
    ref_q = bn.block_qp(orc.build_qp_batch(model, otr, N, DT, x0, xr, xl, ul), E)
    ref = orc.qp_solve_batch_aux(*[ref_q[k] for k in QP])
    assert (ref["exitflag"] == 0).all(), ref["exitflag"]          # the oracle alone solves every instance: nothing may be left out
    mpc = fm.LtvBatch(model, N, DT, tr, B, blocking=lens)
    q = _np(torch, mpc.build_qp(*_inputs(torch, inp)))
    out = _np(torch, mpc.step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    assert out["lam"].shape == (B, 2 * M + ns + q["lbA"].shape[1]) and out["u_opt"].shape == (B, 2 * N)
    assert (out["exitflag"] == 0).all(), np.unique(out["exitflag"], return_counts=True)
    print("blocked step", model, N, "kkt max", out["kkt"].max(), "iter mean", out["iter"].mean(), "vertex share", (out["polished"] > 0).mean(),
          "oracle vertex share", (ref["polished"] > 0).mean())
    assert out["kkt"].max() <= KKT_TOL, out["kkt"].max()
    # the blocked variables: the first held value of every block and the slacks
    first = np.array([np.nonzero(E[:, j])[0][0] for j in range(2 * M)])
    z = np.concatenate([out["u_opt"][:, first], out["slack"]], axis=1)
    assert np.array_equal(out["u_opt"], z[:, : 2 * M] @ E[: 2 * N, : 2 * M].T)          # expanded u_opt == E z (copies: exact)
    c = kkt_certificate(*[q[k] for k in QP], z, out["lam"])
    print("  certificate max", c["max"].max())
    assert c["max"].max() <= KKT_TOL, {k: float(np.max(c[k])) for k in ("stationarity", "primal", "sign", "complementarity")}
    fo = ref["fval"] + ref_q["const"]
    ferr = np.abs(out["fval"] - fo) / np.maximum(1.0, np.abs(fo))
    print("  fval err max", ferr.max())
    assert ferr.max() <= FVAL_TOL, ferr.max()
    xo = q["pred"] + np.einsum("bcr,bc->br", q["Bt"], z)
    xerr = relerr(out["x_opt"], xo)
    print("  x_opt err", xerr)
    assert xerr <= 1e-9
    # x against the oracle, per instance: 1e-6 where both sides report the refined vertex (else the working sets and the recomputed
    # vertex decide, as in tests/test_gpu_parity.py::_vertex_agreement), 5e-3 where either side returned an interior-point iterate
    ex = np.abs(z - ref["x"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1))
    both = (out["polished"] > 0) & (ref["polished"] > 0)
    print("  x err: both at the vertex (%d) max %.3e, others max %.3e" % (both.sum(), ex[both].max() if both.any() else 0.0, ex[~both].max() if (~both).any() else 0.0))
    assert (ex[~both] <= X_TOL).all(), ex[~both].max()
    bad = np.nonzero(both & (ex > X_TOL_VERTEX))[0]
    assert len(bad) <= max(1, int(both.sum()) // 10), ex[bad]
    for b in bad:
        H, g, A = q["H"][b].T, q["g"][b], q["A"][b].T
        args = (q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b])
        ws_g = working_set(*args, z[b], A @ z[b], out["lam"][b])
        ws_o = working_set(*args, ref["x"][b], A @ ref["x"][b], ref["lam"][b])
        assert np.array_equal(ws_g, ws_o), (b, np.nonzero(ws_g != ws_o)[0])
    # the oracle refines few blocked instances (its refinement gives up on working sets larger than nV): the GPU's own claim, then --
    # wherever it reports the vertex, x is the vertex of its own working set as dense numpy algebra recomputes it
    worst = 0.0
    for b in np.nonzero(out["polished"] > 0)[0]:
        H, g, A = q["H"][b].T, q["g"][b], q["A"][b].T
        args = (q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b])
        xv = vertex_from_working_set(H, g, A, *args, working_set(*args, z[b], A @ z[b], out["lam"][b]))[0]
        err = np.abs(z[b] - xv).max() / max(1.0, np.abs(xv).max())
        worst = max(worst, err)
        assert err <= X_TOL_VERTEX, (b, err)
    print("  own vertex err max", worst)


# ---- 4. the layout route ----
def test_generic_solve_with_and_without_the_slack_hint(fm, torch_, orc):
    torch = torch_
    tr, otr = _tracks(fm, orc, "fsg2019")
    model, N, lens, B = 1, 80, [2] * 40, 32
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    q = fm.LtvBatch(model, N, DT, tr, B, blocking=lens).build_qp(*_inputs(torch, inp))
    assert tuple(q["g"].shape) == (B, 84)
    hint = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP], n_slack=4, want_aux=True))
    plain = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP], want_aux=True))
    assert (hint["exitflag"] == 0).all() and (plain["exitflag"] == 0).all(), (hint["exitflag"], plain["exitflag"])
    ferr = np.abs(hint["fval"] - plain["fval"]) / np.maximum(1.0, np.abs(plain["fval"]))
    assert ferr.max() <= FVAL_TOL, ferr.max()
    # dynamic N = 60 in 30 blocks: nV_b = 64, the shape whose slack columns only the hint keeps off the matrix cores
    model, N, lens = 1, 60, [2] * 30
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    q = fm.LtvBatch(model, N, DT, tr, B, blocking=lens).build_qp(*_inputs(torch, inp))
    hint = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP], n_slack=4))
    plain = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP]))
    assert (hint["exitflag"] == 0).all(), hint["exitflag"]
    ok = plain["exitflag"] == 0
    ferr = np.abs(hint["fval"] - plain["fval"])[ok] / np.maximum(1.0, np.abs(plain["fval"][ok]))
    print("nV_b = 64 without the hint: flags", np.unique(plain["exitflag"], return_counts=True), "fval err", ferr.max() if ok.any() else None)
    assert ferr.size == 0 or ferr.max() <= FVAL_TOL
    # a reference-shaped QP: the matching hint changes nothing, bit for bit
    for model, N in ((0, 40), (1, 60)):
        ns = 1 if model == 0 else 4
        inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
        q = fm.LtvBatch(model, N, DT, tr, B).build_qp(*_inputs(torch, inp))
        a = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP], n_slack=ns, want_lambda=True, want_aux=True))
        b = _np(torch, fm.qp_solve_batch_device(*[q[k] for k in QP], want_lambda=True, want_aux=True))
        for k in ("x", "fval", "exitflag", "iter", "lam", "kkt", "polished"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (model, N, k)


# ---- 5. closed loop ----
def _standstill_carts(orc, otr, B):
    """The start of tests/test_gpu_parity.py::test_closed_loop_short_run: cars at rest on the centre line, 5 m apart."""
    carts = np.zeros((B, 7))
    orc.lib().orc_spline_d.restype = C.c_double
    for b in range(B):
        s = 5.0 * b
        x, y = (orc.lib().orc_spline_val(P, otr.M, C.c_double(otr.dl), C.c_double(s)) for P in (otr.c.xP, otr.c.yP))
        th = np.arctan2(orc.lib().orc_spline_d(otr.c.yP, otr.M, C.c_double(otr.dl), C.c_double(s)), orc.lib().orc_spline_d(otr.c.xP, otr.M, C.c_double(otr.dl), C.c_double(s)))
        carts[b, :3] = [x, y, th]
    return carts


@pytest.mark.parametrize("model", [0, 1])
def test_blocked_closed_loop_short_run(fm, torch_, orc, model):
    """The blocked counterpart of tests/test_gpu_parity.py::test_closed_loop_short_run: the HIP loop with held inputs against the same loop
    driven through the oracle (build, numpy condensation, solve, expansion), same 1e-4 on the Cartesian states."""
    torch = torch_
    tr, otr = _tracks(fm, orc, "fss2019")
    N, dt, B, T = 20, 0.05, 3, 6
    lens = [1] * 4 + [2] * 4 + [4] * 2
    carts = _standstill_carts(orc, otr, B)
    cl = fm.ClosedLoop(model, N, dt, tr, carts, blocking=lens)
    nx, ns = cl.nx, (1 if model == 0 else 4)
    E = bn.blocking_matrix(lens, ns)
    k = np.arange(1, N + 1) * dt
    xo = np.zeros((B, N, nx)); uo = np.zeros((B, N, 2)); xo[:, :, 0] = 10 * k ** 2 / 2; xo[:, :, 3] = 10 * k; uo[:, :, 0] = 10
    xo[:, :, 0] += 5.0 * np.arange(B)[:, None]
    cl.x_opt[:, :, 0] += _dev(torch, 5.0 * np.arange(B))[:, None]
    oc = carts.copy(); opid = np.zeros((B, 4))
    for step in range(T):
        out = cl.step(); torch.cuda.synchronize()
        assert (out["exitflag"].cpu().numpy() == 0).all()
        x0 = np.zeros((B, nx)); xr = np.zeros((B, N, nx))
        for b in range(B):
            x0[b], x_ref, fin = orc.cl_pre(model, N, dt, otr, oc[b], xo[b, 0, 0])
            xr[b] = x_ref.T
        qf = orc.build_qp_batch(model, otr, N, dt, x0, xr, xo, uo, keep_prediction=True)
        qb = bn.block_qp(qf, E)
        r = orc.qp_solve_batch_aux(*[qb[kk] for kk in QP])
        assert (r["exitflag"] == 0).all(), r["exitflag"]
        zf = r["x"] @ E.T
        pred = np.einsum("bcr,bc->br", qf["A_bar"], x0) + qf["d_bar"]
        xo = (pred + np.einsum("bcr,bc->br", qf["Bt"], zf)).reshape(B, N, nx); uo = zf[:, : 2 * N].reshape(B, N, 2)
        for b in range(B):
            oc[b], opid[b], _ = orc.plant_step(oc[b], opid[b], xo[b, 0, 3], xo[b, 0, nx - 1], dt)
        assert np.max(np.abs(cl.cart.cpu().numpy() - oc)) <= 1e-4 * max(1.0, np.abs(oc).max()), step
    assert (cl.cart[:, 3] > 0.3).all()       # the cars accelerated from standstill


@pytest.mark.parametrize("model", [0, 1])
def test_blocked_closed_loop_warm_start_returns_the_same_flags(fm, torch_, orc, model):
    """ClosedLoop(warm_start=True, blocking=...): x_init is the shifted previous plan sampled at each block's first step; the same
    cars, the same exit flags as the cold loop over 10 steps."""
    torch = torch_
    tr, otr = _tracks(fm, orc, "fss2019")
    N, dt, B, T = 20, 0.05, 3, 10
    lens = [1] * 4 + [2] * 4 + [4] * 2
    carts = _standstill_carts(orc, otr, B)
    flags = {}
    for warm in (False, True):
        cl = fm.ClosedLoop(model, N, dt, tr, carts, blocking=lens, warm_start=warm)
        cl.x_opt[:, :, 0] += _dev(torch, 5.0 * np.arange(B))[:, None]
        fl = []
        for step in range(T):
            out = cl.step(); torch.cuda.synchronize()
            fl.append(out["exitflag"].cpu().numpy().copy())
            if warm and step > 0:      # what the solve was started from: held inputs of the previous plan, one step on
                assert tuple(cl._x_init.shape) == (B, 2 * len(lens) + (1 if model == 0 else 4))
        flags[warm] = np.array(fl)
    assert np.array_equal(flags[False], flags[True]), (flags[False], flags[True])
    assert (flags[False] == 0).all(), flags[False]


# ---- 6. isolation and refusals ----
@pytest.mark.parametrize("model,N,lens", [(0, 40, [1] * 8 + [2] * 8 + [4] * 4), (1, 60, [1] * 12 + [2] * 12 + [4] * 6)])
def test_a_blocked_instance_alone_and_inside_a_batch(fm, torch_, model, N, lens):
    torch = torch_
    tr = fm.Track.load("fsg2019")
    B, pick = 256, 137
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    one = tuple(a[pick:pick + 1] for a in inp)
    big = _np(torch, fm.LtvBatch(model, N, DT, tr, B, blocking=lens).step(*_inputs(torch, inp), want_aux=True, want_lambda=True))
    solo = _np(torch, fm.LtvBatch(model, N, DT, tr, 1, blocking=lens).step(*_inputs(torch, one), want_aux=True, want_lambda=True))
    for k in STEP_KEYS + ("kkt", "polished", "lam"):
        assert np.array_equal(big[k][pick], solo[k][0], equal_nan=True), k
    qb = _np(torch, fm.LtvBatch(model, N, DT, tr, B, blocking=lens).build_qp(*_inputs(torch, inp)))
    qs = _np(torch, fm.LtvBatch(model, N, DT, tr, 1, blocking=lens).build_qp(*_inputs(torch, one)))
    for k in QP_KEYS:
        assert np.array_equal(qb[k][pick], qs[k][0], equal_nan=True), k


def test_paths_without_a_blocked_form_refuse_a_blocked_batch(fm, torch_):
    torch = torch_
    tr = fm.Track.load("fsg2019")
    model, N, B, lens = 0, 20, 4, [1] * 4 + [2] * 4 + [4] * 2
    inp = fm.instances(model, N, DT, tr.L, SEED, range(B))
    x0, xr, xl, ul = _inputs(torch, inp)
    mpc = fm.LtvBatch(model, N, DT, tr, B, blocking=lens)
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.SqpBatch(model, N, DT, tr, B, blocking=lens)
    fm.SqpBatch(model, N, DT, tr, B, blocking=[1] * N)
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.ltv_step_affine_maps(mpc, xl, ul)
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.ltv_step_vjp(mpc, {}, x0, xr, xl, ul, ubar=torch.ones((B, 2 * N), dtype=torch.float64, device="cuda"))
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.ltv_step_diff(mpc, x0, xr, xl, ul)
    with pytest.raises(NotImplementedError, match="blocking"):
        fm.feedback_gain(mpc, x0, xr, xl, ul)
    # the re-linearisation loop does run on a blocked batch, in blocked sizes
    out = mpc.sqp(x0, xr, xl, ul, sweeps=2)
    torch.cuda.synchronize()
    assert (out["exitflag"] == 0).all() and tuple(out["u_opt"].shape) == (B, 2 * N) and len(out["du"]) == 2
    u = out["u_opt"].cpu().numpy().reshape(B, N, 2)
    assert np.array_equal(u, u[:, [mpc.blocking.start[j] for j in mpc.block_of_step], :])     # held over every block
