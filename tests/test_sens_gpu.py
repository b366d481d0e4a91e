"""GPU tests of the vector-Jacobian product of the batched QP solve (fsaempc_qp_vjp_batch_device, fsae_mpc_amd.qp_vjp / QpFunction):
against the dense numpy adjoint (tests/sens_numpy.py), against directional differences of the forward GPU solve, known answers,
the autograd wrapper, and isolation of instances."""
import numpy as np
import pytest

import sens_numpy as sn

pytestmark = pytest.mark.gpu

DT = 0.05


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
def track(fm):
    return fm.Track.load("fsg2019")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _problem(fm, torch, tr, model, N, B, seed=20190):
    x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, seed, range(B))
    q = fm.LtvBatch(model, N, DT, tr, B).build_qp(_dev(torch, x0), _dev(torch, xr), _dev(torch, xl), _dev(torch, ul))
    return q, _solve(fm, q)


def _solve(fm, q):
    return fm.qp_solve_batch_device(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"], want_lambda=True, want_aux=True)


def _vjp(fm, q, r, xbar, fbar=None, **kw):
    return fm.qp_vjp(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"], r["x"], r["lam"], r["exitflag"], r["polished"],
                     xbar, fbar, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b))))) if np.size(b) else 0.0


@pytest.mark.parametrize("model,N,B", [(0, 40, 256), (1, 60, 64), (1, 80, 64)])
def test_vjp_matches_numpy_adjoint(fm, torch_, track, model, N, B):
    torch = torch_
    q, r = _problem(fm, torch, track, model, N, B)
    nV = q["g"].shape[1]
    rng = np.random.default_rng(N)
    k = 2
    xbar = rng.standard_normal((B, k, nV))
    fbar = rng.standard_normal((B, k))
    out = _vjp(fm, q, r, _dev(torch, xbar), _dev(torch, fbar), want_H=True, want_A=(model == 0 or N == 60))
    torch.cuda.synchronize()
    st = _np(out["status"])
    pol = _np(r["polished"]) > 0
    flag = _np(r["exitflag"])
    # every refined instance gets its derivative: status 0, or 1 where a working-set multiplier is degenerate (weakly active)
    assert not (pol & (flag == 0) & (st < 0)).any(), (st[pol], np.unique(st, return_counts=True))
    assert (st == 0).sum() >= (pol & (flag == 0)).sum() - (st == 1).sum()
    assert (st[pol & (flag == 0)] != 2).all() and (st[~pol & (flag == 0)] != 0).all()
    H, g, A, lb, ub, lbA, ubA = (_np(q[k_]) for k_ in ("H", "g", "A", "lb", "ub", "lbA", "ubA"))
    x, lam = _np(r["x"]), _np(r["lam"])
    got = {key: _np(v) for key, v in out.items() if key != "status"}
    worst, where = 0.0, None
    for b in np.nonzero(st == 0)[0]:
        ws = sn.working_set_rule(lb[b], ub[b], lbA[b], ubA[b], x[b], A[b].T, lam[b])
        for c in range(k):
            ref = sn.adjoint(H[b].T, g[b], A[b].T, x[b], lam[b], ws, xbar[b, c], fbar[b, c])
            # the tolerance rule is sens_numpy.compare's
            e, w_ = sn.compare({key: got[key][b, c] for key in got}, ref, H[b].T, g[b], A[b].T, x[b], lam[b], xbar[b, c], fbar[b, c])
            if e > worst:
                worst, where = e, (int(b), c) + w_
    assert worst <= 1.0, (worst, where)
    # the returned (w, mu) solves the adjoint system, on every computed status (1 and 2 use the rule's working set by the same
    # algebra): residual relative to the sizes of its terms (w relative to xbar / |H|, since w vanishes on a full vertex); the kernel
    # itself stops at 1e-12 of its equilibrated system (measured here: 2.6e-10 worst)
    rmax, rwhere = 0.0, None
    for b in np.nonzero(st >= 0)[0]:
        for c in range(k):
            e, parts = sn.residual({key: got[key][b, c] for key in ("g", "lb", "ub", "lbA", "ubA")}, H[b].T, g[b], A[b].T, x[b], xbar[b, c], fbar[b, c])
            if e > rmax:
                rmax, rwhere = e, (int(b), c) + parts
    assert rmax <= 1e-9, (rmax, rwhere)
    # the weak-multiplier rule (|lambda| <= tol (1 + |lambda|_inf), the slack costs make |lambda|_inf ~1e8) puts many dynamic vertices
    # in status 1; their cotangents are computed all the same (measured: kinematic N=40 70 % status 0, dynamic N=80 34 %)
    assert (st >= 0).sum() >= B * 9 // 10 and (st == 0).sum() >= B // 4, np.unique(st, return_counts=True)


def _ws(fm, q, r):
    """Working set of the rule per instance (device -> numpy), for comparing two solves."""
    x, lam = _np(r["x"]), _np(r["lam"])
    lb, ub, lbA, ubA, A = (_np(q[k_]) for k_ in ("lb", "ub", "lbA", "ubA", "A"))
    return np.stack([sn.working_set_rule(lb[b], ub[b], lbA[b], ubA[b], x[b], A[b].T, lam[b]) for b in range(x.shape[0])])


@pytest.mark.parametrize("model,N,B", [(0, 40, 128), (1, 60, 32)])
def test_vjp_matches_directional_differences_of_the_forward_solve(fm, torch_, track, model, N, B):
    torch = torch_
    q, r = _problem(fm, torch, track, model, N, B)
    nV, nC = q["g"].shape[1], q["lbA"].shape[1]
    rng = np.random.default_rng(3)
    xbar = rng.standard_normal((B, nV))
    out = _vjp(fm, q, r, _dev(torch, xbar))
    st = _np(out["status"])
    ws0 = _ws(fm, q, r)
    total = 0
    for key, n_ in (("g", nV), ("lbA", nC), ("ubA", nC)):
        base = _np(q[key])
        finite = np.abs(base) < 1e9
        # entries span many scales (g holds the 1e8 slack costs): each moves by h relative to its own size
        s0 = float(np.median(np.abs(base[finite & (base != 0)]))) if (finite & (base != 0)).any() else 1.0
        v = rng.standard_normal(base.shape) * np.where(finite, np.maximum(np.abs(base), s0), 0.0)
        # the map is affine while the working set holds: per instance the largest step that keeps it at +-h is used, which keeps
        # the forward's own rounding out of the quotient as far as possible
        fd, ok = np.zeros(B), np.zeros(B, dtype=bool)
        for h in (1e-5, 1e-4, 1e-3):
            xs, same = [], (st == 0)
            for s in (1.0, -1.0):
                q2 = dict(q)
                q2[key] = _dev(torch, base + s * h * v)
                r2 = _solve(fm, q2)
                same &= (_np(r2["polished"]) > 0) & (_np(r2["exitflag"]) == 0) & (_ws(fm, q2, r2) == ws0).all(axis=1)
                xs.append(_np(r2["x"]))
            fd = np.where(same, np.einsum("bi,bi->b", xbar, (xs[0] - xs[1]) / (2 * h)), fd)
            ok |= same
        an = np.einsum("bi,bi->b", _np(out[key]), v)
        sc = np.maximum(1.0, np.maximum(np.abs(an), np.abs(fd)))
        err = np.abs(fd - an) / sc
        # the forward vertex itself is only as exact as the solver's refinement: most instances agree to 1e-6, a few near-degenerate
        # working sets less well
        assert ok.sum() >= B // 8, (key, int(ok.sum()), int((st == 0).sum()))
        assert np.quantile(err[ok], 0.9) <= 1e-6 and err[ok].max() <= 1e-3, (key, np.sort(err[ok])[-5:], np.median(err[ok]), int(ok.sum()))
        total += int(ok.sum())
    assert total >= B


def _one(fm, torch, H, g, A, lb, ub, lbA, ubA):
    n = len(g)
    A = np.zeros((0, n)) if A is None else np.asarray(A, dtype=np.float64)
    q = dict(H=_dev(torch, np.asarray(H, dtype=np.float64).T[None]), g=_dev(torch, np.asarray(g)[None]),
             A=_dev(torch, A.T[None]), lb=_dev(torch, np.asarray(lb)[None]), ub=_dev(torch, np.asarray(ub)[None]),
             lbA=_dev(torch, np.asarray(lbA, dtype=np.float64).reshape(1, -1)), ubA=_dev(torch, np.asarray(ubA, dtype=np.float64).reshape(1, -1)))
    return q, _solve(fm, q)


def test_vjp_known_answers(fm, torch_):
    torch = torch_
    rng = np.random.default_rng(11)
    xbar = np.array([0.3, -1.2, 0.8])
    # no active set: gbar = -H^-1 xbar, every bound / row cotangent zero
    M = rng.standard_normal((3, 3)); H = M @ M.T + 3 * np.eye(3)
    q, r = _one(fm, torch, H, [0.1, -0.2, 0.3], rng.standard_normal((2, 3)), -10 * np.ones(3), 10 * np.ones(3), [-10, -10], [10, 10])
    o = _vjp(fm, q, r, _dev(torch, xbar[None]))
    assert int(o["status"][0]) == 0
    assert _rel(_np(o["g"][0]), -np.linalg.solve(H, xbar)) <= 1e-12
    assert not np.any(_np(o["lb"])) and not np.any(_np(o["ub"])) and not np.any(_np(o["lbA"])) and not np.any(_np(o["ubA"]))
    # a full vertex (one row, one bound): gbar = 0, bbar = A^-T xbar
    xb2 = np.array([0.7, -0.4])
    q, r = _one(fm, torch, np.eye(2), [-5.0, 3.0], [[1.0, 1.0]], [-10.0, -1.0], [10.0, 10.0], [-100.0], [1.0])
    assert np.allclose(_np(r["x"][0]), [2.0, -1.0])
    o = _vjp(fm, q, r, _dev(torch, xb2[None]))
    assert int(o["status"][0]) == 0
    assert np.max(np.abs(_np(o["g"][0]))) <= 1e-14
    Ahat = np.array([[1.0, 1.0], [0.0, 1.0]])
    mu = np.linalg.solve(Ahat.T, xb2)
    assert abs(float(o["ubA"][0, 0]) - mu[0]) <= 1e-13 and abs(float(o["lb"][0, 1]) - mu[1]) <= 1e-13
    assert float(o["lbA"][0, 0]) == 0.0 and float(o["ub"][0, 1]) == 0.0 and float(o["lb"][0, 0]) == 0.0
    # bounds only (nC = 0)
    q, r = _one(fm, torch, np.diag([2.0, 3.0, 4.0]), [-4.0, 9.0, 0.0], None, -np.ones(3), np.ones(3), np.zeros(0), np.zeros(0))
    assert np.allclose(_np(r["x"][0]), [1.0, -1.0, 0.0])
    o = _vjp(fm, q, r, _dev(torch, xbar[None]))
    assert int(o["status"][0]) == 0
    assert np.allclose(_np(o["g"][0]), [0.0, 0.0, -xbar[2] / 4.0], rtol=0, atol=1e-15)
    assert np.allclose(_np(o["ub"][0]), [xbar[0], 0, 0], rtol=0, atol=1e-15) and np.allclose(_np(o["lb"][0]), [0, xbar[1], 0], rtol=0, atol=1e-15)
    # forward exit flag != 0: status -2, zeros
    r2 = dict(r)
    r2["exitflag"] = torch.ones_like(r["exitflag"])
    o = _vjp(fm, q, r2, _dev(torch, xbar[None]), want_H=True)
    assert int(o["status"][0]) == -2 and not np.any(_np(o["g"])) and not np.any(_np(o["H"])) and not np.any(_np(o["ub"]))
    # the interior-point iterate (polished <= 0) still gets the rule's working set, with status 2
    r3 = dict(r)
    r3["polished"] = torch.zeros_like(r["polished"])
    o = _vjp(fm, q, r3, _dev(torch, xbar[None]))
    assert int(o["status"][0]) == 2 and np.allclose(_np(o["g"][0]), [0.0, 0.0, -xbar[2] / 4.0], rtol=0, atol=1e-15)


def test_qp_function_gradients_equal_the_vjp(fm, torch_, track):
    torch = torch_
    q, r = _problem(fm, torch, track, 0, 40, 64)
    rng = np.random.default_rng(5)
    cx = _dev(torch, rng.standard_normal(q["g"].shape))
    cf = _dev(torch, rng.standard_normal(q["g"].shape[0]))
    leaves = {key: q[key].clone().requires_grad_(True) for key in ("H", "g", "A", "lb", "ub", "lbA", "ubA")}
    status = torch.empty(q["g"].shape[0], dtype=torch.int32, device="cuda")
    x, fval, flag, pol = fm.QpFunction.apply(leaves["H"], leaves["g"], leaves["A"], leaves["lb"], leaves["ub"], leaves["lbA"],
                                             leaves["ubA"], None, status)
    assert torch.equal(x, r["x"]) and torch.equal(flag, r["exitflag"])
    loss = (x * cx).sum() + (fval * cf).sum()
    loss.backward()
    ref = _vjp(fm, q, r, cx, cf, want_H=True, want_A=True)
    assert torch.equal(status, ref["status"])
    for key in leaves:
        assert torch.equal(leaves[key].grad, ref[key]), key


def test_vjp_instances_are_isolated_and_deterministic(fm, torch_, track):
    torch = torch_
    B = 4096
    q, r = _problem(fm, torch, track, 0, 40, B)
    rng = np.random.default_rng(9)
    xbar = _dev(torch, rng.standard_normal(q["g"].shape))
    o1 = _vjp(fm, q, r, xbar)
    o2 = _vjp(fm, q, r, xbar)
    for key in ("g", "lb", "ub", "lbA", "ubA", "status"):
        assert torch.equal(o1[key], o2[key]), key
    for j in (0, 1, 2047, 4095):
        qj = {key: v[j:j + 1].contiguous() for key, v in q.items()}
        rj = {key: (v[j:j + 1].contiguous() if v is not None and hasattr(v, "shape") and v.dim() >= 1 and v.shape[0] == B else v)
              for key, v in r.items()}
        oj = _vjp(fm, qj, rj, xbar[j:j + 1].contiguous())
        for key in ("g", "lb", "ub", "lbA", "ubA", "status"):
            assert torch.equal(oj[key][0], o1[key][j]), (j, key)
    st = _np(o1["status"])
    assert (st >= 0).sum() >= B // 2, np.unique(st, return_counts=True)
