"""Pins tests/dual_numpy.py, the dual-number restatement behind tests/test_exact_build_gpu.py (no GPU): at float64 its kappa, f and
psi against the oracle and the numpy statements the other tests use, its exact Jacobians and linearised rows against central
differences of those statements, and its float64 run against its long-double run on the GPU test's inputs (e64)."""
import numpy as np
import pytest

import dual_numpy as dn
import exact_cases as ec
import nlp_numpy as nn
import param_numpy as pn

DT = ec.DT


@pytest.fixture(scope="module")
def tab():
    return ec.table()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def _states(model, tab):
    """Random states, one on each side of a spline segment boundary, and wrapped arc lengths s < 0 and s > L."""
    rng = np.random.default_rng(3 + model)
    X = np.zeros((12, 5 if model == 0 else 7))
    X[:, 0] = rng.uniform(0, tab.L, 12)
    X[:4, 0] = [7 * tab.dl - 1e-3, 7 * tab.dl + 1e-3, -2.5, tab.L + 4.25]
    X[:, 1], X[:, 2], X[:, 3] = rng.uniform(-0.5, 0.5, 12), rng.uniform(-0.1, 0.1, 12), rng.uniform(5, 20, 12)
    if model == 0:
        X[:, 4] = rng.uniform(-0.1, 0.1, 12)
    else:
        X[:, 4], X[:, 5], X[:, 6] = rng.uniform(-0.2, 0.2, 12), rng.uniform(-0.3, 0.3, 12), rng.uniform(-0.1, 0.1, 12)
    U = np.stack([rng.uniform(-2, 2, 12), rng.uniform(-0.08, 0.08, 12)], 1)
    return X, U


def _block(model, away):
    import fsae_mpc_amd as fm
    return fm.param_draws(model, [5], 17, 0.2)[0] if away else dn.default_block(model)


def test_default_block_is_the_librarys():
    import fsae_mpc_amd as fm
    for model in (0, 1):
        assert np.array_equal(dn.default_block(model), fm.default_params(model))


def test_kappa_matches_the_oracle(orc, otrack, tab):
    s = np.concatenate([np.random.default_rng(1).uniform(-tab.L, 2 * tab.L, 200), [0.0, tab.dl, 7 * tab.dl - 1e-9, 7 * tab.dl + 1e-9, -1e-9, tab.L]])
    err = max(abs(float(dn.kappa(tab, np.float64(v))) - orc.kappa(otrack, float(v))) for v in s)
    print("kappa: max |dual_numpy - oracle| = %.2e" % err)
    assert err <= 1e-13
    # the derivative the dual number carries is kappa'(s): central difference inside a segment
    for v in (3.3, 40.7, -2.5, tab.L + 4.25):
        d = dn.kappa(tab, dn.Dual(np.float64(v), np.float64(1.0))).d
        fd = (orc.kappa(otrack, v + 1e-5) - orc.kappa(otrack, v - 1e-5)) / 2e-5
        assert abs(d - fd) <= 1e-7 * max(1.0, abs(fd)), (v, d, fd)


@pytest.mark.parametrize("model", [0, 1])
def test_f_and_psi_match_the_numpy_statements(orc, otrack, tab, model):
    X, U = _states(model, tab)
    for away in (False, True):
        P = _block(model, away)
        for x, u in zip(X, U):
            f = dn.f_model(P, tab, model, dn._vec(x, np.float64), dn._vec(u, np.float64))
            assert _rel(f, pn.f_model(P, orc, model, otrack, x, u)) <= 1e-13
            if not away:
                assert _rel(f, orc.f_model(model, otrack, x, u)) <= 1e-13
            for integ in (0, 1, 2):
                xn = dn.psi_step(P, tab, model, dn._vec(x, np.float64), dn._vec(u, np.float64), np.float64(DT), integ)
                assert _rel(xn, pn.psi(P, orc, model, otrack, x, u, DT, integ)) <= 1e-13
                if not away:
                    assert _rel(xn, nn.psi(orc, model, otrack, x, u, DT, integ)) <= 1e-13


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_exact_jacobians_match_central_differences(orc, otrack, tab, model, integ):
    """[Ad Bd] of one step against central differences of nlp_numpy.rollout (default block) and param_numpy.rollout (a drawn one)
    at 1e-6; the float64 Jacobians against the long-double ones (the issue's prototype measured 1.0e-14 relative, worst case)."""
    X, U = _states(model, tab)
    nx, h, worst = X.shape[1], 1e-5, 0.0
    for away in (False, True):
        P = _block(model, away)
        step = (lambda x, u: pn.rollout(P, orc, model, otrack, x, u[None], DT, integ)[0]) if away else \
               (lambda x, u: nn.rollout(orc, model, otrack, x, u[None], DT, integ)[0])
        for x, u in zip(X, U):
            xn, Ad, Bd = dn.linearise_exact(P, tab, model, x, u, DT, integ)
            assert _rel(xn, step(x, u)) <= 1e-13
            z = np.concatenate([x, u])
            for c in range(nx + 2):
                zp, zm = z.copy(), z.copy()
                zp[c] += h; zm[c] -= h
                fd = (step(zp[:nx], zp[nx:]) - step(zm[:nx], zm[nx:])) / (2 * h)
                assert _rel(np.concatenate([Ad, Bd], 1)[:, c], fd) <= 1e-6, (away, c)
            _, Al, Bl = dn.linearise_exact(P, tab, model, x, u, DT, integ, np.longdouble)
            worst = max(worst, dn.gap(np.concatenate([Ad, Bd], 1), np.concatenate([Al, Bl], 1)))
    print("model %d integ %d: float64 [Ad Bd] against long double, worst relative gap %.2e" % (model, integ, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("model", [0, 1])
def test_linearised_rows_match_central_differences(tab, model):
    X, U = _states(model, tab)
    P0 = dn.default_block(model)
    nx, h = X.shape[1], 1e-6
    for away in (False, True):
        P = _block(model, away)
        rows = (lambda Z: pn.rows(P, model, Z[:, :nx], Z[:, nx:])) if away else (lambda Z: nn.rows(model, Z[:, :nx], Z[:, nx:]))
        c, Cx, Cu = dn.rows_linearised(P, model, X, U)
        Z = np.concatenate([X, U], 1)
        assert _rel(c, rows(Z)) <= 1e-13
        if not away:
            assert _rel(c, pn.rows(P0, model, X, U)) <= 1e-13
        J = np.concatenate([Cx, Cu], 1)
        for col in range(nx + 2):
            Zp, Zm = Z.copy(), Z.copy()
            Zp[:, col] += h; Zm[:, col] -= h
            fd = (rows(Zp) - rows(Zm)) / (2 * h)
            assert _rel(J[:, col], fd) <= 1e-6, (away, col)
        assert np.array_equal(dn.row_step(model, X.shape[0]).shape, c.shape)


@pytest.mark.parametrize("case", ec.exact_cases(), ids=ec.case_id)
def test_float64_against_long_double_on_the_gpu_tests_inputs(case):
    """e64 per tensor: the relative gap (entry-wise max over the tensor's max-norm) of the float64 run of the restatement to the
    long-double run, on the inputs of tests/test_exact_build_gpu.py.  Largest values over all cases: DESIGN.md 6e-1."""
    ref = ec.reference(*case)
    for k, e in ref["e64"].items():
        print("e64 %-24s %-5s %.2e" % (ec.case_id(case), k, e.max()))
        assert e.max() <= ec.E64_MAX, (k, e)
    assert np.finfo(np.longdouble).eps < 2e-19, "long double is no wider than double on this machine"
