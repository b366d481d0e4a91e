"""GPU tests of the sensitivities of the LTV-MPC step (fsaempc_ltv_affine_maps_batch_device, fsaempc_ltv_step_batch_device_lambda,
fsaempc_ltv_step_vjp_batch_device; Python ltv_step_lambda / ltv_step_vjp / LtvStepFunction / feedback_gain): the forward with
multipliers against LtvBatch.step, the affine maps against the build, feedback_gain and the step VJP against central differences of
LtvBatch.step in x0 and x_ref, and the autograd wrapper against the VJP."""
import numpy as np
import pytest

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


def _np(t):
    return t.detach().cpu().numpy()


def _setup(fm, torch, tr, model, N, B, seed=20190):
    x0, xl, ul, xr = fm.instances(model, N, DT, tr.L, seed, range(B))
    mpc = fm.LtvBatch(model, N, DT, tr, B)
    flat = lambda a: _dev(torch, np.asarray(a).reshape(B, -1))   # instance-major, each instance column-major (nx x N)
    return mpc, flat(x0), flat(xr), flat(xl), flat(ul)


def _same_ws(f0, f1):
    """Same working set and both refined: the multipliers of a refined vertex are exactly zero off its working set."""
    return (np.sign(_np(f0["lam"])) == np.sign(_np(f1["lam"]))).all(axis=1) & (_np(f1["polished"]) > 0) & (_np(f1["exitflag"]) == 0)


@pytest.mark.parametrize("model,N", [(0, 40), (1, 60)])
def test_forward_with_lambda_matches_the_fused_step(fm, torch_, track, model, N):
    torch = torch_
    mpc, x0, xr, xl, ul = _setup(fm, torch, track, model, N, 64)
    ref = mpc.step(x0, xr, xl, ul, want_aux=True)
    out = fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    for key in ("u_opt", "x_opt", "slack", "fval", "exitflag", "polished"):
        assert torch.equal(out[key], ref[key]), key
    assert torch.isfinite(out["lam"]).all()


@pytest.mark.parametrize("model,N", [(0, 40), (1, 40)])
def test_affine_maps_match_the_build(fm, torch_, track, model, N):
    torch = torch_
    B = 16
    mpc, x0, xr, xl, ul = _setup(fm, torch, track, model, N, B)
    Abar, Crow = fm.ltv_step_affine_maps(mpc, xl, ul)
    Abar, Crow = _np(Abar), _np(Crow)
    q0 = mpc.build_qp(x0, xr, xl, ul)
    nx, nC = mpc.nx, mpc.nC
    rows = np.arange(nC)
    if model == 0:
        step = np.where(rows < 4 * N, rows % N, (rows - 4 * N) % N)
    else:
        step = np.where(rows < 4 * N, rows % N, np.where(rows < 8 * N, ((rows - 4 * N) % (2 * N)) // 2, (rows - 8 * N) // 12))
    for j in range(nx):
        d = 1e-2
        x1 = x0.clone()
        x1[:, j] += d
        q1 = mpc.build_qp(x1, xr, xl, ul)
        dpred = (_np(q1["pred"]) - _np(q0["pred"])) / d
        assert np.abs(dpred - Abar[:, j, :]).max() <= 1e-7 * max(1.0, np.abs(Abar[:, j, :]).max())
        P = Abar[:, j, :].reshape(B, N, nx)
        want = -np.einsum("brj,brj->br", np.transpose(Crow, (0, 2, 1)), P[:, step, :])
        for key in ("lbA", "ubA"):
            base, new = _np(q0[key]), _np(q1[key])
            fin = np.abs(base) < 1e9
            got = (new - base) / d
            assert np.abs(np.where(fin, got - want, 0.0)).max() <= 1e-6 * max(1.0, np.abs(want).max()), key
        assert np.array_equal(_np(q1["H"]), _np(q0["H"])) and np.array_equal(_np(q1["A"]), _np(q0["A"]))


@pytest.mark.parametrize("model,N", [(0, 40), (1, 40)])
def test_feedback_gain_matches_central_differences_of_the_step(fm, torch_, track, model, N):
    check_feedback_gain(fm, torch_, track, model, N, 64)


def check_feedback_gain(fm, torch, track, model, N, B):
    """feedback_gain against central differences of the step in each x0 component, on every instance whose working set holds at
    +-h (tests/test_sens_shapes_gpu.py runs it off N = 40 too).  Returns the figures it asserted on."""
    mpc, x0, xr, xl, ul = _setup(fm, torch, track, model, N, B)
    K, st = fm.feedback_gain(mpc, x0, xr, xl, ul)
    K, st = _np(K), _np(st)
    f0 = fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    n_ok, worst = 0, 0.0
    for j in range(mpc.nx):
        h = 1e-5 * max(1.0, float(_np(x0[:, j].abs()).max()))
        fs, same = [], st == 0
        for s in (1.0, -1.0):
            x1 = x0.clone()
            x1[:, j] += s * h
            f1 = fm.ltv_step_lambda(mpc, x1, xr, xl, ul)
            same &= _same_ws(f0, f1)
            fs.append(_np(f1["u_opt"])[:, :2])
        fd = (fs[0] - fs[1]) / (2 * h)
        err = np.abs(fd - K[:, :, j]).max(axis=1) / np.maximum(1.0, np.abs(K[:, :, j]).max(axis=1))
        worst = max(worst, float(err[same].max()) if same.any() else 0.0)
        assert (err[same] <= 1e-6).all(), (j, np.sort(err[same])[-5:], int(same.sum()))
        n_ok += int(same.sum())
    assert n_ok >= mpc.nx * B // 4, n_ok
    assert (st >= 0).sum() >= B * 9 // 10, np.unique(st, return_counts=True)
    return dict(nV=mpc.nV, compared=n_ok, of=mpc.nx * B, worst=worst, status=dict(zip(*(a.tolist() for a in np.unique(st, return_counts=True)))))


@pytest.mark.parametrize("model,N", [(0, 40), (1, 40)])
def test_step_vjp_matches_directional_differences_in_x0_and_xref(fm, torch_, track, model, N):
    check_step_vjp(fm, torch_, track, model, N, 64)


def check_step_vjp(fm, torch, track, model, N, B):
    """The step VJP against directional differences of the step in x0 and x_ref, on every instance whose working set holds at +-h.
    Returns the figures it asserted on."""
    mpc, x0, xr, xl, ul = _setup(fm, torch, track, model, N, B)
    rng = np.random.default_rng(1)
    cu = rng.standard_normal((B, 2 * N))
    cx = rng.standard_normal((B, mpc.nx * N))
    cf = rng.standard_normal(B) * 1e-3
    f0 = fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    r = fm.ltv_step_vjp(mpc, f0, x0, xr, xl, ul, ubar=_dev(torch, cu), xbar=_dev(torch, cx), fbar=_dev(torch, cf))
    st = _np(r["status"])
    v0 = rng.standard_normal((B, mpc.nx)) * np.maximum(1.0, np.abs(_np(x0)))
    vr = rng.standard_normal((B, mpc.nx * N)) * np.maximum(1.0, np.abs(_np(xr)))
    an = np.einsum("bi,bi->b", _np(r["x0"]), v0) + np.einsum("bi,bi->b", _np(r["x_ref"]), vr)
    h = 1e-6
    vals, same = [], st == 0
    for s in (1.0, -1.0):
        f1 = fm.ltv_step_lambda(mpc, x0 + s * h * _dev(torch, v0), (xr + s * h * _dev(torch, vr)).contiguous(), xl, ul)
        same &= _same_ws(f0, f1)
        vals.append(np.einsum("bi,bi->b", cu, _np(f1["u_opt"])) + np.einsum("bi,bi->b", cx, _np(f1["x_opt"])) + cf * _np(f1["fval"]))
    fd = (vals[0] - vals[1]) / (2 * h)
    err = np.abs(fd - an) / np.maximum(1.0, np.maximum(np.abs(an), np.abs(fd)))
    assert same.sum() >= B // 4, int(same.sum())
    assert (err[same] <= 1e-6).all(), (np.sort(err[same])[-5:], int(same.sum()))
    return dict(nV=mpc.nV, compared=int(same.sum()), of=B, worst=float(err[same].max()),
                status=dict(zip(*(a.tolist() for a in np.unique(st, return_counts=True)))))


def test_ltv_step_function_gradients_equal_the_vjp(fm, torch_, track):
    torch = torch_
    B, N = 32, 40
    mpc, x0, xr, xl, ul = _setup(fm, torch, track, 0, N, B)
    rng = np.random.default_rng(2)
    cu, cx, cf = _dev(torch, rng.standard_normal((B, 2 * N))), _dev(torch, rng.standard_normal((B, mpc.nx * N))), _dev(torch, rng.standard_normal(B))
    a0, ar = x0.clone().requires_grad_(True), xr.clone().requires_grad_(True)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    u, x, s, f, flag, pol = fm.ltv_step_diff(mpc, a0, ar, xl, ul, status)
    ((u * cu).sum() + (x * cx).sum() + (f * cf).sum()).backward()
    f0 = fm.ltv_step_lambda(mpc, x0, xr, xl, ul)
    ref = fm.ltv_step_vjp(mpc, f0, x0, xr, xl, ul, ubar=cu, xbar=cx, fbar=cf)
    assert torch.equal(status, ref["status"])
    assert torch.equal(a0.grad, ref["x0"]) and torch.equal(ar.grad, ref["x_ref"])
