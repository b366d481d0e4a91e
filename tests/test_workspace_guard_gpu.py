"""Every entry of the C ABI that takes a caller's workspace stays inside the size its *_workspace_bytes function reports.  Each case
allocates the reported size plus 4 KiB, fills the whole buffer -- the tail with it -- with 0xFF bytes (every double in it is a NaN with
all bits set), and then (1) passes one byte less than the reported size: the entry refuses with "workspace too small" and has written
nothing, neither to the buffer nor to an output; (2) passes exactly the reported size: the entry succeeds, every exit flag and every
SQP status is 0 (the VJPs: their own status, see below) and the tail is bit for bit what it was.  The shapes are the smallest that use every
array of a layout: both models at N = 6, batch 3, the instances tests/test_abi_paths_cpu.py vets on the oracle; racing lines with
N_c = 8, N_s = 16 and two plans on fsg2019 (tests/corridor_cells_cases.py: "both minima"); the plain QP solve and its VJP on the QPs of
the kinematic N = 6 step (13 x 36, one-wavefront kernel) and of the dynamic N = 60 step (124 x 1200, workgroup kernel).

A QP VJP status is 0, 1 or 2 for a derivative that was formed and negative for one that was not (include/fsaempc.h): asserted >= 0."""
import ctypes as C

import numpy as np
import pytest

import corridor_cells_cases as cases
from test_abi_paths_cpu import BLOCKED, DT, N0 as N, B0 as B, SEED

pytestmark = pytest.mark.gpu

TAIL = 4096
SENT = 7            # what every output holds before a call
TOO_SMALL = (-5, "workspace too small")
N_S, N_C, PLANS = 16, 8, 2
MARGIN, V_CAP, GRIP = cases.MARGIN, 20.0, 1.0


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd as fm
    return fm, torch, fm.Track.load("fsg2019")


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def outputs(torch, **shapes):
    """name -> count (float64) or (count, "i") (int32), every entry SENT"""
    mk = lambda n, dt: torch.full((n,), SENT, dtype=dt, device="cuda:0")
    return {k: mk(v[0], torch.int32) if isinstance(v, tuple) else mk(v, torch.float64) for k, v in shapes.items()}


def guarded(env, need, call, out):
    """call(workspace pointer, bytes) -> rc; returns after the two calls of the module's docstring, the device idle"""
    fm, torch, _ = env
    assert need > 0, need
    buf = torch.full((need + TAIL,), 0xFF, dtype=torch.uint8, device="cuda:0")
    rc = call(p(buf), C.c_longlong(need - 1))
    torch.cuda.synchronize()
    assert (rc, fm.lib().fsaempc_last_error().decode()) == TOO_SMALL
    assert bool((buf == 0xFF).all()) and all(bool((v == SENT).all()) for v in out.values()), "a refused call wrote"
    rc = call(p(buf), C.c_longlong(need))
    torch.cuda.synchronize()
    assert rc == 0, (rc, fm.lib().fsaempc_last_error())
    assert bool((buf[need:] == 0xFF).all()), "the entry wrote past the size it reports"
    assert not bool((buf[:need] == 0xFF).all())   # (it did use the workspace)


def all_zero(t):
    return bool((t == 0).all())


class Ltv:
    """descriptor, spline and instances of one model at N = 6, batch 3 (or N = 60 for the workgroup-kernel QPs)"""

    def __init__(self, env, model, horizon=N, seed=SEED):
        fm, torch, tr = env
        self.model, self.N = model, horizon
        self.nx, self.ns, self.nV, self.nC = fm.dims(model, horizon)
        self.mpc = fm.LtvBatch(model, horizon, DT, tr, B)
        self.desc, self.sp = C.byref(self.mpc.desc), C.byref(self.mpc.sp)
        x0, xl, ul, xr = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in fm.instances(model, horizon, DT, tr.L, seed, range(B))]
        self.x0, self.xl, self.ul, self.xr = x0, xl, ul, xr
        self.ins = [p(t) for t in (x0, xr, xl, ul)]

    def step_outputs(self, torch):
        return outputs(torch, u_opt=B * 2 * self.N, x_opt=B * self.nx * self.N, slack=B * self.ns, fval=B, exitflag=(B, "i"), iter=(B, "i"))


STEP_KEYS = ("u_opt", "x_opt", "slack", "fval", "exitflag", "iter")


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
@pytest.mark.parametrize("blocked", [False, True], ids=["plain", "blocked"])
def test_ltv_step(env, model, blocked):
    fm, torch, _ = env
    L, c = fm.lib(), Ltv(env, model)
    out = c.step_outputs(torch)
    if blocked:
        blk = fm._lib.Blocking(BLOCKED, N)
        need = L.fsaempc_ltv_workspace_bytes_b(c.desc, blk.ref())
        call = lambda ws, n: L.fsaempc_ltv_step_batch_device_b(c.desc, c.sp, None, blk.ref(), *c.ins, None, *[p(out[k]) for k in STEP_KEYS], None, None, ws, n, None)
    else:
        need = L.fsaempc_ltv_workspace_bytes(c.desc)
        call = lambda ws, n: L.fsaempc_ltv_step_batch_device(c.desc, c.sp, *c.ins, None, *[p(out[k]) for k in STEP_KEYS], ws, n, None)
    guarded(env, need, call, out)
    assert all_zero(out["exitflag"]), out["exitflag"]


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_ltv_step_vjp(env, model):
    fm, torch, _ = env
    L, c, k = fm.lib(), Ltv(env, model), 2
    fwd = fm.ltv_step_lambda(c.mpc, c.x0, c.xr, c.xl, c.ul)
    torch.cuda.synchronize()
    assert all_zero(fwd["exitflag"])
    ubar = torch.ones(B * k * 2 * N, dtype=torch.float64, device="cuda:0")
    out = outputs(torch, x0bar=B * k * c.nx, xrefbar=B * k * c.nx * N, status=(B, "i"))
    io = fm._lib.LtvVjpIO(p(ubar), None, None, None, p(out["x0bar"]), p(out["xrefbar"]))
    need = L.fsaempc_ltv_step_vjp_workspace_bytes(c.desc, k)
    call = lambda ws, n: L.fsaempc_ltv_step_vjp_batch_device(c.desc, c.sp, k, *c.ins, p(fwd["u_opt"]), p(fwd["slack"]), p(fwd["lam"]), p(fwd["exitflag"]),
                                                             p(fwd["polished"]), None, C.byref(io), p(out["status"]), ws, n, None)
    guarded(env, need, call, out)
    assert bool((out["status"] >= 0).all()), out["status"]


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_sqp(env, model):
    fm, torch, _ = env
    L, c = fm.lib(), Ltv(env, model)
    out = outputs(torch, u_opt=B * 2 * N, x_opt=B * c.nx * N, slack=B * c.ns, fval=B, status=(B, "i"), sweeps=(B, "i"))
    need = L.fsaempc_sqp_workspace_bytes(c.desc)
    call = lambda ws, n: L.fsaempc_sqp_batch_device(c.desc, c.sp, p(c.x0), p(c.xr), p(c.ul), None, None,
                                                    *[p(out[k]) for k in ("u_opt", "x_opt", "slack", "fval", "status", "sweeps")], None, ws, n, None)
    guarded(env, need, call, out)
    print("SQP status", out["status"].tolist(), "sweeps", out["sweeps"].tolist())
    assert all_zero(out["status"]), out["status"]


def _line(env, orc, otrack):
    fm, torch, tr = env
    xP, yP = tr.device(torch.device("cuda:0"))
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    cor = fm.Corridor.from_table(*cases.corridor(orc, otrack, N_S, "kappa"), tr.L)
    out = outputs(torch, line=PLANS * N_C, flag=(PLANS, "i"), table=PLANS * N_S * 8, t=PLANS * N_S)
    head = lambda *mid: (1, C.byref(sp), C.c_double(tr.L), None, *mid, PLANS, N_S, N_C, C.c_double(MARGIN), C.c_double(V_CAP), C.c_double(GRIP), None)
    res = [p(out[k]) for k in ("line", "flag", "table", "t")]
    return (xP, yP, sp), cor, out, head, res


@pytest.mark.parametrize("entry", ["plain", "corridor", "cells"])
def test_raceline(env, orc, otrack, entry):
    fm, torch, tr = env
    L = fm.lib()
    keep, cor, out, head, res = _line(env, orc, otrack)
    if entry == "plain":
        need = L.fsaempc_plan_raceline_workspace_bytes(PLANS, N_C)
        call = lambda ws, n: L.fsaempc_plan_raceline_batch_device(*head(), *res, ws, n, None)
    elif entry == "corridor":
        need = L.fsaempc_plan_raceline_workspace_bytes(PLANS, N_C)
        call = lambda ws, n: L.fsaempc_plan_raceline_batch_device_c(*head(cor.ref()), *res, ws, n, None)
    else:
        out.update(outputs(torch, row_lambda=PLANS * N_S))
        need = L.fsaempc_plan_raceline_cells_workspace_bytes(PLANS, N_S, N_C)
        call = lambda ws, n: L.fsaempc_plan_raceline_cells_batch_device(*head(cor.ref()), *res, p(out["row_lambda"]), ws, n, None)
    guarded(env, need, call, out)
    assert all_zero(out["flag"]), out["flag"]
    assert not bool(torch.isnan(out["table"]).any())


def test_minlap(env, orc, otrack):
    fm, torch, tr = env
    L, iters, n_rho = fm.lib(), 1, 2
    keep, cor, out, head, res = _line(env, orc, otrack)
    out.update(outputs(torch, lap=PLANS * (iters + 1), step=(PLANS * iters, "i")))
    rho = (C.c_double * n_rho)(1e3, 100.0)
    need = L.fsaempc_plan_minlap_workspace_bytes(PLANS, N_C, n_rho)
    call = lambda ws, n: L.fsaempc_plan_minlap_batch_device(*head(), iters, rho, n_rho, None, None, None, *res, p(out["lap"]), p(out["step"]), ws, n, None)
    guarded(env, need, call, out)
    assert all_zero(out["flag"]), out["flag"]
    assert not bool(torch.isnan(out["lap"]).any())


@pytest.mark.parametrize("model,horizon,seed", [(0, 6, SEED), (1, 60, 20190)], ids=["13x36-wavefront", "124x1200-workgroup"])
def test_qp_solve_and_vjp(env, model, horizon, seed):
    """(dynamic N = 60 at seed 20190: the instances the smoke run solves with exit flag 0)"""
    fm, torch, _ = env
    L, c = fm.lib(), Ltv(env, model, horizon, seed)
    nV, nC, nx = c.nV, c.nC, c.nx
    assert (nV, nC) == ((13, 36) if model == 0 else (124, 1200))
    lay = (C.c_int * 4)()
    desc = fm._lib.QpDesc(nV, nC, B, 0)
    assert L.fsaempc_qp_layout(C.byref(desc), -1, lay) == 0 and lay[3] == (1 if model == 0 else 0)
    q = {k: torch.empty(B * n, dtype=torch.float64, device="cuda:0")
         for k, n in zip(("H", "g", "A", "lb", "ub", "lbA", "ubA", "pred", "Bt", "const"), (nV * nV, nV, nC * nV, nV, nV, nC, nC, nx * horizon, nx * horizon * nV, 1))}
    assert L.fsaempc_ltv_build_qp_batch_device(c.desc, c.sp, *c.ins, *[p(v) for v in q.values()], None) == 0, L.fsaempc_last_error()
    qp = [p(q[k]) for k in ("H", "g", "A", "lb", "ub", "lbA", "ubA")]
    out = outputs(torch, x=B * nV, fval=B, exitflag=(B, "i"), iter=(B, "i"), lam=B * (nV + nC), polished=(B, "i"))
    aux = fm._lib.QpAux(None, p(out["polished"]), None, None)
    need = L.fsaempc_qp_workspace_bytes(C.byref(desc))
    call = lambda ws, n: L.fsaempc_qp_solve_batch_device_aux(C.byref(desc), *qp, None, *[p(out[k]) for k in ("x", "fval", "exitflag", "iter", "lam")],
                                                             C.byref(aux), ws, n, None)
    guarded(env, need, call, out)
    assert all_zero(out["exitflag"]), out["exitflag"]
    k = 1
    xbar = torch.ones(B * k * nV, dtype=torch.float64, device="cuda:0")
    bar = outputs(torch, g=B * k * nV, lb=B * k * nV, ub=B * k * nV, lbA=B * k * nC, ubA=B * k * nC, status=(B, "i"))
    io = fm._lib.QpVjpIO(p(xbar), None, p(bar["g"]), p(bar["lb"]), p(bar["ub"]), p(bar["lbA"]), p(bar["ubA"]), None, None)
    need = L.fsaempc_qp_vjp_workspace_bytes(C.byref(desc))
    call = lambda ws, n: L.fsaempc_qp_vjp_batch_device(C.byref(desc), k, *qp, p(out["x"]), p(out["lam"]), p(out["exitflag"]), p(out["polished"]), None,
                                                       C.byref(io), p(bar["status"]), ws, n, None)
    guarded(env, need, call, bar)
    assert bool((bar["status"] >= 0).all()), bar["status"]
