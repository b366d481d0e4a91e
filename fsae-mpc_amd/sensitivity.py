"""Sensitivities of the batched QP solve on the MI355X: the reverse-mode counterpart of the reference's
qpOASES_sequence('e', ...) (optimizers/matlab/qpOASES/qpOASES_sequence.m:64), batched over instances and run by the HIP
kernel of csrc/qp_sens.hip (fsaempc_qp_vjp_batch_device).

qp_vjp() maps cotangents of (x, fval) of solved QPs to cotangents of the data (g, lb, ub, lbA, ubA, optionally H and A);
QpFunction is the torch.autograd.Function over (H, g, A, lb, ub, lbA, ubA) -> (x, fval) whose backward runs that kernel.
For the LTV-MPC step (x_lin, u_lin fixed): ltv_step_lambda() is the fused step that also returns its QP's multipliers,
ltv_step_vjp() maps cotangents of (u_opt, x_opt, slack, fval) to x0 and x_ref (fsaempc_ltv_step_vjp_batch_device),
LtvStepFunction / ltv_step_diff() make the step differentiable in x0 and x_ref, and feedback_gain() is the local feedback law
d u_opt[:2] / d x0 as two VJP columns.
Per-instance statuses (0 vertex, 1 weakly active side kept, 2 interior-point iterate, -1 singular, -2 forward failed) are
returned with the results and never raised; instances with a negative status get zero cotangents."""
import ctypes as C

import torch

from ._lib import LtvVjpIO, QpAux, QpDesc, QpVjpIO, check, default_opts, lib
from .qpoases import qp_solve_batch_device

STATUS = {0: "vertex", 1: "weakly active side kept", 2: "interior-point iterate", -1: "singular / not converged", -2: "forward failed"}


def qp_vjp(H, g, A, lb, ub, lbA, ubA, x, lam, exitflag, polished, xbar, fbar=None, want_H=False, want_A=False,
           shared_HA=False, options=None, workspace=None, stream=None):
    """Vector-Jacobian product of the solve of B QPs (device tensors in the layout of qp_solve_batch_device: H (B,nV,nV),
    A (B,nV,nC), vectors (B,*); with shared_HA, H (nV,nV) and A (nV,nC) once).  x, lam (B,nV+nC), exitflag, polished: the
    forward's outputs (want_lambda=True, want_aux=True); polished may be None (every instance counts as unrefined).
    xbar: (B,nV) or (B,k,nV) cotangent columns of x; fbar: None, (B,) or (B,k) of fval.
    Returns dict(g, lb, ub, lbA, ubA [, H, A], status): cotangents shaped like xbar's columns ((B,nV) / (B,k,nV), (B,nC) ...),
    H (B[,k],nV,nV), A (B[,k],nV,nC), status (B,) int32."""
    B, nV = g.shape
    nC = lbA.shape[1] if lbA is not None and lbA.dim() == 2 else 0
    dev = g.device
    cols = xbar.dim() == 3
    xb = (xbar if cols else xbar.unsqueeze(1)).contiguous()
    k = xb.shape[1]
    if tuple(xb.shape) != (B, k, nV):
        raise ValueError("xbar must be (B, nV) or (B, k, nV)")
    fb = None
    if fbar is not None:
        fb = (fbar if fbar.dim() == 2 else fbar.reshape(B, 1)).contiguous()
        if tuple(fb.shape) != (B, k):
            raise ValueError("fbar must be (B,) or (B, k) matching xbar")
    for t in (H, g, A, lb, ub, lbA, ubA, x, lam, xb, fb):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError("device tensors must be contiguous float64 on the GPU")
    for t in (exitflag, polished):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or not t.is_cuda or tuple(t.shape) != (B,)):
            raise ValueError("exitflag / polished must be contiguous int32 (B,) tensors on the GPU")
    desc = QpDesc(nV, nC, B, 1 if shared_HA else 0)
    need = lib().fsaempc_qp_vjp_workspace_bytes(C.byref(desc))
    if need < 0:
        check(int(need), "fsaempc_qp_vjp_workspace_bytes")
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((max(need, 8) + 7) // 8, dtype=torch.float64, device=dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    out = dict(g=f64(B, k, nV), lb=f64(B, k, nV), ub=f64(B, k, nV), lbA=f64(B, k, nC), ubA=f64(B, k, nC),
               status=torch.empty(B, dtype=torch.int32, device=dev))
    if want_H:
        out["H"] = f64(B, k, nV, nV)
    if want_A:
        out["A"] = f64(B, k, nV, nC)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None
    io = QpVjpIO(P(xb), P(fb), P(out["g"]), P(out["lb"]), P(out["ub"]), P(out["lbA"]), P(out["ubA"]), P(out.get("H")), P(out.get("A")))
    opts = options if options is not None else default_opts()
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    rc = lib().fsaempc_qp_vjp_batch_device(C.byref(desc), k, P(H), P(g), P(A), P(lb), P(ub), P(lbA), P(ubA), P(x), P(lam),
                                           P(exitflag), P(polished), C.byref(opts), C.byref(io), P(out["status"]), P(workspace),
                                           C.c_longlong(workspace.numel() * 8), C.c_void_p(st))
    check(rc, "fsaempc_qp_vjp_batch_device")
    if not cols:
        for key in ("g", "lb", "ub", "lbA", "ubA", "H", "A"):
            if key in out:
                out[key] = out[key][:, 0]
    return out


class QpFunction(torch.autograd.Function):
    """(H, g, A, lb, ub, lbA, ubA) -> (x, fval, exitflag, polished) of the batched GPU solve (layout of qp_solve_batch_device);
    x and fval are differentiable, the backward runs the VJP kernel.  `status_out` (optional (B,) int32 device tensor) receives
    the VJP's per-instance status when the backward runs; instances with a negative status get zero gradients."""

    @staticmethod
    def forward(ctx, H, g, A, lb, ub, lbA, ubA, options=None, status_out=None):
        H, g, A, lb, ub, lbA, ubA = (t.detach().contiguous() for t in (H, g, A, lb, ub, lbA, ubA))
        r = qp_solve_batch_device(H, g, A, lb, ub, lbA, ubA, options=options, want_lambda=True, want_aux=True)
        ctx.save_for_backward(H, g, A, lb, ub, lbA, ubA, r["x"], r["lam"], r["exitflag"], r["polished"])
        ctx.options, ctx.status_out = options, status_out
        ctx.mark_non_differentiable(r["exitflag"], r["polished"])
        return r["x"], r["fval"], r["exitflag"], r["polished"]

    @staticmethod
    def backward(ctx, gx, gf, _gflag, _gpol):
        H, g, A, lb, ub, lbA, ubA, x, lam, flag, pol = ctx.saved_tensors
        xbar = gx.contiguous() if gx is not None else torch.zeros_like(x)
        fbar = gf.contiguous() if gf is not None else None
        need = ctx.needs_input_grad
        r = qp_vjp(H, g, A, lb, ub, lbA, ubA, x, lam, flag, pol, xbar, fbar, want_H=need[0], want_A=need[2], options=ctx.options)
        if ctx.status_out is not None:
            ctx.status_out.copy_(r["status"])
        return r.get("H"), r["g"], r.get("A"), r["lb"], r["ub"], r["lbA"], r["ubA"], None, None


def _no_params(batch, what):
    """The affine maps and the VJP kernels carry the reference's constants: refuse a batch with a parameter block instead of
    differentiating a different problem."""
    if getattr(batch, "params", None) is not None:
        raise NotImplementedError("%s is not available for an LtvBatch with a parameter block (set_params(None) first)" % what)
    blk = getattr(batch, "blocking", None)
    if blk is not None and not blk.trivial:   # the same holds for move blocking: the maps and the VJP chain are those of the unblocked build
        raise NotImplementedError("%s is not available for an LtvBatch with move blocking (blocking=None, or one step per block)" % what)
    if getattr(batch, "corridor", None) is not None:   # and for a corridor: the row shifts of the chain are those of the constant width
        raise NotImplementedError("%s is not available for an LtvBatch with a corridor (corridor=None)" % what)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _stream(batch, stream):
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(batch.device).cuda_stream)


def ltv_step_lambda(batch, x0, x_ref, x_lin, u_lin, stream=None):
    """The fused step of `batch` (an LtvBatch) that also returns its QP's multipliers: dict(u_opt, x_opt, slack, fval, exitflag, iter,
    kkt, polished, lam (B, nV+nC)).  u_opt, x_opt, fval are those of LtvBatch.step on the same inputs."""
    _no_params(batch, "ltv_step_lambda")
    B = batch.batch
    need = lib().fsaempc_ltv_workspace_bytes(C.byref(batch.desc))
    if need < 0:
        check(int(need), "fsaempc_ltv_workspace_bytes")
    if batch._ws is None or batch._ws.numel() * 8 < need:
        batch._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=batch.device)
    f64 = lambda *s_: torch.empty(s_, dtype=torch.float64, device=batch.device)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=batch.device)
    out = dict(u_opt=f64(B, 2 * batch.N), x_opt=f64(B, batch.nx * batch.N), slack=f64(B, batch.ns), fval=f64(B), exitflag=i32(B), iter=i32(B),
               kkt=f64(B), polished=i32(B), lam=f64(B, batch.nV + batch.nC))
    aux = QpAux(_ptr(out["kkt"]), _ptr(out["polished"]), None, None)
    P = _ptr
    rc = lib().fsaempc_ltv_step_batch_device_lambda(C.byref(batch.desc), C.byref(batch.sp), P(x0), P(x_ref), P(x_lin), P(u_lin), C.byref(batch.opts),
                                                    P(out["u_opt"]), P(out["x_opt"]), P(out["slack"]), P(out["fval"]), P(out["exitflag"]),
                                                    P(out["iter"]), P(out["lam"]), C.byref(aux), P(batch._ws), C.c_longlong(batch._ws.numel() * 8),
                                                    _stream(batch, stream))
    check(rc, "fsaempc_ltv_step_batch_device_lambda")
    return out


def ltv_step_affine_maps(batch, x_lin, u_lin, stream=None):
    """Abar (B, nx, nx N) and Crow (B, nx, nC): the memory of the column-major nx N x nx and nC x nx matrices of
    fsaempc_ltv_affine_maps_batch_device (Abar[b, j, e] = d pred_e / d x0_j; Crow[b, j, r] = coefficient of row r on state j)."""
    _no_params(batch, "ltv_step_affine_maps")
    B = batch.batch
    Abar = torch.empty((B, batch.nx, batch.nx * batch.N), dtype=torch.float64, device=batch.device)
    Crow = torch.empty((B, batch.nx, batch.nC), dtype=torch.float64, device=batch.device)
    rc = lib().fsaempc_ltv_affine_maps_batch_device(C.byref(batch.desc), C.byref(batch.sp), _ptr(x_lin), _ptr(u_lin), _ptr(Abar), _ptr(Crow),
                                                    _stream(batch, stream))
    check(rc, "fsaempc_ltv_affine_maps_batch_device")
    return Abar, Crow


def ltv_step_vjp(batch, fwd, x0, x_ref, x_lin, u_lin, ubar=None, xbar=None, sbar=None, fbar=None, want_xref=True, stream=None):
    """VJP of the step in x0 and x_ref.  fwd: the dict of ltv_step_lambda on the same inputs.  Cotangents (B, 2N) / (B, nx N) / (B, ns)
    / (B,) for one column, or with a column axis (B, k, *) / (B, k); None = 0.  Returns dict(x0 (B[,k],nx), x_ref (B[,k],nx N), status)."""
    _no_params(batch, "ltv_step_vjp")
    B, N, nx = batch.batch, batch.N, batch.nx
    given = [t for t in (ubar, xbar, sbar) if t is not None]
    cols = bool(given) and given[0].dim() == 3 or (fbar is not None and fbar.dim() == 2)
    k = (given[0].shape[1] if given else fbar.shape[1]) if cols else 1
    shape = lambda t, n: None if t is None else t.reshape(B, k, n).contiguous()
    ub, xb, sb = shape(ubar, 2 * N), shape(xbar, nx * N), shape(sbar, batch.ns)
    fb = None if fbar is None else fbar.reshape(B, k).contiguous()
    for t in (x0, x_ref, x_lin, u_lin, ub, xb, sb, fb):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError("device tensors must be contiguous float64 on the GPU")
    need = lib().fsaempc_ltv_step_vjp_workspace_bytes(C.byref(batch.desc), k)
    if need < 0:
        check(int(need), "fsaempc_ltv_step_vjp_workspace_bytes")
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=batch.device)
    out = dict(x0=torch.empty((B, k, nx), dtype=torch.float64, device=batch.device),
               x_ref=torch.empty((B, k, nx * N), dtype=torch.float64, device=batch.device) if want_xref else None,
               status=torch.empty(B, dtype=torch.int32, device=batch.device))
    io = LtvVjpIO(_ptr(ub), _ptr(xb), _ptr(sb), _ptr(fb), _ptr(out["x0"]), _ptr(out["x_ref"]))
    P = _ptr
    rc = lib().fsaempc_ltv_step_vjp_batch_device(C.byref(batch.desc), C.byref(batch.sp), k, P(x0), P(x_ref), P(x_lin), P(u_lin),
                                                 P(fwd["u_opt"]), P(fwd["slack"]), P(fwd["lam"]), P(fwd["exitflag"]), P(fwd["polished"]),
                                                 C.byref(batch.opts), C.byref(io), P(out["status"]), P(ws), C.c_longlong(ws.numel() * 8),
                                                 _stream(batch, stream))
    check(rc, "fsaempc_ltv_step_vjp_batch_device")
    if not cols:
        out["x0"] = out["x0"][:, 0]
        if want_xref:
            out["x_ref"] = out["x_ref"][:, 0]
    return out


class LtvStepFunction(torch.autograd.Function):
    """(x0, x_ref) -> (u_opt, x_opt, slack, fval, exitflag, polished) of the LTV-MPC step of `batch` at fixed (x_lin, u_lin);
    u_opt, x_opt, slack and fval are differentiable in x0 and x_ref, the backward runs fsaempc_ltv_step_vjp_batch_device.
    `status_out` (optional (B,) int32 device tensor) receives the VJP's status; a negative status gives zero gradients."""

    @staticmethod
    def forward(ctx, batch, x0, x_ref, x_lin, u_lin, status_out=None):
        _no_params(batch, "LtvStepFunction")
        x0, x_ref, x_lin, u_lin = (t.detach().contiguous() for t in (x0, x_ref, x_lin, u_lin))
        fwd = ltv_step_lambda(batch, x0, x_ref, x_lin, u_lin)
        ctx.batch, ctx.fwd, ctx.status_out = batch, fwd, status_out
        ctx.save_for_backward(x0, x_ref, x_lin, u_lin)
        ctx.mark_non_differentiable(fwd["exitflag"], fwd["polished"])
        return fwd["u_opt"], fwd["x_opt"], fwd["slack"], fwd["fval"], fwd["exitflag"], fwd["polished"]

    @staticmethod
    def backward(ctx, gu, gx, gs, gf, _gflag, _gpol):
        x0, x_ref, x_lin, u_lin = ctx.saved_tensors
        c = lambda t: None if t is None else t.contiguous()
        r = ltv_step_vjp(ctx.batch, ctx.fwd, x0, x_ref, x_lin, u_lin, c(gu), c(gx), c(gs), c(gf), want_xref=ctx.needs_input_grad[2])
        if ctx.status_out is not None:
            ctx.status_out.copy_(r["status"])
        xr = r["x_ref"].reshape(x_ref.shape) if r["x_ref"] is not None else None
        return None, r["x0"].reshape(x0.shape), xr, None, None, None


def ltv_step_diff(batch, x0, x_ref, x_lin, u_lin, status_out=None):
    """The LTV-MPC step of `batch`, differentiable in x0 and x_ref: (u_opt, x_opt, slack, fval, exitflag, polished)."""
    return LtvStepFunction.apply(batch, x0, x_ref, x_lin, u_lin, status_out)


def feedback_gain(batch, x0, x_ref, x_lin, u_lin):
    """The local feedback law of the step: K (B, 2, nx) = d u_opt[:2] / d x0 (the first step's two inputs), as two VJP columns, and
    the per-instance status (B,) (negative: K is zero)."""
    _no_params(batch, "feedback_gain")
    B = batch.batch
    fwd = ltv_step_lambda(batch, x0, x_ref, x_lin, u_lin)
    ubar = torch.zeros((B, 2, 2 * batch.N), dtype=torch.float64, device=batch.device)
    ubar[:, 0, 0] = 1.0
    ubar[:, 1, 1] = 1.0
    r = ltv_step_vjp(batch, fwd, x0, x_ref, x_lin, u_lin, ubar=ubar, want_xref=False)
    return r["x0"], r["status"]
