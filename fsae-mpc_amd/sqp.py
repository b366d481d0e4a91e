"""Batched SQP of the nonlinear MPC step (DESIGN.md "Nonlinear MPC: batched SQP"): the LTV-MPC problem with the
rollout of the model as its dynamics, solved per instance by a Gauss-Newton SQP with exact linearisation, a parallel l1-merit line
search and per-instance termination.  All compute runs on the MI355X through libfsaempc.so (fsaempc_sqp_batch_device)."""
import ctypes as C

from ._lib import LtvDesc, ParamBlock, QpOpts, SqpAux, Spline, check, check_blocking, default_opts, lib, sqp_default_opts
from .ltvmpc import dims

STATUS = {0: "converged", 1: "sweep limit", 2: "no step accepted", -1: "QP failed", -2: "QP infeasible", 4: "skipped"}


class SqpBatch:
    """Device-resident batched SQP.  Inputs / outputs are torch tensors on the GPU, laid out as for LtvBatch.step."""

    def __init__(self, model, N, dt, track, batch, device="cuda:0", options=None, integrator=-1, params=None, blocking=None, corridor=None):
        """blocking: accepted for symmetry with LtvBatch, but only the trivial one ([1] * N): the exact build of the NLP has no
        move-blocked form (LtvBatch.sqp re-linearises a blocked batch)."""
        if corridor is not None:   # (accepted for symmetry too: the exact build has no corridor form)
            raise NotImplementedError("SqpBatch (the exact build of the NLP, nlp_build_qp) is not available with a corridor; "
                                      "LtvBatch(..., corridor=...).sqp re-linearises a batch inside a corridor")
        if blocking is not None and len(check_blocking(blocking, N)) != N:
            raise NotImplementedError("SqpBatch (the exact build of the NLP, nlp_build_qp) is not available with move blocking; "
                                      "LtvBatch(..., blocking=...).sqp re-linearises a blocked batch")
        import torch
        self.torch = torch
        self.model, self.N, self.dt, self.batch = model, N, float(dt), batch
        self.device = torch.device(device)
        self.nx, self.ns, self.nV, self.nC = dims(model, N)
        self.track = track
        self.xP, self.yP = track.device(self.device)
        self.sp = Spline(track.M, track.dl, C.c_void_p(self.xP.data_ptr()), C.c_void_p(self.yP.data_ptr()))
        self.desc = LtvDesc(model, N, batch, self.dt, integrator)   # integrator: -1 model default (RK2 kin. / RK4 dyn.), 0 Euler, 1 RK2, 2 RK4
        self.opts = options if options is not None else default_opts()
        self._ws = None
        self.params = None
        self.set_params(params)

    def set_params(self, params):
        """The parameter block of the batch, as for LtvBatch: None, (32,) or (batch, 32); read by the build, the rollouts and the
        line search."""
        self.params = ParamBlock(params, self.batch, self.device) if params is not None else None

    def _f64(self, *shape):
        return self.torch.empty(shape, dtype=self.torch.float64, device=self.device)

    def _check(self, name, t, shape):
        torch = self.torch
        if t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device or t.numel() != shape:
            raise ValueError("%s must be a contiguous float64 tensor of %d elements on %s" % (name, shape, self.device))

    def build_qp(self, x0, x_ref, u_lin, stream=None):
        """The exact QP of the NLP at u_lin (fsaempc_nlp_build_qp_batch_device): H, g, A, lb, ub, lbA, ubA, pred (= the rollout),
        Bt, const."""
        B, nx, N, nV, nC = self.batch, self.nx, self.N, self.nV, self.nC
        q = dict(H=self._f64(B, nV, nV), g=self._f64(B, nV), A=self._f64(B, nV, nC), lb=self._f64(B, nV), ub=self._f64(B, nV),
                 lbA=self._f64(B, nC), ubA=self._f64(B, nC), pred=self._f64(B, N * nx), Bt=self._f64(B, nV, N * nx), const=self._f64(B))
        P = lambda t: C.c_void_p(t.data_ptr())
        out = (P(q["H"]), P(q["g"]), P(q["A"]), P(q["lb"]), P(q["ub"]), P(q["lbA"]), P(q["ubA"]), P(q["pred"]), P(q["Bt"]), P(q["const"]))
        rc = lib().fsaempc_nlp_build_qp_batch_device_p(C.byref(self.desc), C.byref(self.sp), self.params.ref() if self.params is not None else None,
                                                       P(x0), P(x_ref), P(u_lin), *out, self._stream(stream))
        check(rc, "fsaempc_nlp_build_qp_batch_device_p")
        return q

    def _stream(self, stream):
        if stream is None and self.device.type != "cuda":
            return C.c_void_p(None)       # the library reports the missing device: there is no CPU path
        return C.c_void_p(stream if stream is not None else self.torch.cuda.current_stream(self.device).cuda_stream)

    def solve(self, x0, x_ref, u_init, stream=None, skip=None, **sqp_opts):
        """Returns dict(u_opt (B,2N), x_opt (B,nx*N) = rollout of u_opt, slack (B,ns), fval (NLP objective), status, sweeps, lambda
        (B, nV+nC) of the last QP, qp_iter (total interior-point iterations), step_norm, hard_viol, merit (B, max_sweeps)).
        skip: None, or an int32 (B,) device tensor: an instance with a non-zero entry is left out of every sub-batch
        (fsaempc_sqp_batch_device_m): status 4 ("skipped"), sweeps 0, qp_iter 0, u_opt the clamped u_init and x_opt its rollout.
        sqp_opts: fields of fsaempc_sqp_opts (max_sweeps, trials, tol_step, tol_feas, armijo, rho0, warm_start)."""
        torch = self.torch
        B, N, nx = self.batch, self.N, self.nx
        o = sqp_default_opts(**sqp_opts)
        self._check("x0", x0, B * nx)
        self._check("x_ref", x_ref, B * nx * N)
        self._check("u_init", u_init, B * 2 * N)
        if skip is not None and (skip.dtype != torch.int32 or not skip.is_contiguous() or skip.device != self.device or tuple(skip.shape) != (B,)):
            raise ValueError("skip must be a contiguous int32 tensor of shape (%d,) on %s" % (B, self.device))
        need = lib().fsaempc_sqp_workspace_bytes(C.byref(self.desc))
        if need < 0:
            check(int(need), "fsaempc_sqp_workspace_bytes")
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=self.device)
        out = dict(u_opt=self._f64(B, 2 * N), x_opt=self._f64(B, nx * N), slack=self._f64(B, self.ns), fval=self._f64(B),
                   status=i32(B), sweeps=i32(B), **{"lambda": self._f64(B, self.nV + self.nC)}, qp_iter=i32(B),
                   step_norm=self._f64(B), hard_viol=self._f64(B), merit=self._f64(B, o.max_sweeps))
        P = lambda t: C.c_void_p(t.data_ptr())
        aux = SqpAux(P(out["lambda"]), P(out["qp_iter"]), P(out["step_norm"]), P(out["hard_viol"]), P(out["merit"]))
        tail = (C.byref(self.opts), C.byref(o), P(out["u_opt"]), P(out["x_opt"]), P(out["slack"]), P(out["fval"]), P(out["status"]),
                P(out["sweeps"]), C.byref(aux), P(self._ws), C.c_longlong(self._ws.numel() * 8), self._stream(stream))
        rc = lib().fsaempc_sqp_batch_device_m(C.byref(self.desc), C.byref(self.sp), self.params.ref() if self.params is not None else None,
                                              P(x0), P(x_ref), P(u_init), P(skip) if skip is not None else None, *tail)
        check(rc, "fsaempc_sqp_batch_device_m")
        return out


def sqp_timing():
    """Phase times (ms) of the last SqpBatch.solve by device events, summed over its sweeps (needs fsaempc_qp_set_timing(1))."""
    v = [C.c_double() for _ in range(4)]
    check(lib().fsaempc_sqp_get_timing(*[C.byref(x) for x in v]), "fsaempc_sqp_get_timing")
    return dict(build=v[0].value, solve=v[1].value, linesearch=v[2].value, compact=v[3].value)


__all__ = ["SqpBatch", "sqp_timing", "STATUS", "QpOpts"]
