"""s-domain plans: the table the reference's loop is meant to track (main.m:20 makes it with
dynamic_minimum_time_planner, main.m:115 resamples it with obtain_reference).  `Plan.profile` fills one on the device with the
planner stand-in (a quasi-steady-state minimum-time speed profile on the centre line), `Plan.from_table` takes a user's own;
`plan.reference` and ClosedLoop(reference=plan) resample it in time for a batch of cars.  `Plan.raceline` chooses a minimum-curvature
line first and makes the profile on it; `Plan.profile(line=c)` takes a user's own control points.  `Plan.minlap` lowers
the lap time of that profile over the control points from there; `Plan.lap_gradient` is the lap time and its gradient."""
import ctypes as C
import math

import numpy as np

from .corridor import Corridor, check_corridor
from ._lib import (LINE_MAX_NS, LINE_MIN_NC, MAX_NV, MINLAP_MAX_NS, MINLAP_MAX_RHO, MINLAP_RHO, NPAR, PLAN_MAX_NS, ParamBlock, PlanTable, Spline, check,
                   default_opts, lib)


def check_profile_args(N_s, v_cap, grip, n_plans):
    """Validates the arguments of Plan.profile (no library call)."""
    if int(N_s) != N_s or not 2 <= N_s <= PLAN_MAX_NS:
        raise ValueError("N_s must be an integer in 2 .. %d, got %r" % (PLAN_MAX_NS, N_s))
    for name, v in (("v_cap", v_cap), ("grip", grip)):
        if not (isinstance(v, (int, float, np.floating, np.integer)) and math.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, got %r" % (name, v))
    if grip > 1:
        raise ValueError("grip must be <= 1, got %r" % (grip,))
    if int(n_plans) != n_plans or n_plans < 1:
        raise ValueError("n_plans must be an integer >= 1, got %r" % (n_plans,))


def check_line_args(N_s, N_c, margin=None):
    """Validates the cell and control-point counts of a line, and the margin of Plan.raceline (no library call)."""
    if int(N_c) != N_c or not LINE_MIN_NC <= N_c <= MAX_NV:
        raise ValueError("N_c must be an integer in %d .. %d, got %r" % (LINE_MIN_NC, MAX_NV, N_c))
    if int(N_s) != N_s or not 2 * N_c <= N_s <= LINE_MAX_NS:
        raise ValueError("N_s must be an integer in 2 N_c = %d .. %d, got %r" % (2 * N_c, LINE_MAX_NS, N_s))
    if margin is not None and not (isinstance(margin, (int, float, np.floating, np.integer)) and math.isfinite(margin) and margin >= 0):
        raise ValueError("margin must be finite and >= 0, got %r" % (margin,))


def check_minlap_args(N_s, iters, rho):
    """Validates the cell cap, iteration count and ladder of Plan.minlap (no library call); returns the ladder as a tuple of floats."""
    if N_s > MINLAP_MAX_NS:
        raise ValueError("N_s must be <= %d for the minimum-time line, got %r" % (MINLAP_MAX_NS, N_s))
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError("iters must be an integer >= 0, got %r" % (iters,))
    try:
        rho = tuple(float(r) for r in rho)
    except (TypeError, ValueError):
        raise ValueError("rho must be a sequence of numbers")
    if not 1 <= len(rho) <= MINLAP_MAX_RHO:
        raise ValueError("rho must hold 1 .. %d values, got %d" % (MINLAP_MAX_RHO, len(rho)))
    if not all(math.isfinite(r) and r > 0 for r in rho):
        raise ValueError("every rho must be finite and > 0, got %r" % (rho,))
    return rho


def check_params(params, n_plans):
    """Validates the parameter blocks of a planner call against n_plans (no library call); returns (params, n_plans)."""
    if params is None:
        return None, n_plans
    if not hasattr(params, "shape"):
        try:
            params = np.asarray(params, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("params must be an array of %d or (n_plans, %d) numbers" % (NPAR, NPAR))
    shape = tuple(params.shape)
    if len(shape) == 2 and shape[1] == NPAR and shape[0] >= 1 and n_plans in (1, shape[0]):
        n_plans = shape[0]
    elif shape != (NPAR,) or n_plans != 1:
        raise ValueError("params must be (%d,) with n_plans = 1 or (n_plans, %d), got %s with n_plans = %d" % (NPAR, NPAR, shape, n_plans))
    return params, n_plans


def check_line(line, N_s, n_plans):
    """Validates a user's control points, (N_c,) or (P, N_c), against N_s and n_plans (no library call); returns (line, N_c, n_plans)."""
    if not hasattr(line, "shape"):
        try:
            line = np.asarray(line, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("line must be an array of (N_c,) or (n_plans, N_c) numbers")
    shape = tuple(line.shape)
    if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] < 1):
        raise ValueError("line must be (N_c,) or (n_plans, N_c), got %s" % (shape,))
    check_line_args(N_s, shape[-1])
    if len(shape) == 2 and shape[0] != n_plans:
        if n_plans != 1:
            raise ValueError("line holds %d sets of control points, n_plans = %d" % (shape[0], n_plans))
        n_plans = shape[0]
    return line, shape[-1], n_plans


def check_table(table, t, ds):
    """Validates the shapes of a user's plan (no library call); returns (P, N_s).  table: (N_s, 8), (8 N_s,) or (P, N_s, 8);
    t: (N_s,) or (P, N_s)."""
    ts, tt = tuple(table.shape), tuple(t.shape)
    if len(tt) == 1 and len(ts) == 1 and ts[0] == 8 * tt[0]:
        ts = (tt[0], 8)
    if len(tt) == 1 and ts == (tt[0], 8):
        P, N_s = 1, tt[0]
    elif len(tt) == 2 and ts == (tt[0], tt[1], 8):
        P, N_s = tt
    else:
        raise ValueError("plan shapes disagree: table %s (want (N_s, 8) or (P, N_s, 8)), t %s (want (N_s,) or (P, N_s))" % (tuple(table.shape), tt))
    if N_s < 1 or P < 1:
        raise ValueError("an empty plan")
    if not (math.isfinite(ds) and ds > 0):
        raise ValueError("ds must be finite and > 0, got %r" % (ds,))
    return P, N_s


class Plan:
    """P plans of N_s cells on the device: table (P, N_s, 8) = n, mu, x_d, y_d, theta_d, delta, a, delta_d per cell, t (P, N_s)
    traversal times, ds the cell length.  P = 1: shared by every car; otherwise car b drives on plan b."""

    def __init__(self, table, t, ds):
        self.table, self.t, self.ds = table, t, float(ds)
        self.P, self.N_s = int(t.shape[0]), int(t.shape[1])
        self.device = table.device
        self.c = PlanTable(C.c_void_p(table.data_ptr()), C.c_void_p(t.data_ptr()), self.N_s, self.ds, 1 if self.P > 1 else 0)
        self.line, self.line_flag = None, None   # control points of the lateral offset and the flags of their QPs (Plan.raceline)
        self.row_lambda = None                   # multipliers of the cell rows (Plan.raceline(rows="cells", want_row_lambda=True))
        self.control_points, self.lap_history, self.step_history = None, None, None   # Plan.minlap: .line and the record of its iterations

    def ref(self):
        return C.byref(self.c)

    @staticmethod
    def profile(model, track, N_s=500, v_cap=20.0, grip=1.0, params=None, n_plans=1, device="cuda:0", stream=None, line=None):
        """The planner stand-in on the device (fsaempc_plan_profile_batch_device).  params: None (the reference's constants),
        (32,) one car, or (P, 32) one plan per block (n_plans is then P).  line: None (the centre line) or the control points of a
        lateral offset, (N_c,) shared by the plans or (P, N_c) (fsaempc_plan_line_profile_batch_device)."""
        check_profile_args(N_s, v_cap, grip, n_plans)
        if model not in (0, 1):
            raise ValueError("unknown model %r" % (model,))
        params, n_plans = check_params(params, n_plans)
        N_c = 0
        if line is not None:
            line, N_c, n_line = check_line(line, N_s, n_plans)
            if n_line != n_plans:
                if params is not None and len(tuple(params.shape)) == 1:
                    raise ValueError("a shared parameter block makes one plan, line holds %d" % n_line)
                n_plans = n_line
        import torch
        dev = torch.device(device)
        N_s, n_plans = int(N_s), int(n_plans)
        xP, yP = track.device(dev)
        sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        blocks = ParamBlock(params, n_plans, dev) if params is not None else None
        table = torch.empty((n_plans, N_s, 8), dtype=torch.float64, device=dev)
        t = torch.empty((n_plans, N_s), dtype=torch.float64, device=dev)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        if line is None:
            rc = lib().fsaempc_plan_profile_batch_device(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                         n_plans, N_s, C.c_double(v_cap), C.c_double(grip), C.c_void_p(table.data_ptr()),
                                                         C.c_void_p(t.data_ptr()), st)
            check(rc, "fsaempc_plan_profile_batch_device")
        else:
            c = (line if isinstance(line, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(line, dtype=np.float64)))
            c = c.to(device=dev, dtype=torch.float64).contiguous()
            rc = lib().fsaempc_plan_line_profile_batch_device(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                              n_plans, N_s, int(N_c), C.c_void_p(c.data_ptr()), 1 if c.dim() == 2 else 0,
                                                              C.c_double(v_cap), C.c_double(grip), C.c_void_p(table.data_ptr()),
                                                              C.c_void_p(t.data_ptr()), st)
            check(rc, "fsaempc_plan_line_profile_batch_device")
        plan = Plan(table, t, track.L / N_s)
        plan._blocks = blocks   # (read by a launch that may still be queued)
        if line is not None:
            plan.line = c.reshape(-1, int(N_c))
        return plan

    @staticmethod
    def raceline(model, track, N_s=500, N_c=100, margin=0.25, v_cap=20.0, grip=1.0, params=None, n_plans=1, options=None, device="cuda:0",
                 stream=None, corridor=None, rows="points", want_row_lambda=False):
        """Racing-line plans (fsaempc_plan_raceline_batch_device): a minimum-curvature line within +-(N_MAX - margin) of
        the centre line (N_MAX: the block's, default 0.75) as N_c control points of a periodic cubic B-spline, then the profile of
        Plan.profile on it.  Returns a Plan with .line (P, N_c) control points and .line_flag (P,) exit flags of the line QPs; a plan
        whose flag is not 0 is the centre-line plan.  corridor: None, or a Corridor (shared, or one per plan; n_plans is then its count):
        the line stays within [n_lo + margin, n_hi - margin] at every cell (fsaempc_plan_raceline_batch_device_c, DESIGN.md 6l: each
        control point takes the tightest limits of the cells it touches, so a pinch is smeared over four knot spacings).  A plan whose
        corridor leaves a control point no room has flag -1 and is NaN; in a corridor NO plan falls back to the centre line (it may
        lie outside the corridor): every plan whose flag is not 0 is NaN in table, t and line.
        rows: "points" (the default: the box of every control point, as above) or "cells": one constraint row per cell,
        n_lo(s_i) + margin <= n_i <= n_hi(s_i) - margin, with free control points (fsaempc_plan_raceline_cells_batch_device).  The
        line then uses the width of every single cell, and its control points may lie outside the corridor; it is inside the corridor
        at the N_s cells, not between them.  "cells" needs a corridor (Corridor.constant(L, half_width) for a band of fixed width).
        want_row_lambda (rows="cells" only): the plan carries .row_lambda (P, N_s), the multipliers of the cell rows (>= 0 on the
        right edge n_lo, <= 0 on the left edge n_hi, 0 where the corridor does not bind)."""
        check_profile_args(N_s, v_cap, grip, n_plans)
        check_line_args(N_s, N_c, margin)
        if rows not in ("points", "cells"):
            raise ValueError("rows must be \"points\" or \"cells\", got %r" % (rows,))
        if rows == "cells" and corridor is None:
            raise ValueError("rows=\"cells\" needs a corridor: Corridor.constant(L, half_width) is the band of fixed width")
        if want_row_lambda and rows != "cells":
            raise ValueError("want_row_lambda needs rows=\"cells\"")
        if model not in (0, 1):
            raise ValueError("unknown model %r" % (model,))
        params, n_plans = check_params(params, n_plans)
        if corridor is not None:
            if not isinstance(corridor, Corridor):
                raise ValueError("corridor must be None or a Corridor")
            if corridor.P > 1 and params is not None and len(tuple(params.shape)) == 1:
                raise ValueError("a shared parameter block makes one plan, the corridor holds %d" % corridor.P)
            if corridor.P > 1 and params is None and n_plans == 1:
                n_plans = corridor.P                     # (one plan per corridor; with (P, 32) blocks n_plans is already their count)
            check_corridor(corridor, n_plans, device)
        import torch
        dev = torch.device(device)
        N_s, N_c, n_plans = int(N_s), int(N_c), int(n_plans)
        xP, yP = track.device(dev)
        sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        blocks = ParamBlock(params, n_plans, dev) if params is not None else None
        cells = rows == "cells"
        need = lib().fsaempc_plan_raceline_cells_workspace_bytes(n_plans, N_s, N_c) if cells else lib().fsaempc_plan_raceline_workspace_bytes(n_plans, N_c)
        if need < 0:
            check(int(need), "fsaempc_plan_raceline_cells_workspace_bytes" if cells else "fsaempc_plan_raceline_workspace_bytes")
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        line = torch.empty((n_plans, N_c), dtype=torch.float64, device=dev)
        flag = torch.empty(n_plans, dtype=torch.int32, device=dev)
        table = torch.empty((n_plans, N_s, 8), dtype=torch.float64, device=dev)
        t = torch.empty((n_plans, N_s), dtype=torch.float64, device=dev)
        opts = options if options is not None else default_opts()
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        p = lambda a: C.c_void_p(a.data_ptr())
        row_lambda = None
        if cells:
            row_lambda = torch.empty((n_plans, N_s), dtype=torch.float64, device=dev) if want_row_lambda else None
            rc = lib().fsaempc_plan_raceline_cells_batch_device(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                                corridor.ref(), n_plans, N_s, N_c, C.c_double(margin), C.c_double(v_cap),
                                                                C.c_double(grip), C.byref(opts), p(line), p(flag), p(table), p(t),
                                                                p(row_lambda) if row_lambda is not None else None, p(ws),
                                                                C.c_longlong(ws.numel() * 8), st)
            check(rc, "fsaempc_plan_raceline_cells_batch_device")
        else:
            rc = lib().fsaempc_plan_raceline_batch_device_c(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                            corridor.ref() if corridor is not None else None, n_plans, N_s, N_c, C.c_double(margin),
                                                            C.c_double(v_cap), C.c_double(grip), C.byref(opts), p(line), p(flag), p(table), p(t), p(ws),
                                                            C.c_longlong(ws.numel() * 8), st)
            check(rc, "fsaempc_plan_raceline_batch_device_c")
        plan = Plan(table, t, track.L / N_s)
        plan._blocks, plan._ws, plan._corridor = blocks, ws, corridor   # (read by launches that may still be queued)
        plan.line, plan.line_flag, plan.row_lambda = line, flag, row_lambda
        return plan

    @staticmethod
    def minlap(model, track, N_s=500, N_c=100, iters=12, rho=None, margin=0.25, corridor=None, params=None, grip=1.0, v_cap=20.0, c_init=None,
               n_plans=1, options=None, device="cuda:0", stream=None):
        """Minimum-time racing-line plans (fsaempc_plan_minlap_batch_device): from the line of Plan.raceline (or c_init,
        (N_c,) or (P, N_c)), `iters` iterations that lower the lap time of the profile on the line, T(c) = sum t, by steps
        d = argmin 1/2 rho d'H d + grad T'd inside the box of the control points, the best of the ladder `rho` per iteration (default:
        MINLAP_RHO).  The line depends on model, grip, v_cap and the parameter block, because T does.  corridor: None (the box
        +-(N_MAX - margin)) or a Corridor: the per-control-point boxes of Plan.raceline(corridor=).  Returns a Plan with .line
        (= .control_points, (P, N_c)), .line_flag (P,) of the initial QPs, .lap_history (P, iters + 1), non-increasing, and
        .step_history (P, iters): the index of the rho taken, -1 = stayed.  Still the quasi-steady-state profile (y_d = 0), a fixed
        number of local steps, no IPOPT: not the reference's minimum_time_planner."""
        check_profile_args(N_s, v_cap, grip, n_plans)
        check_line_args(N_s, N_c, margin)
        rho = check_minlap_args(N_s, iters, MINLAP_RHO if rho is None else rho)
        if model not in (0, 1):
            raise ValueError("unknown model %r" % (model,))
        params, n_plans = check_params(params, n_plans)
        shared_block = params is not None and len(tuple(params.shape)) == 1
        if corridor is not None:
            if not isinstance(corridor, Corridor):
                raise ValueError("corridor must be None or a Corridor")
            if corridor.P > 1 and shared_block:
                raise ValueError("a shared parameter block makes one plan, the corridor holds %d" % corridor.P)
            if corridor.P > 1 and params is None and n_plans == 1:
                n_plans = corridor.P
            check_corridor(corridor, n_plans, device)
        if c_init is not None:
            c_init, n_ci, n_line = check_line(c_init, N_s, n_plans)
            if n_ci != N_c:
                raise ValueError("c_init holds %d control points, N_c = %d" % (n_ci, N_c))
            if n_line != n_plans:
                if shared_block:
                    raise ValueError("a shared parameter block makes one plan, c_init holds %d" % n_line)
                n_plans = n_line
        import torch
        dev = torch.device(device)
        N_s, N_c, n_plans, iters, J = int(N_s), int(N_c), int(n_plans), int(iters), len(rho)
        xP, yP = track.device(dev)
        sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        blocks = ParamBlock(params, n_plans, dev) if params is not None else None
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        p = lambda a: C.c_void_p(a.data_ptr())
        lo = hi = ci = None
        if corridor is not None:
            lo = torch.empty((n_plans, N_c), dtype=torch.float64, device=dev)
            hi = torch.empty((n_plans, N_c), dtype=torch.float64, device=dev)
            rc = lib().fsaempc_corridor_line_bounds_device(corridor.ref(), C.c_double(track.L), n_plans, N_s, N_c, C.c_double(margin), p(lo), p(hi), st)
            check(rc, "fsaempc_corridor_line_bounds_device")
        if c_init is not None:
            ci = c_init if isinstance(c_init, torch.Tensor) else torch.from_numpy(np.array(c_init, dtype=np.float64))
            ci = ci.to(device=dev, dtype=torch.float64).reshape(-1, N_c).expand(n_plans, N_c).contiguous()
        need = lib().fsaempc_plan_minlap_workspace_bytes(n_plans, N_c, J)
        if need < 0:
            check(int(need), "fsaempc_plan_minlap_workspace_bytes")
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        line = torch.empty((n_plans, N_c), dtype=torch.float64, device=dev)
        flag = torch.empty(n_plans, dtype=torch.int32, device=dev)
        table = torch.empty((n_plans, N_s, 8), dtype=torch.float64, device=dev)
        t = torch.empty((n_plans, N_s), dtype=torch.float64, device=dev)
        lap = torch.empty((n_plans, iters + 1), dtype=torch.float64, device=dev)
        step = torch.empty((n_plans, iters), dtype=torch.int32, device=dev)
        opts = options if options is not None else default_opts()
        rho_c = (C.c_double * J)(*rho)
        rc = lib().fsaempc_plan_minlap_batch_device(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                    n_plans, N_s, N_c, C.c_double(margin), C.c_double(v_cap), C.c_double(grip), C.byref(opts), iters,
                                                    rho_c, J, p(ci) if ci is not None else None, p(lo) if lo is not None else None,
                                                    p(hi) if hi is not None else None, p(line), p(flag), p(table), p(t), p(lap),
                                                    p(step) if iters > 0 else None, p(ws), C.c_longlong(ws.numel() * 8), st)
        check(rc, "fsaempc_plan_minlap_batch_device")
        plan = Plan(table, t, track.L / N_s)
        plan._blocks, plan._ws, plan._corridor, plan._box = blocks, ws, corridor, (lo, hi, ci)   # (read by launches that may still be queued)
        plan.line, plan.line_flag = line, flag
        plan.control_points, plan.lap_history, plan.step_history, plan.rho = line, lap, step, rho
        return plan

    @staticmethod
    def lap_gradient(model, track, c, N_s=500, v_cap=20.0, grip=1.0, params=None, n_plans=1, device="cuda:0", stream=None):
        """(T, grad): the lap time (P,) of the profile of Plan.profile(line=c) and its gradient (P, N_c) in the control points c, (N_c,)
        shared by the plans or (P, N_c), on the device (fsaempc_plan_line_lapgrad_batch_device).  A NaN plan has T = NaN
        and a NaN gradient."""
        check_profile_args(N_s, v_cap, grip, n_plans)
        check_minlap_args(N_s, 0, MINLAP_RHO)
        if model not in (0, 1):
            raise ValueError("unknown model %r" % (model,))
        params, n_plans = check_params(params, n_plans)
        c, N_c, n_line = check_line(c, N_s, n_plans)
        if n_line != n_plans:
            if params is not None and len(tuple(params.shape)) == 1:
                raise ValueError("a shared parameter block makes one plan, c holds %d" % n_line)
            n_plans = n_line
        import torch
        dev = torch.device(device)
        N_s, N_c, n_plans = int(N_s), int(N_c), int(n_plans)
        xP, yP = track.device(dev)
        sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        blocks = ParamBlock(params, n_plans, dev) if params is not None else None
        cd = (c if isinstance(c, torch.Tensor) else torch.from_numpy(np.array(c, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()
        T = torch.empty(n_plans, dtype=torch.float64, device=dev)
        grad = torch.empty((n_plans, N_c), dtype=torch.float64, device=dev)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
        rc = lib().fsaempc_plan_line_lapgrad_batch_device(int(model), C.byref(sp), C.c_double(track.L), blocks.ref() if blocks is not None else None,
                                                          n_plans, N_s, N_c, C.c_void_p(cd.data_ptr()), 1 if cd.dim() == 2 else 0, C.c_double(v_cap),
                                                          C.c_double(grip), C.c_void_p(T.data_ptr()), C.c_void_p(grad.data_ptr()), st)
        check(rc, "fsaempc_plan_line_lapgrad_batch_device")
        T._keep = (blocks, cd)   # (read by a launch that may still be queued)
        return T, grad

    @staticmethod
    def from_table(table, t, ds, device="cuda:0"):
        """A user's own plan (numpy arrays or tensors), from the reference's planner for instance: table (N_s, 8), (8 N_s,) or
        (P, N_s, 8), t (N_s,) or (P, N_s), ds the cell length."""
        if not hasattr(table, "shape"):
            table = np.asarray(table, dtype=np.float64)
        if not hasattr(t, "shape"):
            t = np.asarray(t, dtype=np.float64)
        P, N_s = check_table(table, t, ds)
        import torch
        dev = torch.device(device)
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).to(device=dev, dtype=torch.float64)
        return Plan(up(table).reshape(P, N_s, 8).contiguous(), up(t).reshape(P, N_s).contiguous(), ds)

    def lap_time(self):
        """Sum of the traversal times of each plan, (P,) numpy."""
        return self.t.sum(dim=1).cpu().numpy()

    def check_batch(self, B):
        if self.P not in (1, B):
            raise ValueError("the plan holds %d tables: it serves a batch of %d (one per car) or any batch (one shared), not %d" % (self.P, self.P, B))

    def check_device(self, device):
        """The plan lives on one device; the loop that tracks it must run there (compared by name, before any device call)."""
        want, have = str(device), str(self.device)
        if want.split(":")[0] != have.split(":")[0] or (":" in want and ":" in have and want != have):
            raise ValueError("the plan is on %s, the loop on %s" % (have, want))

    def reference(self, model, s0, N, dt, stream=None):
        """x_ref (B, N, nx) for cars at arc lengths s0 (B,), the layout LtvBatch.step takes (fsaempc_plan_reference_batch_device)."""
        import torch
        if not isinstance(s0, torch.Tensor):
            s0 = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(s0), dtype=np.float64))
        s0 = s0.to(device=self.device, dtype=torch.float64).contiguous().reshape(-1)
        B = s0.numel()
        self.check_batch(B)
        nx = 5 if model == 0 else 7
        x_ref = torch.empty((B, int(N), nx), dtype=torch.float64, device=self.device)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)
        rc = lib().fsaempc_plan_reference_batch_device(int(model), self.ref(), C.c_void_p(s0.data_ptr()), C.c_double(dt), int(N), B,
                                                       C.c_void_p(x_ref.data_ptr()), st)
        check(rc, "fsaempc_plan_reference_batch_device")
        return x_ref


def raceline_qp(track, N_s, N_c, device="cuda:0", stream=None):
    """H (N_c, N_c) and g (N_c,) of the line QP of (track, N_s, N_c) on the device (fsaempc_raceline_build_qp_device)."""
    check_line_args(N_s, N_c)
    import torch
    dev = torch.device(device)
    N_s, N_c = int(N_s), int(N_c)
    xP, yP = track.device(dev)
    sp = Spline(track.M, track.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
    H = torch.empty((N_c, N_c), dtype=torch.float64, device=dev)
    g = torch.empty(N_c, dtype=torch.float64, device=dev)
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    rc = lib().fsaempc_raceline_build_qp_device(C.byref(sp), C.c_double(track.L), N_s, N_c, C.c_void_p(H.data_ptr()), C.c_void_p(g.data_ptr()), st)
    check(rc, "fsaempc_raceline_build_qp_device")
    return H, g
