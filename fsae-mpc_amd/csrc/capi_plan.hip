// capi_plan.hip -- the C ABI of libfsaempc.so (include/fsaempc.h), planning part: the s-domain plans, the racing lines (minimum
// curvature: plain, in a corridor, with cell-wise corridor rows; minimum time) and the corridors built from cones.  Host-side glue
// only: argument checks, workspace layout, kernel launches.
#include "capi_common.h"
#include "qp_solver.h"
#include "planner.h"
#include "raceline.h"
#include "minlap.h"
#include "cones.h"
using namespace capi;

extern "C" {

/* ---- s-domain plans ---- */
static int plan_check(const fsaempc_plan* plan, PlanTable* out) {
  if (!plan || !plan->table || !plan->t) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (plan->N_s < 1 || !pos_finite(plan->ds)) return fail(FSAEMPC_ERR_ARG, "bad plan dimensions");
  out->table = plan->table; out->t = plan->t; out->N_s = plan->N_s; out->ds = plan->ds; out->per_instance = plan->per_instance ? 1 : 0;
  return 0;
}

int fsaempc_plan_profile_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                      double v_cap, double grip, double* table, double* t, void* stream) {
  if (!sp || !sp->xP || !sp->yP || !table || !t) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (sp->M <= 0 || !(sp->dl > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (N_s < 2 || N_s > FSAEMPC_PLAN_MAX_NS) return fail(FSAEMPC_ERR_ARG, "N_s must be 2 .. FSAEMPC_PLAN_MAX_NS");
  if (!pos_finite(v_cap) || !pos_finite(grip) || !pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "v_cap, grip and L must be finite and > 0");
  if (grip > 1) return fail(FSAEMPC_ERR_ARG, "grip must be <= 1");
  if (n_plans < 1) return fail(FSAEMPC_ERR_ARG, "n_plans must be >= 1");
  if (par_values(par) && !par->per_instance && n_plans != 1) return fail(FSAEMPC_ERR_ARG, "a shared parameter block makes one plan");
  PlanProfileParams P; P.dynamic = model == FSAEMPC_MODEL_DYNAMIC; P.n_plans = n_plans; P.N_s = N_s; P.ds = L / N_s; P.v_cap = v_cap; P.grip = grip;
  set_spline(&P, sp); P.table = table; P.t = t;
  return launched(plan_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream), "plan_profile_launch");
}

int fsaempc_plan_reference_batch_device(int model, const fsaempc_plan* plan, const double* s0, double dt, int N, int batch, double* x_ref,
                                        void* stream) {
  PlanRefParams P;
  if (int rc = plan_check(plan, &P.plan)) return rc;
  if (!s0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.s0 = s0; P.x_ref = x_ref;
  return launched(plan_reference_launch(P, (hipStream_t)stream), "plan_reference_launch");
}

int fsaempc_cl_pre_plan_batch_device(int model, int N, double dt, double L, const fsaempc_spline* sp, const fsaempc_plan* plan,
                                     const double* cart, const double* s_guess, int batch, double* x0, double* x_ref, int* finished,
                                     void* stream) {
  ClPrePlanParams P;
  if (!sp || !sp->xP || !sp->yP || !cart || !s_guess || !x0 || !x_ref || !finished) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = plan_check(plan, &P.plan)) return rc;
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !pos_finite(dt) || sp->M <= 0 || !(sp->dl > 0) || !(L > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.L = L;
  set_spline(&P, sp); P.cart = cart; P.s_guess = s_guess; P.x0 = x0; P.x_ref = x_ref; P.finished = finished;
  return launched(cl_pre_plan_launch(P, (hipStream_t)stream), "cl_pre_plan_launch");
}

/* ---- minimum-curvature racing line ---- */
static int line_grid_check(double L, int N_s, int N_c) {
  if (!pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "L must be finite and > 0");
  if (N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_ARG, "N_c must be FSAEMPC_LINE_MIN_NC .. FSAEMPC_MAX_NV");
  if (N_s < 2 * N_c || N_s > FSAEMPC_LINE_MAX_NS) return fail(FSAEMPC_ERR_ARG, "N_s must be 2 N_c .. FSAEMPC_LINE_MAX_NS");
  return 0;
}
static int line_check(const fsaempc_spline* sp, double L, int N_s, int N_c) {
  if (!sp || !sp->xP || !sp->yP) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (sp->M <= 0 || !(sp->dl > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  return line_grid_check(L, N_s, N_c);
}
static int line_profile_check(int model, const fsaempc_ltv_params* par, int n_plans, double v_cap, double grip) {
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (!pos_finite(v_cap) || !pos_finite(grip)) return fail(FSAEMPC_ERR_ARG, "v_cap and grip must be finite and > 0");
  if (grip > 1) return fail(FSAEMPC_ERR_ARG, "grip must be <= 1");
  if (n_plans < 1) return fail(FSAEMPC_ERR_ARG, "n_plans must be >= 1");
  if (par_values(par) && !par->per_instance && n_plans != 1) return fail(FSAEMPC_ERR_ARG, "a shared parameter block makes one plan");
  return 0;
}
static RacelineQpParams line_qp_params(const fsaempc_spline* sp, double L, int N_s, int N_c, double* H, double* g) {
  RacelineQpParams Q; Q.N_s = N_s; Q.N_c = N_c; Q.ds = L / N_s; set_spline(&Q, sp); Q.H = H; Q.g = g;
  return Q;
}
static PlanLineParams line_profile_params(int model, const fsaempc_spline* sp, double L, int n_plans, int N_s, int N_c, double v_cap, double grip,
                                          double* table, double* t) {
  PlanLineParams P; memset(&P, 0, sizeof(P));
  P.dynamic = model == FSAEMPC_MODEL_DYNAMIC; P.n_plans = n_plans; P.N_s = N_s; P.N_c = N_c; P.ds = L / N_s; P.h = L / N_c; P.v_cap = v_cap; P.grip = grip;
  set_spline(&P, sp); P.table = table; P.t = t;
  return P;
}

int fsaempc_raceline_build_qp_device(const fsaempc_spline* sp, double L, int N_s, int N_c, double* H, double* g, void* stream) {
  if (!H || !g) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  return launched(raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, H, g), (hipStream_t)stream), "raceline_qp_launch");
}

int fsaempc_plan_line_profile_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                           int N_c, const double* line, int line_per_plan, double v_cap, double grip, double* table, double* t,
                                           void* stream) {
  if (!line || !table || !t) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = line_per_plan ? N_c : 0;
  return launched(plan_line_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream), "plan_line_profile_launch");
}

// The workspace layouts of this unit (Bump, capi_common.h): base NULL for the size alone; a shape the layout refuses is a code.
// workspace of fsaempc_plan_raceline_batch_device: H | g, lb, ub (n_plans x N_c each) | fval | iter | the solver's own
struct LineWs { double *H, *g, *lb, *ub, *fval; int* iter; char* qp; long long qp_bytes; size_t total; };
static int line_ws(int n_plans, int N_c, void* base, LineWs* c) {
  if (n_plans < 1 || N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV) return FSAEMPC_ERR_ARG;
  const fsaempc_qp_desc d = {N_c, 0, n_plans, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, 0);
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = (size_t)n_plans * N_c;
  Bump b(base);
  c->H = b.take<double>((size_t)N_c * N_c); c->g = b.take<double>(vec); c->lb = b.take<double>(vec); c->ub = b.take<double>(vec);
  c->fval = b.take<double>(n_plans); c->iter = b.take<int>(n_plans); c->qp = b.take<char>((size_t)c->qp_bytes);
  c->total = b.off;
  return 0;
}
long long fsaempc_plan_raceline_workspace_bytes(int n_plans, int N_c) {
  LineWs c;
  if (int rc = line_ws(n_plans, N_c, nullptr, &c)) return rc;
  return (long long)c.total;
}

// start (optional, fsaempc_plan_minlap_batch_device): the caller's boxes lo, hi (n_plans x N_c each) in place of +-(N_MAX_p - margin) --
// a plan whose QP is then not solved is NaN, as in a corridor -- and/or the caller's control points c_init in place of the solve.
struct LineStart { const double* lo; const double* hi; const double* c_init; };
static int plan_raceline(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, const fsaempc_corridor* cor, int n_plans,
                         int N_s, int N_c, double margin, double v_cap, double grip, const fsaempc_qp_opts* opts, double* line, int* flag,
                         double* table, double* t, void* workspace, long long workspace_bytes, void* stream, const LineStart* start = nullptr) {
  CorLineParams CL; memset(&CL, 0, sizeof(CL));
  const bool boxed = start && start->lo, given = start && start->c_init;
  if (cor) { if (int rc = cor_check(cor, &CL.cor)) return rc; }
  if (!line || !flag || !table || !t || !workspace) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  if (int rc = margin_check(margin)) return rc;
  LineWs c;
  if (int rc = line_ws(n_plans, N_c, workspace, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = launched(raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, c.H, c.g), st), "raceline_qp_launch")) return rc;
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = c.g; CL.lb = c.lb; CL.ub = c.ub; CL.line = line; CL.flag = flag;
  if (cor) {
    if (int rc = launched(cor_line_bounds_launch(CL, st), "cor_line_bounds_launch")) return rc;
  } else if (boxed) {
    MinlapBoxParams B; B.n_plans = n_plans; B.N_c = N_c; B.lo = start->lo; B.hi = start->hi; B.g = c.g; B.lb = c.lb; B.ub = c.ub;
    if (int rc = launched(minlap_box_launch(B, st), "minlap_box_launch")) return rc;
  } else {
    RacelineBoundsParams B; B.n_plans = n_plans; B.N_c = N_c; B.margin = margin; B.g = c.g; B.lb = c.lb; B.ub = c.ub;
    if (int rc = launched(raceline_bounds_launch(B, par_values(par), par_stride(par), st), "raceline_bounds_launch")) return rc;
  }
  if (given) {   // the caller's control points: no solve, every flag 0
    hipError_t e = hipMemcpyAsync(line, start->c_init, sizeof(double) * (size_t)n_plans * N_c, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(int) * (size_t)n_plans, st);
    if (int rc = launched(e, "copy of c_init")) return rc;
  } else {
    const fsaempc_qp_desc d = {N_c, 0, n_plans, 1};
    if (int rc = fsaempc_qp_solve_batch_device_s(&d, 0, c.H, c.g, nullptr, c.lb, c.ub, nullptr, nullptr, opts, line, c.fval, flag,
                                                 c.iter, nullptr, nullptr, c.qp, c.qp_bytes, stream)) return rc;
    // a plan whose QP was not solved (no box: flag -1, or any other flag but 0): NaN control points, which the profile turns into a NaN plan
    if (cor || boxed) if (int rc = launched(cor_line_void_launch(CL, st), "cor_line_void_launch")) return rc;
  }
  const bool fallback = !cor && !boxed && !given;   // (in a corridor or a box: no centre-line fallback)
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = N_c; P.flag = fallback ? flag : nullptr; P.line_out = line; P.check_width = (cor || boxed) ? 0 : 1; P.margin = margin;
  return launched(plan_line_profile_launch(P, par_values(par), par_stride(par), st), "plan_line_profile_launch");
}

int fsaempc_plan_raceline_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                       int N_c, double margin, double v_cap, double grip, const fsaempc_qp_opts* opts, double* line, int* flag,
                                       double* table, double* t, void* workspace, long long workspace_bytes, void* stream) {
  return plan_raceline(model, sp, L, par, nullptr, n_plans, N_s, N_c, margin, v_cap, grip, opts, line, flag, table, t, workspace, workspace_bytes, stream);
}
int fsaempc_plan_raceline_batch_device_c(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, const fsaempc_corridor* cor,
                                         int n_plans, int N_s, int N_c, double margin, double v_cap, double grip, const fsaempc_qp_opts* opts,
                                         double* line, int* flag, double* table, double* t, void* workspace, long long workspace_bytes, void* stream) {
  return plan_raceline(model, sp, L, par, cor, n_plans, N_s, N_c, margin, v_cap, grip, opts, line, flag, table, t, workspace, workspace_bytes, stream);
}

// the checks of the entries that make the line's bounds or rows alone, after the corridor's and the pointers'
static int line_rows_check(double L, int n_plans, int N_s, int N_c, double margin) {
  if (int rc = line_grid_check(L, N_s, N_c)) return rc;
  if (n_plans < 1) return fail(FSAEMPC_ERR_ARG, "n_plans must be >= 1");
  return margin_check(margin);
}

int fsaempc_corridor_line_bounds_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                        double* lb, double* ub, void* stream) {
  CorLineParams CL;
  if (!cor) return fail(FSAEMPC_ERR_ARG, "null argument (corridor)");
  if (int rc = cor_check(cor, &CL.cor)) return rc;
  if (!lb || !ub) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_rows_check(L, n_plans, N_s, N_c, margin)) return rc;
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = nullptr; CL.lb = lb; CL.ub = ub; CL.line = nullptr; CL.flag = nullptr;
  return launched(cor_line_bounds_launch(CL, (hipStream_t)stream), "cor_line_bounds_launch");
}

/* ---- the minimum-time racing line ---- */
static int minlap_check(const fsaempc_spline* sp, double L, int N_s, int N_c) {
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  if (N_s > FSAEMPC_MINLAP_MAX_NS) return fail(FSAEMPC_ERR_ARG, "N_s must be <= FSAEMPC_MINLAP_MAX_NS");
  return 0;
}
static MinlapGradParams minlap_grad_params(int model, const fsaempc_spline* sp, double L, int n_waves, int N_s, int N_c, double v_cap, double grip) {
  MinlapGradParams P; memset(&P, 0, sizeof(P));
  P.dynamic = model == FSAEMPC_MODEL_DYNAMIC; P.n_waves = n_waves; P.N_s = N_s; P.N_c = N_c; P.cand = 1; P.ds = L / N_s; P.h = L / N_c;
  P.v_cap = v_cap; P.grip = grip; set_spline(&P, sp); P.T_stride = 1;
  return P;
}

int fsaempc_plan_line_lapgrad_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                           int N_c, const double* line, int line_per_plan, double v_cap, double grip, double* T, double* grad,
                                           void* stream) {
  if (!line || !T || !grad) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = minlap_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  MinlapGradParams P = minlap_grad_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip);
  P.line = line; P.line_stride = line_per_plan ? N_c : 0; P.T = T; P.grad = grad;
  return launched(minlap_lapgrad_launch(P, par_values(par), par_stride(par), (hipStream_t)stream), "minlap_lapgrad_launch");
}

// workspace of fsaempc_plan_minlap_batch_device: that of fsaempc_plan_raceline_batch_device for n_plans (H, the boxes and the initial
// solve) | grad (n_plans x N_c) | per candidate (n_plans J): g, lb, ub, x (N_c each), T, fval, iter, flag | gradc (n_plans J x N_c) |
// the solver's own for n_plans J instances
struct MinlapWs { LineWs line; double *grad, *g, *lb, *ub, *x, *T, *fval; int *iter, *flag; double* gradc; char* qp; long long qp_bytes; size_t total; };
static int minlap_ws(int n_plans, int N_c, int J, void* base, MinlapWs* c) {
  if (J < 1 || J > FSAEMPC_MINLAP_MAX_RHO) return FSAEMPC_ERR_ARG;
  if (int rc = line_ws(n_plans, N_c, base, &c->line)) return rc;
  if ((long long)n_plans * J > 0x7fffffffLL) return FSAEMPC_ERR_ARG;
  const int nJ = n_plans * J;
  const fsaempc_qp_desc d = {N_c, 0, nJ, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, 0);
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = (size_t)nJ * N_c;
  Bump b(base, c->line.total);
  c->grad = b.take<double>((size_t)n_plans * N_c); c->g = b.take<double>(vec); c->lb = b.take<double>(vec); c->ub = b.take<double>(vec);
  c->x = b.take<double>(vec); c->T = b.take<double>(nJ); c->fval = b.take<double>(nJ);
  c->iter = b.take<int>(2 * (size_t)nJ); c->flag = b.take<int>(2 * (size_t)nJ);   // (the room of nJ doubles each: the sizes have always counted them so)
  c->gradc = b.take<double>(vec); c->qp = b.take<char>((size_t)c->qp_bytes);
  c->total = b.off;
  return 0;
}
long long fsaempc_plan_minlap_workspace_bytes(int n_plans, int N_c, int n_rho) {
  MinlapWs c;
  if (int rc = minlap_ws(n_plans, N_c, n_rho, nullptr, &c)) return rc;
  return (long long)c.total;
}

int fsaempc_plan_minlap_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                     int N_c, double margin, double v_cap, double grip, const fsaempc_qp_opts* opts, int iters,
                                     const double* rho, int n_rho, const double* c_init, const double* lo, const double* hi, double* line,
                                     int* flag, double* table, double* t, double* lap_hist, int* step_hist, void* workspace,
                                     long long workspace_bytes, void* stream) {
  if (!line || !flag || !table || !t || !workspace || !rho || !lap_hist) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = minlap_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  if (int rc = margin_check(margin)) return rc;
  if (iters < 0) return fail(FSAEMPC_ERR_ARG, "iters must be >= 0");
  if (iters > 0 && !step_hist) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (n_rho < 1 || n_rho > FSAEMPC_MINLAP_MAX_RHO) return fail(FSAEMPC_ERR_ARG, "n_rho must be 1 .. FSAEMPC_MINLAP_MAX_RHO");
  for (int j = 0; j < n_rho; ++j)
    if (!pos_finite(rho[j])) return fail(FSAEMPC_ERR_ARG, "every rho must be finite and > 0");
  if ((lo != nullptr) != (hi != nullptr)) return fail(FSAEMPC_ERR_ARG, "lo and hi come together");
  MinlapWs c;
  if (int rc = minlap_ws(n_plans, N_c, n_rho, workspace, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  // the start: fsaempc_plan_raceline_batch_device itself (with K = 0 and neither boxes nor c_init this call is that entry)
  const LineStart start = {lo, hi, c_init};
  if (int rc = plan_raceline(model, sp, L, par, nullptr, n_plans, N_s, N_c, margin, v_cap, grip, opts, line, flag, table, t, workspace,
                             (long long)c.line.total, stream, (lo || c_init) ? &start : nullptr)) return rc;
  const double *H = c.line.H, *blo = c.line.lb, *bhi = c.line.ub;
  const int nJ = n_plans * n_rho, check_width = lo ? 0 : 1;
  MinlapGradParams G = minlap_grad_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip);
  G.check_width = check_width; G.margin = margin; G.line = line; G.line_stride = N_c; G.T = lap_hist; G.T_stride = iters + 1; G.grad = c.grad;
  if (int rc = launched(minlap_lapgrad_launch(G, par_values(par), par_stride(par), st), "minlap_lapgrad_launch")) return rc;
  for (int it = 0; it < iters; ++it) {
    MinlapCandParams Q; memset(&Q, 0, sizeof(Q));
    Q.n_plans = n_plans; Q.J = n_rho; Q.N_c = N_c; Q.grad = c.grad; Q.c = line; Q.lo = blo; Q.hi = bhi;
    for (int j = 0; j < n_rho; ++j) Q.rho[j] = rho[j];
    Q.g = c.g; Q.lb = c.lb; Q.ub = c.ub;
    if (int rc = launched(minlap_candidates_launch(Q, st), "minlap_candidates_launch")) return rc;
    const fsaempc_qp_desc d = {N_c, 0, nJ, 1};
    if (int rc = fsaempc_qp_solve_batch_device_s(&d, 0, H, Q.g, nullptr, Q.lb, Q.ub, nullptr, nullptr, opts, c.x, c.fval, c.flag,
                                                 c.iter, nullptr, nullptr, c.qp, c.qp_bytes, stream)) return rc;
    MinlapGradParams C = minlap_grad_params(model, sp, L, nJ, N_s, N_c, v_cap, grip);   // the candidates: clamp(c + d, lo, hi), each with its plan's block
    C.cand = n_rho; C.check_width = check_width; C.margin = margin; C.line = c.x; C.line_stride = N_c; C.base = line; C.lo = blo; C.hi = bhi;
    C.line_out = c.x; C.T = c.T; C.grad = c.gradc;
    if (int rc = launched(minlap_lapgrad_launch(C, par_values(par), par_stride(par), st), "minlap_lapgrad_launch")) return rc;
    MinlapSelectParams S; S.n_plans = n_plans; S.J = n_rho; S.N_c = N_c; S.it = it; S.K = iters; S.Tc = c.T; S.flagc = c.flag; S.cc = c.x; S.gradc = c.gradc;
    S.c = line; S.grad = c.grad; S.lap_hist = lap_hist; S.step_hist = step_hist;
    if (int rc = launched(minlap_select_launch(S, st), "minlap_select_launch")) return rc;
  }
  if (iters > 0) {   // the table of the final control points, by the line-profile path
    PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
    P.line = line; P.line_stride = N_c; P.flag = nullptr; P.line_out = line; P.check_width = check_width; P.margin = margin;
    if (int rc = launched(plan_line_profile_launch(P, par_values(par), par_stride(par), st), "plan_line_profile_launch")) return rc;
  }
  return 0;
}

/* ---- the racing line with cell-wise corridor rows ---- */
// The slack count handed to the solve, always given: N_s = 3 (N_c - 1) and 10 (N_c - 4) carry the signature of the LTV QPs, which must
// not be read off a line QP.  0 up to twelve column tiles; the last four control points as the border beyond (N_c 193 .. 196, the
// split the solver gives FSAEMPC_MAX_NV everywhere else): 13 tiles are more than the kernels are built for.
static int cells_n_slack(int N_c) { return N_c > 16 * QP_MAX_T ? 4 : 0; }
// workspace of fsaempc_plan_raceline_cells_batch_device:
//   H | A (N_s x N_c) | g, lb, ub (n_plans x N_c each) | lbA, ubA (n_plans x N_s each) | fval | iter | lambda (n_plans x (N_c + N_s)) | the solver's own
struct CellsWs { double *H, *A, *g, *lb, *ub, *lbA, *ubA, *fval; int* iter; double* lambda; char* qp; long long qp_bytes; size_t total; };
static int cells_ws(int n_plans, int N_s, int N_c, void* base, CellsWs* c) {
  if (n_plans < 1 || N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV || N_s < 2 * N_c || N_s > FSAEMPC_LINE_MAX_NS) return FSAEMPC_ERR_ARG;
  const fsaempc_qp_desc d = {N_c, N_s, n_plans, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, cells_n_slack(N_c));
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = (size_t)n_plans * N_c, row = (size_t)n_plans * N_s;
  Bump b(base);
  c->H = b.take<double>((size_t)N_c * N_c); c->A = b.take<double>((size_t)N_s * N_c);
  c->g = b.take<double>(vec); c->lb = b.take<double>(vec); c->ub = b.take<double>(vec); c->lbA = b.take<double>(row); c->ubA = b.take<double>(row);
  c->fval = b.take<double>(n_plans); c->iter = b.take<int>(n_plans); c->lambda = b.take<double>(vec + row);
  c->qp = b.take<char>((size_t)c->qp_bytes);
  c->total = b.off;
  return 0;
}
long long fsaempc_plan_raceline_cells_workspace_bytes(int n_plans, int N_s, int N_c) {
  CellsWs c;
  if (int rc = cells_ws(n_plans, N_s, N_c, nullptr, &c)) return rc;
  return (long long)c.total;
}
// what fsaempc_qp_solve_batch_device_s refuses for its shape, with its codes and texts, before anything is launched
static int cells_shape_check(int N_s, int N_c) {
  QpDims d; qp_make_dims(N_c, N_s, &d, cells_n_slack(N_c));
  if (d.T > QP_MAX_T) return fail(FSAEMPC_ERR_DIM, "more column tiles than the kernels are built for");
  if ((qp_runs_wavefront_kernel(d) ? d.lds_solve : d.lds_wg) > 160 * 1024 || d.lds_prep > 160 * 1024)
    return fail(FSAEMPC_ERR_DIM, "problem exceeds the 160 KiB LDS budget of the kernels");
  return 0;
}

int fsaempc_plan_raceline_cells_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, const fsaempc_corridor* cor,
                                             int n_plans, int N_s, int N_c, double margin, double v_cap, double grip, const fsaempc_qp_opts* opts,
                                             double* line, int* flag, double* table, double* t, double* row_lambda, void* workspace,
                                             long long workspace_bytes, void* stream) {
  CorLineRowsParams R;
  if (!cor) return fail(FSAEMPC_ERR_ARG, "null argument (corridor)");
  if (int rc = cor_check(cor, &R.cor)) return rc;
  if (!line || !flag || !table || !t || !workspace) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  if (int rc = margin_check(margin)) return rc;
  if (int rc = cells_shape_check(N_s, N_c)) return rc;
  CellsWs c;
  if (int rc = cells_ws(n_plans, N_s, N_c, workspace, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  double* lambda = row_lambda ? c.lambda : nullptr;
  if (int rc = launched(raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, c.H, c.g), st), "raceline_qp_launch")) return rc;
  R.n_plans = n_plans; R.N_s = N_s; R.N_c = N_c; R.L = L; R.margin = margin; R.A = c.A; R.lbA = c.lbA; R.ubA = c.ubA;
  R.g = c.g; R.lb = c.lb; R.ub = c.ub;
  if (int rc = launched(cor_line_rows_launch(R, st), "cor_line_rows_launch")) return rc;
  const fsaempc_qp_desc d = {N_c, N_s, n_plans, 1};
  if (int rc = fsaempc_qp_solve_batch_device_s(&d, cells_n_slack(N_c), c.H, c.g, R.A, R.lb, R.ub, R.lbA, R.ubA, opts, line, c.fval, flag,
                                               c.iter, lambda, nullptr, c.qp, c.qp_bytes, stream)) return rc;
  if (row_lambda) if (int rc = launched(cor_line_lambda_launch(lambda, row_lambda, n_plans, N_s, N_c, st), "cor_line_lambda_launch")) return rc;
  CorLineParams CL; CL.cor = R.cor;
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = c.g; CL.lb = R.lb; CL.ub = R.ub; CL.line = line; CL.flag = flag;
  // (no centre-line fallback: every plan whose flag is not 0 is NaN)
  if (int rc = launched(cor_line_void_launch(CL, st), "cor_line_void_launch")) return rc;
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = N_c; P.flag = nullptr; P.line_out = line; P.check_width = 0; P.margin = margin;
  return launched(plan_line_profile_launch(P, par_values(par), par_stride(par), st), "plan_line_profile_launch");
}

int fsaempc_corridor_line_rows_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                      double* A, double* lbA, double* ubA, void* stream) {
  CorLineRowsParams R;
  if (!cor) return fail(FSAEMPC_ERR_ARG, "null argument (corridor)");
  if (int rc = cor_check(cor, &R.cor)) return rc;
  if (!A || !lbA || !ubA) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_rows_check(L, n_plans, N_s, N_c, margin)) return rc;
  R.n_plans = n_plans; R.N_s = N_s; R.N_c = N_c; R.L = L; R.margin = margin; R.A = A; R.lbA = lbA; R.ubA = ubA; R.g = nullptr; R.lb = nullptr; R.ub = nullptr;
  return launched(cor_line_rows_launch(R, (hipStream_t)stream), "cor_line_rows_launch");
}

/* ---- track corridors from cone positions ---- */
int fsaempc_corridor_from_cones_device(const fsaempc_spline* sp, double L, const fsaempc_cones* cones, int n_corridors,
                                       int N_w, double margin, double reach, double* n_lo, double* n_hi, double* info, void* stream) {
  if (!sp) return fail(FSAEMPC_ERR_ARG, "cones: sp is NULL");
  if (!sp->xP || !sp->yP) return fail(FSAEMPC_ERR_ARG, "cones: the spline tables are NULL");
  if (!cones) return fail(FSAEMPC_ERR_ARG, "cones: cones is NULL");
  if (!n_lo) return fail(FSAEMPC_ERR_ARG, "cones: n_lo is NULL");
  if (!n_hi) return fail(FSAEMPC_ERR_ARG, "cones: n_hi is NULL");
  if (n_corridors < 1) return fail(FSAEMPC_ERR_ARG, "cones: n_corridors must be >= 1");
  if (N_w < 2) return fail(FSAEMPC_ERR_ARG, "cones: N_w must be >= 2");
  if (!pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "cones: L must be finite and > 0");
  if (int rc = margin_check(margin, "cones: ")) return rc;
  if (!pos_finite(reach)) return fail(FSAEMPC_ERR_ARG, "cones: reach must be finite and > 0");
  if (cones->n_left < 0) return fail(FSAEMPC_ERR_ARG, "cones: n_left must be >= 0");
  if (cones->n_right < 0) return fail(FSAEMPC_ERR_ARG, "cones: n_right must be >= 0");
  if (!cones->left && cones->n_left > 0) return fail(FSAEMPC_ERR_ARG, "cones: left is NULL with n_left > 0");
  if (!cones->right && cones->n_right > 0) return fail(FSAEMPC_ERR_ARG, "cones: right is NULL with n_right > 0");
  if (sp->M < 1 || !pos_finite(sp->dl)) return fail(FSAEMPC_ERR_ARG, "cones: the spline needs M >= 1 and dl finite and > 0");
  if (cones->n_left > FSAEMPC_CONES_MAX) return fail(FSAEMPC_ERR_DIM, "cones: n_left exceeds FSAEMPC_CONES_MAX");
  if (cones->n_right > FSAEMPC_CONES_MAX) return fail(FSAEMPC_ERR_DIM, "cones: n_right exceeds FSAEMPC_CONES_MAX");
  if (sp->M > FSAEMPC_CONES_MAX_M) return fail(FSAEMPC_ERR_DIM, "cones: M exceeds FSAEMPC_CONES_MAX_M");
  ConesParams P;
  set_spline(&P, sp);
  P.L = L; P.left = cones->left; P.right = cones->right; P.n_left = cones->n_left; P.n_right = cones->n_right;
  P.per_corridor = cones->per_corridor ? 1 : 0; P.n_corridors = n_corridors; P.N_w = N_w; P.margin = margin; P.reach = reach;
  P.n_lo = n_lo; P.n_hi = n_hi; P.info = info;
  Range r("fsaempc.corridor.cones");
  return launched(cor_from_cones_launch(P, (hipStream_t)stream), "cor_from_cones_launch");
}

}  // extern "C"
