// capi_ltv.hip -- the C ABI of libfsaempc.so (include/fsaempc.h), MPC part: the LTV build, step, affine maps and step-VJP families
// and the batched SQP.  Host-side glue only: argument checks, workspace layout, kernel launches.
// The LTV build and step entries share one host path each (ltv_build_impl, ltv_step_impl) that takes the parameter block, the
// blocking and the corridor as optional descriptors; the entries without a suffix and _aux, _lambda, _p, _b are forwards with NULL
// for what they do not take, plus the one check that is theirs.
#include "capi_common.h"
#include "sqp.h"
#include "cl_nmpc.h"
using namespace capi;

extern "C" {

int fsaempc_ltv_nx(int model) { return model == FSAEMPC_MODEL_KINEMATIC ? 5 : 7; }
int fsaempc_ltv_nV(int model, int N) { return 2 * N + ltv_ns(model); }
int fsaempc_ltv_nC(int model, int N) { return (model == FSAEMPC_MODEL_KINEMATIC ? 6 : 20) * N; }

/* ---- parameter blocks ---- */
int fsaempc_ltv_default_params(int model, double* out) {
  if (!out) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  const bool dyn = model == FSAEMPC_MODEL_DYNAMIC;
  out[FSAEMPC_P_M] = 280; out[FSAEMPC_P_IZ] = 200; out[FSAEMPC_P_LF] = 0.8672; out[FSAEMPC_P_LR] = 0.6183; out[FSAEMPC_P_GRAV] = 9.81;
  out[FSAEMPC_P_PB] = 12.56; out[FSAEMPC_P_PC] = 1.38; out[FSAEMPC_P_PD] = 1.60; out[FSAEMPC_P_PE] = -0.58;
  out[FSAEMPC_P_Q_S] = 5; out[FSAEMPC_P_Q_N] = 250; out[FSAEMPC_P_Q_MU] = 2000; out[FSAEMPC_P_Q_TERMINAL] = 10;
  out[FSAEMPC_P_R_ACC] = 10; out[FSAEMPC_P_R_STEER] = 10;
  out[FSAEMPC_P_R_SOFT0] = 1e8; out[FSAEMPC_P_R_SOFT1] = dyn ? 1e6 : 0; out[FSAEMPC_P_R_SOFT2] = dyn ? 1e6 : 0; out[FSAEMPC_P_R_SOFT3] = dyn ? 1e4 : 0;
  out[FSAEMPC_P_U_ACC_MAX] = 10; out[FSAEMPC_P_U_STEER_MAX] = 0.4; out[FSAEMPC_P_DELTA_MAX] = 0.4; out[FSAEMPC_P_N_MAX] = 0.75;
  out[FSAEMPC_P_V_MIN] = 0; out[FSAEMPC_P_ALAT_MAX] = 5; out[FSAEMPC_P_SLIP_MAX] = 0.1; out[FSAEMPC_P_ELL_LONG] = 10.0; out[FSAEMPC_P_ELL_LAT] = 9.163;
  out[FSAEMPC_P_PID_KP_V] = 16000; out[FSAEMPC_P_PID_MAX_F] = 2800; out[FSAEMPC_P_PID_KP_D] = 80; out[FSAEMPC_P_PID_MAX_DRATE] = 0.8;
  return 0;
}

// the track-row bounds of a built batch (plain or blocked: the rows are the same) from the corridor
static int cor_rows(const fsaempc_ltv_desc* desc, const CorTable& cor, const double* x_lin, const double* pred, double* lbA, double* ubA,
                    void* stream) {
  Range r("fsaempc.ltv.corridor");
  CorRowsParams P; P.nx = fsaempc_ltv_nx(desc->model); P.N = desc->N; P.nC = fsaempc_ltv_nC(desc->model, desc->N); P.batch = desc->batch;
  P.x_lin = x_lin; P.pred = pred; P.lbA = lbA; P.ubA = ubA; P.cor = cor;
  return launched(cor_rows_launch(P, (hipStream_t)stream), "cor_rows_launch");
}

/* ---- move blocking ---- */
int fsaempc_ltv_blocked_nV(int model, const fsaempc_ltv_blocking* blk) {
  if (!blk || blk->n_blocks < 1) return fail(FSAEMPC_ERR_ARG, "blocking: n_blocks >= 1");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  return 2 * blk->n_blocks + ltv_ns(model);
}

// checks the descriptor pair and fills the kernels' block map; *trivial: one step per block (the unblocked problem)
static int blk_check(const fsaempc_ltv_desc* d, const fsaempc_ltv_blocking* blk, LtvBlockMap* bm, bool* trivial) {
  if (!d || !blk || !blk->len) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (d->N <= 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (blk->n_blocks < 1 || blk->n_blocks > d->N) return fail(FSAEMPC_ERR_ARG, "blocking: 1 <= n_blocks <= N");
  long long sum = 0;
  for (int j = 0; j < blk->n_blocks; ++j) { if (blk->len[j] < 1) return fail(FSAEMPC_ERR_ARG, "blocking: every block length >= 1"); sum += blk->len[j]; }
  if (sum != d->N) return fail(FSAEMPC_ERR_ARG, "blocking: the block lengths must sum to N");
  if (d->model != FSAEMPC_MODEL_KINEMATIC && d->model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (fsaempc_ltv_nV(d->model, d->N) > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "2N + ns exceeds FSAEMPC_MAX_NV");
  memset(bm, 0, sizeof(*bm));
  bm->M = blk->n_blocks;
  int st = 0;
  for (int j = 0; j < blk->n_blocks; ++j) { bm->start[j] = (unsigned char)st; st += blk->len[j]; }
  bm->start[blk->n_blocks] = (unsigned char)st;
  *trivial = blk->n_blocks == d->N;
  return 0;
}

/* ---- one build, one layout, one step: every fsaempc_ltv_build_qp_* / _step_* entry below is a forward ---- */
// What the optional descriptors make of a call, worked out once.  Unblocked -- and a trivial blocking (n_blocks == N) is the unblocked
// problem: same kernels, same layout -- the QP has 2N + ns variables and is sized and solved without a slack hint; blocked it has
// 2M + ns and the hint ns, in the workspace size and in the solve alike.
struct LtvShape {
  bool blocked = false, corridor = false;
  LtvBlockMap bm; CorTable cor;
  int nV(const fsaempc_ltv_desc* d) const { return blocked ? 2 * bm.M + ltv_ns(d->model) : fsaempc_ltv_nV(d->model, d->N); }
  int slack_hint(const fsaempc_ltv_desc* d) const { return blocked ? ltv_ns(d->model) : -1; }
};
// refusals in the order of the ABI: the corridor's, then the blocking's (its own text for 2N + ns > FSAEMPC_MAX_NV)
static int ltv_shape(const fsaempc_ltv_desc* desc, const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor, bool have_pred, LtvShape* s) {
  if (cor) {
    if (int rc = cor_check(cor, &s->cor)) return rc;
    if (!have_pred) return fail(FSAEMPC_ERR_ARG, "null argument (pred is required with a corridor)");
    s->corridor = true;
  }
  if (blk) {
    bool trivial = false;
    if (int rc = blk_check(desc, blk, &s->bm, &trivial)) return rc;
    s->blocked = !trivial;
  }
  return 0;
}

// the descriptor pair as the kernels take it; the caller adds the tensors its launch writes
static LtvParams ltv_params(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const double* x_lin, const double* u_lin) {
  LtvParams P; memset(&P, 0, sizeof(P));
  P.nx = fsaempc_ltv_nx(desc->model); P.N = desc->N; P.dt = desc->dt; P.integ = ltv_integ(desc);
  set_spline(&P, sp); P.x_lin = x_lin; P.u_lin = u_lin;
  return P;
}

struct LtvQp { double *H, *g, *A, *lb, *ub, *lbA, *ubA, *pred, *Bt, *qconst; };   // the tensors of a built batch

// The build of a checked shape: LTV about (x_lin, u_lin), or exact (the NLP's: no x_lin); with the constants compiled in, or read
// from par -- par_idx then names the batch instance behind each instance of this (sub-)batch, for the per-instance blocks.
static int ltv_build_shaped(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par, const LtvShape& s,
                            const double* x0, const double* x_ref, const double* x_lin, const double* u_lin, const LtvQp& q, void* stream,
                            bool exact, const int* par_idx) {
  int rc = ltv_check(desc, sp); if (rc) return rc;
  const int nx = fsaempc_ltv_nx(desc->model), N = desc->N;
  const char* too_long = "horizon too long for the LDS staging";
  const LtvBlockMap* bm = s.blocked ? &s.bm : nullptr;
  // (the exact build's carve is refused ahead of a null argument, the order the ABI's tests pin; the check below covers the rest)
  if (exact && ltv_build_lds_bytes(nx, N, 256, true) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, too_long);
  if (!x0 || !x_ref || (!exact && !x_lin) || !u_lin || !q.H || !q.g || !q.A || !q.lb || !q.ub || !q.lbA || !q.ubA || !q.Bt)
    return fail(FSAEMPC_ERR_ARG, "null argument (Bt is required as scratch)");
  if (ltv_build_lds_bytes(nx, N, 256, exact, par_values(par) != nullptr, bm ? bm->M : 0) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, too_long);
  if (desc->batch == 0) return 0;
  LtvParams P = ltv_params(desc, sp, x_lin, u_lin);
  P.x0 = x0; P.x_ref = x_ref;
  P.H = q.H; P.g = q.g; P.A = q.A; P.lb = q.lb; P.ub = q.ub; P.lbA = q.lbA; P.ubA = q.ubA; P.pred = q.pred; P.Bt = q.Bt; P.qconst = q.qconst;
  return launched(ltv_build_launch(P, bm, par_values(par), par_stride(par), par_idx, desc->batch, (hipStream_t)stream, exact), "ltv_build_launch");
}

// the build entries: optional parameter block, blocking and corridor (whose rows overwrite the track rows of the built batch)
static int ltv_build_impl(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                          const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                          const double* x0, const double* x_ref, const double* x_lin, const double* u_lin, const LtvQp& q, void* stream,
                          bool exact) {
  LtvShape s;
  int rc = ltv_shape(desc, blk, cor, q.pred != nullptr, &s); if (rc) return rc;
  rc = ltv_build_shaped(desc, sp, par, s, x0, x_ref, x_lin, u_lin, q, stream, exact, nullptr);
  if (rc || !s.corridor) return rc;
  return cor_rows(desc, s.cor, x_lin, q.pred, q.lbA, q.ubA, stream);
}

// ---- the workspace layouts (Bump, capi_common.h): base NULL for the size alone ----
// the tensors of a built batch, in the order every layout here keeps them
static LtvQp take_qp(Bump& b, size_t B, size_t nV, size_t nC, size_t R) {
  LtvQp q;
  q.H = b.take<double>(B * nV * nV); q.g = b.take<double>(B * nV); q.A = b.take<double>(B * nC * nV);
  q.lb = b.take<double>(B * nV); q.ub = b.take<double>(B * nV); q.lbA = b.take<double>(B * nC); q.ubA = b.take<double>(B * nC);
  q.pred = b.take<double>(B * R); q.Bt = b.take<double>(B * R * nV); q.qconst = b.take<double>(B);
  return q;
}
// the solver's region closes a layout, on a 256-byte boundary; a size query of the solver that fails leaves it empty
static char* take_solver(Bump& b, long long want, size_t* bytes) { *bytes = want > 0 ? (size_t)want : 0; return b.take<char>(*bytes, 256); }

// QP tensors | the solve's point z | the solver's workspace, sized with the slack hint the solve is given
struct LtvWs { LtvQp q; double* z; char* qpws; size_t qp_bytes, total; };
static LtvWs ltv_ws(const fsaempc_ltv_desc* d, int nV_, int slack_hint_, void* base) {
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N;
  const size_t nV = nV_, nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  Bump b(base);
  LtvWs c;
  c.q = take_qp(b, B, nV, nC, R); c.z = b.take<double>(B * nV);
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  c.qpws = take_solver(b, fsaempc_qp_workspace_bytes_s(&q, slack_hint_), &c.qp_bytes);
  c.total = b.off;
  return c;
}

// The step: build (+ corridor rows), solve, post-solve in one workspace.  Refusals in the order of the ABI: corridor, blocking,
// descriptors, nulls, FSAEMPC_MAX_NV, then the empty batch (nothing is written), then the workspace size.
static int ltv_step_impl(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                         const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                         const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                         const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                         int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                         void* workspace, long long workspace_bytes, void* stream) {
  LtvShape s;
  int rc = ltv_shape(desc, blk, cor, true, &s); if (rc) return rc;
  rc = ltv_check(desc, sp); if (rc) return rc;
  if (!x0 || !x_ref || !x_lin || !u_lin || !u_opt || !x_opt || !slack || !fval || !exitflag || !iter || !workspace) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  if (desc->batch == 0) return 0;
  const int nx = fsaempc_ltv_nx(desc->model), ns = ltv_ns(desc->model), nV = s.nV(desc), hint = s.slack_hint(desc);
  const LtvWs c = ltv_ws(desc, nV, hint, workspace);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const LtvQp& q = c.q;
  const hipStream_t st = (hipStream_t)stream;
  Range whole(s.blocked ? "fsaempc.ltv.step_blocked" : "fsaempc.ltv.step");
  const bool timing = g_timing.load();
  if (timing) if ((rc = launched(hipEventRecord(g_evf[0], st), "hipEventRecord"))) return rc;
  { Range r(s.blocked ? "fsaempc.ltv.build_blocked" : "fsaempc.ltv.build");
    rc = ltv_build_shaped(desc, sp, par, s, x0, x_ref, x_lin, u_lin, q, stream, false, nullptr); }
  if (rc) return rc;
  if (s.corridor) { rc = cor_rows(desc, s.cor, x_lin, q.pred, q.lbA, q.ubA, stream); if (rc) return rc; }
  fsaempc_qp_desc qd{nV, fsaempc_ltv_nC(desc->model, desc->N), desc->batch, 0};
  rc = fsaempc_qp_solve_batch_device_s(&qd, hint, q.H, q.g, q.A, q.lb, q.ub, q.lbA, q.ubA, opts, c.z, fval, exitflag, iter,
                                       lambda, aux, c.qpws, (long long)c.qp_bytes, stream);
  if (rc) return rc;
  { Range r("fsaempc.ltv.post");
    hipError_t e = ltv_post_launch(nx, desc->N, ns, s.blocked ? &s.bm : nullptr, desc->batch, c.z, q.pred, q.Bt, q.qconst, u_opt, x_opt, slack, fval, st);
    if ((rc = launched(e, "ltv_post_launch"))) return rc; }
  if (timing) if ((rc = launched(hipEventRecord(g_evf[1], st), "hipEventRecord"))) return rc;
  return 0;
}

/* ---- the entries: the general one of each family is _c; the others forward to it with NULL for what they do not take ---- */
int fsaempc_ltv_build_qp_batch_device_c(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream) {
  return ltv_build_impl(desc, sp, par, blk, cor, x0, x_ref, x_lin, u_lin, LtvQp{H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst}, stream, false);
}
int fsaempc_ltv_build_qp_batch_device_b(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const fsaempc_ltv_blocking* blk,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream) {
  if (!blk) return fail(FSAEMPC_ERR_ARG, "null argument");   // (this entry is for a blocking)
  return fsaempc_ltv_build_qp_batch_device_c(desc, sp, par, blk, nullptr, x0, x_ref, x_lin, u_lin, H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst, stream);
}
int fsaempc_ltv_build_qp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream) {
  return fsaempc_ltv_build_qp_batch_device_c(desc, sp, par, nullptr, nullptr, x0, x_ref, x_lin, u_lin, H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst, stream);
}
int fsaempc_ltv_build_qp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                      double* pred, double* Bt, double* qconst, void* stream) {
  return fsaempc_ltv_build_qp_batch_device_c(desc, sp, nullptr, nullptr, nullptr, x0, x_ref, x_lin, u_lin, H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst, stream);
}
int fsaempc_nlp_build_qp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                        const double* x0, const double* x_ref, const double* u_lin,
                                        double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                        double* pred, double* Bt, double* qconst, void* stream) {
  return ltv_build_impl(desc, sp, par, nullptr, nullptr, x0, x_ref, nullptr, u_lin, LtvQp{H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst}, stream, true);
}
int fsaempc_nlp_build_qp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* u_lin,
                                      double* H, double* g, double* A, double* lb, double* ub, double* lbA, double* ubA,
                                      double* pred, double* Bt, double* qconst, void* stream) {
  return fsaempc_nlp_build_qp_batch_device_p(desc, sp, nullptr, x0, x_ref, u_lin, H, g, A, lb, ub, lbA, ubA, pred, Bt, qconst, stream);
}

long long fsaempc_ltv_workspace_bytes(const fsaempc_ltv_desc* desc) {
  if (!desc || desc->N <= 0 || desc->batch < 0) return FSAEMPC_ERR_ARG;
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  return (long long)ltv_ws(desc, fsaempc_ltv_nV(desc->model, desc->N), -1, nullptr).total;
}
long long fsaempc_ltv_workspace_bytes_b(const fsaempc_ltv_desc* desc, const fsaempc_ltv_blocking* blk) {
  if (!desc || desc->batch < 0) return FSAEMPC_ERR_ARG;
  if (!blk) return fail(FSAEMPC_ERR_ARG, "null argument");
  LtvShape s;
  if (int rc = ltv_shape(desc, blk, nullptr, true, &s)) return rc;
  return (long long)ltv_ws(desc, s.nV(desc), s.slack_hint(desc), nullptr).total;
}

int fsaempc_ltv_step_batch_device_c(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_ltv_blocking* blk, const fsaempc_corridor* cor,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream) {
  return ltv_step_impl(desc, sp, par, blk, cor, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, lambda, aux,
                       workspace, workspace_bytes, stream);
}
int fsaempc_ltv_step_batch_device_b(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_ltv_blocking* blk,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream) {
  if (!blk) return fail(FSAEMPC_ERR_ARG, "null argument");   // (this entry is for a blocking)
  return ltv_step_impl(desc, sp, par, blk, nullptr, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, lambda, aux,
                       workspace, workspace_bytes, stream);
}
int fsaempc_ltv_step_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                    const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                    int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                    void* workspace, long long workspace_bytes, void* stream) {
  return ltv_step_impl(desc, sp, par, nullptr, nullptr, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, lambda, aux,
                       workspace, workspace_bytes, stream);
}
int fsaempc_ltv_step_batch_device_lambda(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                         const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                         const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                         int* exitflag, int* iter, double* lambda, const fsaempc_qp_aux* aux,
                                         void* workspace, long long workspace_bytes, void* stream) {
  if (!lambda) return fail(FSAEMPC_ERR_ARG, "null argument (lambda)");
  return ltv_step_impl(desc, sp, nullptr, nullptr, nullptr, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, lambda, aux,
                       workspace, workspace_bytes, stream);
}
int fsaempc_ltv_step_batch_device_aux(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                      int* exitflag, int* iter, const fsaempc_qp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return ltv_step_impl(desc, sp, nullptr, nullptr, nullptr, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, nullptr, aux,
                       workspace, workspace_bytes, stream);
}
int fsaempc_ltv_step_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                                  const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                  const fsaempc_qp_opts* opts, double* u_opt, double* x_opt, double* slack, double* fval,
                                  int* exitflag, int* iter, void* workspace, long long workspace_bytes, void* stream) {
  return ltv_step_impl(desc, sp, nullptr, nullptr, nullptr, x0, x_ref, x_lin, u_lin, opts, u_opt, x_opt, slack, fval, exitflag, iter, nullptr, nullptr,
                       workspace, workspace_bytes, stream);
}

/* ---- sensitivities of the LTV-MPC step ---- */
int fsaempc_ltv_affine_maps_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const double* x_lin, const double* u_lin,
                                         double* Abar, double* Crow, void* stream) {
  int rc = ltv_check(desc, sp); if (rc) return rc;
  if (!x_lin || !u_lin || !Abar || !Crow) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (ltv_affine_lds_bytes(fsaempc_ltv_nx(desc->model), desc->N) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "horizon too long for the LDS staging");
  if (desc->batch == 0) return 0;
  return launched(ltv_affine_launch(ltv_params(desc, sp, x_lin, u_lin), desc->batch, Abar, Crow, (hipStream_t)stream), "ltv_affine_launch");
}

// the forward's layout up to its solver's region (the QP tensors stay; the solver's workspace is not needed here) | the cotangents
// and the affine maps | the VJP kernel's workspace
struct LtvVjpWs { LtvWs f; double *zbar, *fb, *gbar, *lbAbar, *ubAbar, *Abar, *Crow; char* vjpws; size_t vjp_bytes, total; };
static LtvVjpWs ltv_vjp_ws(const fsaempc_ltv_desc* d, int k, void* base) {
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N, K = k > 0 ? k : 1;
  const size_t nV = fsaempc_ltv_nV(d->model, d->N), nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  LtvVjpWs c;
  c.f = ltv_ws(d, (int)nV, -1, base);
  Bump b(base, c.f.total - c.f.qp_bytes);
  c.zbar = b.take<double>(B * K * nV); c.fb = b.take<double>(B * K); c.gbar = b.take<double>(B * K * nV);
  c.lbAbar = b.take<double>(B * K * nC); c.ubAbar = b.take<double>(B * K * nC);
  c.Abar = b.take<double>(B * R * nx); c.Crow = b.take<double>(B * nC * nx);
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  c.vjpws = take_solver(b, fsaempc_qp_vjp_workspace_bytes(&q), &c.vjp_bytes);
  c.total = b.off;
  return c;
}

long long fsaempc_ltv_step_vjp_workspace_bytes(const fsaempc_ltv_desc* desc, int k) {
  if (!desc || desc->N <= 0 || desc->batch < 0 || k < 1) return FSAEMPC_ERR_ARG;
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  return (long long)ltv_vjp_ws(desc, k, nullptr).total;
}

int fsaempc_ltv_step_vjp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, int k,
                                      const double* x0, const double* x_ref, const double* x_lin, const double* u_lin,
                                      const double* u_opt, const double* slack, const double* lambda, const int* exitflag, const int* polished,
                                      const fsaempc_qp_opts* opts, const fsaempc_ltv_vjp_io* io, int* status,
                                      void* workspace, long long workspace_bytes, void* stream) {
  int rc = ltv_check(desc, sp); if (rc) return rc;
  if (k < 1) return fail(FSAEMPC_ERR_ARG, "k >= 1 cotangent columns");
  if (!x0 || !x_ref || !x_lin || !u_lin || !u_opt || !slack || !lambda || !exitflag || !io || !io->x0bar || !status || !workspace)
    return fail(FSAEMPC_ERR_ARG, "null argument");
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  if (ltv_affine_lds_bytes(fsaempc_ltv_nx(desc->model), desc->N) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "horizon too long for the LDS staging");
  if (desc->batch == 0) return 0;
  const LtvVjpWs c = ltv_vjp_ws(desc, k, workspace);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const LtvQp& f = c.f.q;
  const int nx = fsaempc_ltv_nx(desc->model), N = desc->N, ns = ltv_ns(desc->model);
  const int nV = fsaempc_ltv_nV(desc->model, N), nC = fsaempc_ltv_nC(desc->model, N), B = desc->batch;
  hipStream_t st = (hipStream_t)stream;
  Range whole("fsaempc.ltv.step_vjp");
  // the QP of the step (the build is deterministic: the same QP the forward solved) and the affine maps
  rc = ltv_build_shaped(desc, sp, nullptr, LtvShape(), x0, x_ref, x_lin, u_lin, f, stream, false, nullptr);
  if (rc) return rc;
  rc = fsaempc_ltv_affine_maps_batch_device(desc, sp, x_lin, u_lin, c.Abar, c.Crow, stream);
  if (rc) return rc;
  if ((rc = launched(ltv_vjp_pre_launch(nx, N, ns, B, k, f.Bt, u_opt, slack, io->ubar, io->xbar, io->sbar, c.f.z, c.zbar, st), "ltv_vjp_pre_launch"))) return rc;
  if (io->fbar) if ((rc = launched(hipMemcpyAsync(c.fb, io->fbar, sizeof(double) * (size_t)B * k, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync"))) return rc;
  fsaempc_qp_desc q{nV, nC, B, 0};
  fsaempc_qp_vjp_io qio{c.zbar, io->fbar ? c.fb : nullptr, c.gbar, nullptr, nullptr, c.lbAbar, c.ubAbar, nullptr, nullptr};
  rc = fsaempc_qp_vjp_batch_device(&q, k, f.H, f.g, f.A, f.lb, f.ub, f.lbA, f.ubA, c.f.z, lambda,
                                   exitflag, polished, opts, &qio, status, c.vjpws, (long long)c.vjp_bytes, stream);
  if (rc) return rc;
  return launched(ltv_vjp_chain_launch(nx, N, B, k, f.Bt, f.pred, x_ref, c.Abar, c.Crow, c.gbar, c.lbAbar, c.ubAbar,
                                       io->xbar, io->fbar, status, io->x0bar, io->xrefbar, st), "ltv_vjp_chain_launch");
}

/* ---- batched SQP of the nonlinear MPC step ---- */
void fsaempc_sqp_default_opts(fsaempc_sqp_opts* o) {
  if (!o) return;
  o->max_sweeps = 20; o->trials = 8; o->tol_step = 1e-6; o->tol_feas = 1e-6; o->armijo = 1e-4; o->rho0 = 1.0; o->warm_start = 1;
}

// the active list and its count | the gathered sub-batch and its start | its QP tensors | the QP's results | the merit state | the solver's
struct SqpWs {
  int *idx, *cnt; double *gx0, *gxr, *gu, *xinit; LtvQp q; double *z, *qf; int *qflag, *qit; double *lam, *rho, *J, *viol, *vmax;
  char* qpws; size_t qp_bytes, total;
};
static SqpWs sqp_ws(const fsaempc_ltv_desc* d, void* base) {
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N;
  const size_t nV = fsaempc_ltv_nV(d->model, d->N), nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  Bump b(base);
  SqpWs c;
  c.idx = b.take<int>(B); c.cnt = b.take<int>(1);
  c.gx0 = b.take<double>(B * nx); c.gxr = b.take<double>(B * R); c.gu = b.take<double>(B * 2 * N); c.xinit = b.take<double>(B * nV);
  c.q = take_qp(b, B, nV, nC, R);
  c.z = b.take<double>(B * nV); c.qf = b.take<double>(B); c.qflag = b.take<int>(B); c.qit = b.take<int>(B); c.lam = b.take<double>(B * (nV + nC));
  c.rho = b.take<double>(B); c.J = b.take<double>(B); c.viol = b.take<double>(B); c.vmax = b.take<double>(B);
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  c.qpws = take_solver(b, fsaempc_qp_workspace_bytes(&q), &c.qp_bytes);
  c.total = b.off;
  return c;
}

long long fsaempc_sqp_workspace_bytes(const fsaempc_ltv_desc* desc) {
  if (!desc || desc->N <= 0 || desc->batch < 0) return FSAEMPC_ERR_ARG;
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  return (long long)sqp_ws(desc, nullptr).total;
}

// The one body behind the three entries below.
// (build, initial rollout and line search all read the block: instance i of a compacted sub-batch finds its own through the index list)
// skip (optional): instances with skip[i] != 0 get status FSAEMPC_SQP_SKIPPED right after the initial rollout, so no compaction lists them
static int sqp_impl(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                    const double* x0, const double* x_ref, const double* u_init, const int* skip,
                    const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                    double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                    const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  int rc = ltv_check(desc, sp); if (rc) return rc;
  if (!x0 || !x_ref || !u_init || !u_opt || !x_opt || !slack || !fval || !status || !sweeps || !workspace) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  if (ltv_build_lds_bytes(fsaempc_ltv_nx(desc->model), desc->N, 256, true) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "horizon too long for the LDS staging");
  fsaempc_sqp_opts o; if (sqp_opts) o = *sqp_opts; else fsaempc_sqp_default_opts(&o);
  if (o.max_sweeps < 1 || o.trials < 1 || o.trials > 64 || !(o.tol_step >= 0) || !(o.tol_feas >= 0) || !(o.armijo >= 0) || !(o.rho0 >= 0))
    return fail(FSAEMPC_ERR_ARG, "bad SQP options (max_sweeps >= 1, 1 <= trials <= 64, tolerances / armijo / rho0 >= 0)");
  if (desc->batch == 0) return 0;
  const SqpWs c = sqp_ws(desc, workspace);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const LtvQp& q = c.q;
  hipStream_t st = (hipStream_t)stream;
  const int nx = fsaempc_ltv_nx(desc->model), N = desc->N, nV = fsaempc_ltv_nV(desc->model, N), nC = fsaempc_ltv_nC(desc->model, N);
  SqpParams P; memset(&P, 0, sizeof(P));
  P.nx = nx; P.N = N; P.integ = ltv_integ(desc); P.B = desc->batch; P.dt = desc->dt; set_spline(&P, sp);
  P.x0 = x0; P.x_ref = x_ref; P.u = u_opt; P.x = x_opt; P.s = slack; P.fval = fval; P.status = status; P.sweeps = sweeps;
  P.rho = c.rho; P.J = c.J; P.viol = c.viol; P.vmax = c.vmax;
  if (aux) { P.lambda_out = aux->lambda; P.qp_iter = aux->qp_iter; P.step_norm = aux->step_norm; P.hard_viol = aux->hard_viol; P.merit = aux->merit; }
  P.max_sweeps = o.max_sweeps; P.trials = o.trials; P.tol_step = o.tol_step; P.tol_feas = o.tol_feas; P.armijo = o.armijo; P.rho0 = o.rho0;
  Range whole("fsaempc.sqp");
  const bool timing = g_timing.load();
  auto stamp = [&](int i) { return timing ? launched(hipEventRecord(g_evs[i], st), "hipEventRecord") : 0; };
  for (double& v : g_sqp_ms) v = 0;
  if ((rc = launched(sqp_init_launch(P, u_init, st, par_values(par), par_stride(par)), "sqp_init_launch"))) return rc;
  if (skip && (rc = launched(sqp_skip_launch(desc->batch, skip, status, st), "sqp_skip_launch"))) return rc;
  for (int sweep = 0; sweep < o.max_sweeps; ++sweep) {
    if ((rc = stamp(0))) return rc;
    int cnt = 0;
    { Range r("fsaempc.sqp.compact");
      hipError_t e = sqp_compact_launch(status, desc->batch, c.idx, c.cnt, st);
      if (e == hipSuccess) e = hipMemcpyAsync(&cnt, c.cnt, sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);   // the one read of the sweep
      if ((rc = launched(e, "sqp compaction"))) return rc; }
    if (cnt == 0) break;
    double* xinit = o.warm_start ? c.xinit : nullptr;
    if ((rc = launched(sqp_gather_launch(P, c.idx, cnt, c.gx0, c.gxr, c.gu, xinit, nV, st), "sqp_gather_launch"))) return rc;
    if ((rc = stamp(1))) return rc;
    fsaempc_ltv_desc sub = *desc; sub.batch = cnt;
    { Range r("fsaempc.sqp.build");
      rc = ltv_build_shaped(&sub, sp, par, LtvShape(), c.gx0, c.gxr, nullptr, c.gu, q, stream, true, c.idx); }
    if (rc) return rc;
    if ((rc = stamp(2))) return rc;
    fsaempc_qp_desc qd{nV, nC, cnt, 0};
    fsaempc_qp_aux qa{nullptr, nullptr, xinit, nullptr};
    rc = fsaempc_qp_solve_batch_device_aux(&qd, q.H, q.g, q.A, q.lb, q.ub, q.lbA, q.ubA, qp_opts, c.z, c.qf,
                                           c.qflag, c.qit, c.lam, &qa, c.qpws, (long long)c.qp_bytes, stream);
    if (rc) return rc;
    if ((rc = stamp(3))) return rc;
    { Range r("fsaempc.sqp.linesearch");
      rc = launched(sqp_linesearch_launch(P, c.idx, cnt, sweep, c.z, c.qf, q.qconst, c.qflag, c.qit, c.lam, st,
                                          par_values(par), par_stride(par)), "sqp_linesearch_launch"); }
    if (rc) return rc;
    if (timing) {
      hipError_t e = hipEventRecord(g_evs[4], st); if (e == hipSuccess) e = hipEventSynchronize(g_evs[4]);
      if ((rc = launched(e, "hipEventRecord"))) return rc;
      for (int k = 0; k < 4; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, g_evs[k], g_evs[k + 1]) == hipSuccess) g_sqp_ms[k] += ms; }
    }
  }
  return 0;
}

int fsaempc_sqp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                             const double* x0, const double* x_ref, const double* u_init,
                             const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                             double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                             const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return sqp_impl(desc, sp, nullptr, x0, x_ref, u_init, nullptr, qp_opts, sqp_opts, u_opt, x_opt, slack, fval, status, sweeps, aux,
                  workspace, workspace_bytes, stream);
}
int fsaempc_sqp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                               const double* x0, const double* x_ref, const double* u_init,
                               const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                               double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                               const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return sqp_impl(desc, sp, par, x0, x_ref, u_init, nullptr, qp_opts, sqp_opts, u_opt, x_opt, slack, fval, status, sweeps, aux,
                  workspace, workspace_bytes, stream);
}
int fsaempc_sqp_batch_device_m(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                               const double* x0, const double* x_ref, const double* u_init, const int* skip,
                               const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                               double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                               const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return sqp_impl(desc, sp, par, x0, x_ref, u_init, skip, qp_opts, sqp_opts, u_opt, x_opt, slack, fval, status, sweeps, aux,
                  workspace, workspace_bytes, stream);
}

}  // extern "C"
