// capi_qp.hip -- the C ABI of libfsaempc.so (include/fsaempc.h), QP part: the batched solve and its VJP on device buffers, the
// host-buffer paths (fsaempc_qp_solve_batch, the qpOASES_sequence handles), the self-tests, the dump switch and the timing getters;
// and the one definition of what the units share (capi_common.h).  Host-side glue only: argument checks, workspace layout, kernel
// launches.  There is no CPU compute path: without a gfx950 device every entry point fails with FSAEMPC_ERR_NODEVICE /
// FSAEMPC_ERR_HIP.  The host-buffer paths share the data scans, the checked copies and the layout of the per-call vectors.
#include <mutex>
#include <vector>
#include "capi_common.h"
#include "qp_solver.h"
#include "qp_sens.h"

namespace capi __attribute__((visibility("hidden"))) {
__thread char g_err[512] = "";
std::atomic<double*> g_dump{nullptr}; std::atomic<int> g_dump_stage{0};
std::atomic<bool> g_timing{false}; hipEvent_t g_ev[3] = {nullptr, nullptr, nullptr};
hipEvent_t g_evf[2] = {nullptr, nullptr};
hipEvent_t g_evs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
double g_sqp_ms[4] = {0, 0, 0, 0};
}  // namespace capi
using namespace capi;

extern "C" {

const char* fsaempc_last_error(void) { return g_err; }

void fsaempc_qp_default_opts(fsaempc_qp_opts* o) {
  if (!o) return;
  o->tol = 1e-8; o->tol_loose = 1e-6; o->tol_x = 1e-7; o->inf_bound = 1e9; o->max_iter = 100; o->polish = 1;
}

// n_slack of the _s entries: a negative value means "none given" (QP_NO_SLACK_HINT), else 0, 1 or 4 trailing slack variables
static bool slack_hint_ok(const fsaempc_qp_desc* desc, int n_slack) {
  if (n_slack < 0) return true;
  return (n_slack == 0 || n_slack == 1 || n_slack == 4) && desc->nV > n_slack;
}
static int slack_hint(int n_slack) { return n_slack < 0 ? QP_NO_SLACK_HINT : n_slack; }

long long fsaempc_qp_workspace_bytes_s(const fsaempc_qp_desc* desc, int n_slack) {
  if (!desc || desc->nV <= 0 || desc->nC < 0 || desc->batch < 0 || !slack_hint_ok(desc, n_slack)) return FSAEMPC_ERR_ARG;
  if (desc->nV > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  QpDims d; qp_make_dims(desc->nV, desc->nC, &d, slack_hint(n_slack));
  if (d.T > QP_MAX_T) return FSAEMPC_ERR_DIM;
  return (long long)(d.ws_per_qp * sizeof(double) * (size_t)(desc->batch > 0 ? desc->batch : 1) + qp_order_bytes(desc->batch));
}
long long fsaempc_qp_workspace_bytes(const fsaempc_qp_desc* desc) { return fsaempc_qp_workspace_bytes_s(desc, -1); }

int fsaempc_qp_layout(const fsaempc_qp_desc* desc, int n_slack, int out[4]) {
  if (!desc || !out || desc->nV <= 0 || desc->nC < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!slack_hint_ok(desc, n_slack)) return fail(FSAEMPC_ERR_ARG, "n_slack must be 0, 1 or 4 (negative: none given) and smaller than nV");
  if (desc->nV > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  QpDims d; qp_make_dims(desc->nV, desc->nC, &d, slack_hint(n_slack));
  if (d.T > QP_MAX_T) return fail(FSAEMPC_ERR_DIM, "more column tiles than the kernels are built for");
  out[0] = d.T; out[1] = d.NB; out[2] = d.n; out[3] = qp_runs_wavefront_kernel(d) ? 1 : 0;
  return 0;
}

int fsaempc_qp_solve_batch_device(const fsaempc_qp_desc* desc, const double* H, const double* g, const double* A,
                                  const double* lb, const double* ub, const double* lbA, const double* ubA,
                                  const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter,
                                  double* lambda, void* workspace, long long workspace_bytes, void* stream) {
  return fsaempc_qp_solve_batch_device_aux(desc, H, g, A, lb, ub, lbA, ubA, opts, x, fval, exitflag, iter, lambda, nullptr, workspace, workspace_bytes, stream);
}

int fsaempc_qp_solve_batch_device_aux(const fsaempc_qp_desc* desc, const double* H, const double* g, const double* A,
                                      const double* lb, const double* ub, const double* lbA, const double* ubA,
                                      const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter,
                                      double* lambda, const fsaempc_qp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return fsaempc_qp_solve_batch_device_s(desc, -1, H, g, A, lb, ub, lbA, ubA, opts, x, fval, exitflag, iter, lambda, aux, workspace, workspace_bytes, stream);
}

int fsaempc_qp_solve_batch_device_s(const fsaempc_qp_desc* desc, int n_slack, const double* H, const double* g, const double* A,
                                    const double* lb, const double* ub, const double* lbA, const double* ubA,
                                    const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter,
                                    double* lambda, const fsaempc_qp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  if (!desc || !H || !g || !lb || !ub || !x || !fval || !exitflag || !iter || !workspace) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (desc->nV <= 0 || desc->nC < 0 || desc->batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (desc->nC > 0 && (!A || !lbA || !ubA)) return fail(FSAEMPC_ERR_ARG, "nC > 0 needs A, lbA, ubA");
  if (desc->nV > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  if (!slack_hint_ok(desc, n_slack)) return fail(FSAEMPC_ERR_ARG, "n_slack must be 0, 1 or 4 (negative: none given) and smaller than nV");
  if (desc->batch == 0) return 0;
  fsaempc_qp_opts o; if (opts) o = *opts; else fsaempc_qp_default_opts(&o);
  QpParams P; memset(&P, 0, sizeof(P));
  qp_make_dims(desc->nV, desc->nC, &P.d, slack_hint(n_slack));
  if (P.d.T > QP_MAX_T) return fail(FSAEMPC_ERR_DIM, "more column tiles than the kernels are built for");
  const size_t ws_qps = P.d.ws_per_qp * sizeof(double) * (size_t)desc->batch;
  if ((long long)(ws_qps + qp_order_bytes(desc->batch)) > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  const char* no_order = getenv("FSAEMPC_QP_ORDER");   // A/B runs only: FSAEMPC_QP_ORDER=0 solves in index order (read per call)
  if (qp_order_bytes(desc->batch) && !(no_order && no_order[0] == '0')) { P.score = (int*)((char*)workspace + ws_qps); P.order = P.score + desc->batch; }
  const bool wg = !qp_runs_wavefront_kernel(P.d);
  if ((wg ? P.d.lds_wg : P.d.lds_solve) > 160 * 1024 || P.d.lds_prep > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "problem exceeds the 160 KiB LDS budget of the kernels");
  P.H = H; P.g = g; P.A = A; P.lb = lb; P.ub = ub; P.lbA = lbA; P.ubA = ubA;
  P.ws = (double*)workspace; P.x = x; P.fval = fval; P.lambda = lambda; P.exitflag = exitflag; P.iter = iter;
  P.tol = o.tol; P.tol_loose = o.tol_loose; P.tol_x = o.tol_x; P.inf_bound = o.inf_bound; P.max_iter = o.max_iter; P.polish = o.polish; P.polished = aux ? aux->polished : nullptr; P.kkt = aux ? aux->kkt : nullptr; P.x_init = aux ? aux->x_init : nullptr; P.score_in = aux ? aux->difficulty : nullptr;
  P.shared_HA = desc->shared_HA;
  { const int st = g_dump_stage.load(); P.dump = g_dump.load(); P.dump_stage = st & 0xff; P.dump_iter = st >> 8; }
  const bool timing = g_timing.load();
  if (timing) if (int rc = launched(hipEventRecord(g_ev[0], (hipStream_t)stream), "hipEventRecord")) return rc;
  { Range r("fsaempc.qp.prep+solve");   // (prep, order and solve kernels are enqueued by one call; the kernel trace separates them)
    if (int rc = launched(qp_launch(P, desc->batch, (hipStream_t)stream, timing ? g_ev[1] : nullptr), "qp_launch")) return rc; }
  if (timing) if (int rc = launched(hipEventRecord(g_ev[2], (hipStream_t)stream), "hipEventRecord")) return rc;
  return 0;
}

// ---- VJP of the batched QP solve (qp_sens.hip) ----
static int qp_vjp_plan(const fsaempc_qp_desc* desc, int k, QpsParams* P) {
  if (!desc || desc->nV <= 0 || desc->nC < 0 || desc->batch < 0 || k < 1) return fail(FSAEMPC_ERR_ARG, "bad dimensions (nV > 0, nC >= 0, batch >= 0, k >= 1)");
  if (desc->nV > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  memset(P, 0, sizeof(*P));
  P->n = desc->nV; P->m = desc->nC; P->B = desc->batch; P->k = k; P->shared_HA = desc->shared_HA ? 1 : 0;
  qps_plan(P);
  if (P->lds_bytes > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "problem exceeds the 160 KiB LDS budget of the VJP kernel");
  return 0;
}
long long fsaempc_qp_vjp_workspace_bytes(const fsaempc_qp_desc* desc) {
  QpsParams P;
  const int rc = qp_vjp_plan(desc, 1, &P);
  return rc ? rc : (long long)qps_plan(&P);
}
int fsaempc_qp_vjp_batch_device(const fsaempc_qp_desc* desc, int k, const double* H, const double* g, const double* A,
                                const double* lb, const double* ub, const double* lbA, const double* ubA,
                                const double* x, const double* lambda, const int* exitflag, const int* polished,
                                const fsaempc_qp_opts* opts, const fsaempc_qp_vjp_io* io, int* status,
                                void* workspace, long long workspace_bytes, void* stream) {
  QpsParams P;
  int rc = qp_vjp_plan(desc, k, &P); if (rc) return rc;
  if (!H || !g || !lb || !ub || !x || !lambda || !exitflag || !io || !io->xbar || !io->gbar || !status || !workspace)
    return fail(FSAEMPC_ERR_ARG, "null argument");
  if (desc->nC > 0 && (!A || !lbA || !ubA)) return fail(FSAEMPC_ERR_ARG, "nC > 0 needs A, lbA, ubA");
  if (desc->shared_HA && (io->Hbar || io->Abar)) return fail(FSAEMPC_ERR_ARG, "Hbar / Abar are per instance: not available with shared_HA");
  if (desc->batch == 0) return 0;
  if ((long long)qps_plan(&P) > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  fsaempc_qp_opts o; if (opts) o = *opts; else fsaempc_qp_default_opts(&o);
  P.inf_bound = o.inf_bound; P.tol = o.tol;
  P.H = H; P.g = g; P.A = A; P.lb = lb; P.ub = ub; P.lbA = lbA; P.ubA = ubA;
  P.x = x; P.lam = lambda; P.exitflag = exitflag; P.polished = polished;
  P.xbar = io->xbar; P.fbar = io->fbar; P.gbar = io->gbar; P.lbbar = io->lbbar; P.ubbar = io->ubbar; P.lbAbar = io->lbAbar; P.ubAbar = io->ubAbar;
  P.Hbar = io->Hbar; P.Abar = io->Abar; P.status = status; P.ws = (double*)workspace;
  Range r("fsaempc.qp.vjp");
  return launched(qps_launch(P, (hipStream_t)stream), "qps_launch");
}

// ---- host-buffer QP paths: fsaempc_qp_solve_batch and the qpOASES_sequence handles ----
// The data checks of the original gateway ("Argument %d contains 'NaN' !"): NaN anywhere and Inf in H, g, A are refused.  A null
// pointer is a vector this call does not bring (the handles upload H, A and the per-call vectors at different times).
static int qp_scan(const double* H, size_t nH, const double* g, size_t ng, const double* A, size_t nA,
                   const double* lb, const double* ub, size_t nb, const double* lbA, const double* ubA, size_t nbA) {
  auto finite = [](const double* v, size_t cnt) { if (v) for (size_t i = 0; i < cnt; ++i) if (!isfinite(v[i])) return false; return true; };
  auto no_nan = [](const double* v, size_t cnt) { if (v) for (size_t i = 0; i < cnt; ++i) if (isnan(v[i])) return false; return true; };
  if (!finite(H, nH)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Argument 1 contains 'NaN' or 'Inf' !");
  if (!finite(g, ng)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Argument 2 contains 'NaN' or 'Inf' !");
  if (!finite(A, nA)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Argument 3 contains 'NaN' or 'Inf' !");
  if (!no_nan(lb, nb) || !no_nan(ub, nb)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): bounds contain 'NaN' !");
  if (!no_nan(lbA, nbA) || !no_nan(ubA, nbA)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): constraint bounds contain 'NaN' !");
  return 0;
}
// checked copies; both do nothing once *rc is set, to_host also for an output the caller did not ask for
static void to_device(int* rc, void* dst, const void* src, size_t bytes) {
  if (*rc || bytes == 0) return;
  *rc = launched(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
}
static void to_host(int* rc, void* dst, const void* src, size_t bytes) {
  if (*rc || !dst) return;
  *rc = launched(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
}
// the per-call vectors of a host-buffer solve, carved from one device allocation: g lb ub lbA ubA | x fval lambda | exitflag iter
struct QpVecs {
  double *g, *lb, *ub, *lbA, *ubA, *x, *fval, *lam; int *flag, *iter;
  static size_t doubles(size_t n, size_t m, size_t B) { return B * (4 * n + 2 * m + 1 + (n + m)) + B + 16; }
  QpVecs(double* p, size_t n, size_t m, size_t B) {
    g = p; p += B * n; lb = p; p += B * n; ub = p; p += B * n; lbA = p; p += B * m; ubA = p; p += B * m;
    x = p; p += B * n; fval = p; p += B; lam = p; p += B * (n + m);
    flag = (int*)p; iter = flag + B;
  }
};
// vectors to the device, one solve on the null stream with H and A already there, the results the caller asked for back
static int qp_host_solve(const fsaempc_qp_desc* d, const double* dH, const double* dA, const QpVecs& v, const double* g, const double* lb,
                         const double* ub, const double* lbA, const double* ubA, const fsaempc_qp_opts* opts, double* x, double* fval,
                         int* exitflag, int* iter, double* lambda, void* dws, long long wsb) {
  const size_t n = d->nV, m = d->nC, B = d->batch, D = sizeof(double);
  int rc = 0;
  to_device(&rc, v.g, g, B * n * D); to_device(&rc, v.lb, lb, B * n * D); to_device(&rc, v.ub, ub, B * n * D);
  to_device(&rc, v.lbA, lbA, B * m * D); to_device(&rc, v.ubA, ubA, B * m * D);
  if (rc == 0) rc = fsaempc_qp_solve_batch_device(d, dH, v.g, m ? dA : nullptr, v.lb, v.ub, m ? v.lbA : nullptr, m ? v.ubA : nullptr, opts,
                                                  v.x, v.fval, v.flag, v.iter, v.lam, dws, wsb, nullptr);
  if (rc == 0) rc = launched(hipDeviceSynchronize(), "solve");
  to_host(&rc, x, v.x, B * n * D); to_host(&rc, fval, v.fval, B * D); to_host(&rc, exitflag, v.flag, B * sizeof(int));
  to_host(&rc, iter, v.iter, B * sizeof(int)); to_host(&rc, lambda, v.lam, B * (n + m) * D);
  return rc;
}

int fsaempc_qp_solve_batch(const fsaempc_qp_desc* desc, const double* H, const double* g, const double* A,
                           const double* lb, const double* ub, const double* lbA, const double* ubA,
                           const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter, double* lambda) {
  if (!desc || !H || !g || !lb || !ub || !x) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (desc->nV <= 0 || desc->nC < 0 || desc->batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (desc->nC > 0 && (!A || !lbA || !ubA)) return fail(FSAEMPC_ERR_ARG, "nC > 0 needs A, lbA, ubA");
  if (desc->nV > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  const size_t n = desc->nV, m = desc->nC, B = desc->batch, BH = desc->shared_HA ? 1 : B;
  if (B == 0) return 0;
  if (int rc = qp_scan(H, BH * n * n, g, B * n, A, BH * m * n, lb, ub, B * n, lbA, ubA, B * m)) return rc;
  long long wsb = fsaempc_qp_workspace_bytes(desc);
  if (wsb < 0) return fail((int)wsb, "workspace size");
  const size_t szH = BH * n * n, szA = BH * m * n, szv = QpVecs::doubles(n, m, B);   // H | A | the vectors | the solver's workspace
  double* dev = nullptr;
  if (int rc = launched(hipMalloc((void**)&dev, (szH + szA + szv) * sizeof(double) + (size_t)wsb + 4096), "hipMalloc")) return rc;
  double *dH = dev, *dA = dev + szH;
  void* dws = (void*)(((uintptr_t)(dA + szA + szv) + 255) & ~(uintptr_t)255);
  int rc = 0;
  to_device(&rc, dH, H, szH * sizeof(double)); to_device(&rc, dA, A, szA * sizeof(double));
  if (rc == 0) rc = qp_host_solve(desc, dH, dA, QpVecs(dA + szA, n, m, B), g, lb, ub, lbA, ubA, opts, x, fval, exitflag, iter, lambda, dws, wsb);
  (void)hipFree(dev);
  return rc;
}

// ---- qpOASES_sequence handles (qpOASES_sequence.m:23-78) ----
// A handle owns device copies of H and A (uploaded by 'i' / 'm' only), the solver workspace and the per-call vectors (grown to
// the largest k seen), so a hot start moves (3 nV + 2 nC) k doubles to the device and the results back -- no allocation, no
// matrix upload.  Every solve is a cold interior-point solve; the handle also remembers the working set of its last solve
// (first column) for the 'e' call.
namespace {
struct SeqQP {
  int nV = 0, nC = 0, kcap = 0;
  bool used = false;
  double *dH = nullptr, *dA = nullptr, *dvec = nullptr; void* dws = nullptr; long long wsb = 0;
  std::vector<signed char> wsB, wsC;   // -1 lower / 0 inactive / +1 upper, qpOASES.m:52-62 encoding
  std::vector<double> hA;              // host copy of A (the working set of a solve is derived on the host: it needs A x)
  void release() {
    (void)hipFree(dH); (void)hipFree(dA); (void)hipFree(dvec); (void)hipFree(dws);
    dH = dA = dvec = nullptr; dws = nullptr; kcap = 0; wsb = 0; used = false; wsB.clear(); wsC.clear(); hA.clear();
  }
};
std::mutex g_seq_mu;
std::vector<SeqQP> g_seq;   // handle = index + 1 (the MEX gateway also hands out small integers)
SeqQP* seq_get(int handle) { return (handle >= 1 && handle <= (int)g_seq.size() && g_seq[handle - 1].used) ? &g_seq[handle - 1] : nullptr; }
int seq_upload_matrices(SeqQP* q, const double* H, const double* A) {
  const size_t n = q->nV, m = q->nC;
  if (int rc = qp_scan(H, n * n, nullptr, 0, A, m * n, nullptr, nullptr, 0, nullptr, nullptr, 0)) return rc;
  if (!q->dH) if (int rc = launched(hipMalloc((void**)&q->dH, n * n * sizeof(double)), "hipMalloc")) return rc;
  if (m && !q->dA) if (int rc = launched(hipMalloc((void**)&q->dA, m * n * sizeof(double)), "hipMalloc")) return rc;
  int rc = 0;
  to_device(&rc, q->dH, H, n * n * sizeof(double)); to_device(&rc, q->dA, A, m * n * sizeof(double));
  if (rc) return rc;
  q->hA.assign(A ? A : nullptr, A ? A + m * n : nullptr);
  return 0;
}
int seq_solve(SeqQP* q, const double* g, const double* lb, const double* ub, const double* lbA, const double* ubA, int k,
              const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter, double* lambda, bool remember) {
  const size_t n = q->nV, m = q->nC, B = k;
  if (!g || !lb || !ub || !x || (m && (!lbA || !ubA))) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = qp_scan(nullptr, 0, g, B * n, nullptr, 0, lb, ub, B * n, lbA, ubA, B * m)) return rc;
  fsaempc_qp_desc d{q->nV, q->nC, k, 1};
  if (k > q->kcap) {   // grow the per-call buffers (QpVecs) and the workspace
    (void)hipFree(q->dvec); (void)hipFree(q->dws); q->dvec = nullptr; q->dws = nullptr; q->kcap = 0;
    const long long wsb = fsaempc_qp_workspace_bytes(&d);
    if (wsb < 0) return fail((int)wsb, "workspace size");
    if (int rc = launched(hipMalloc((void**)&q->dvec, QpVecs::doubles(n, m, B) * sizeof(double)), "hipMalloc")) return rc;
    if (int rc = launched(hipMalloc(&q->dws, (size_t)wsb), "hipMalloc")) return rc;
    q->kcap = k; q->wsb = wsb;
  }
  const QpVecs dv(q->dvec, n, m, B);
  int rc = qp_host_solve(&d, q->dH, q->dA, dv, g, lb, ub, lbA, ubA, opts, x, fval, exitflag, iter, lambda, q->dws, q->wsb);
  std::vector<double> lam0, x0h;
  if (rc == 0 && remember && !lambda) { lam0.resize(n + m); to_host(&rc, lam0.data(), dv.lam, (n + m) * sizeof(double)); }
  if (rc == 0 && remember) { x0h.resize(n); to_host(&rc, x0h.data(), dv.x, n * sizeof(double)); }
  if (rc == 0 && remember) {
    // Working set of the first column (qpOASES.m:52-62 encoding), by the rule the kernels' active-set refinement uses: a side is
    // active iff its multiplier has the side's sign AND exceeds the side's slack.  On a refined vertex that is the same as
    // "multiplier non-zero"; on an interior-point iterate (refinement rejected or switched off, opts->polish = 0) every finite
    // side carries a small non-zero multiplier and the sign alone would put all of them into the set.
    const double* l = lambda ? lambda : lam0.data();
    q->wsB.assign(n, 0); q->wsC.assign(m, 0);
    const double ib = opts ? opts->inf_bound : 1e9;
    for (size_t i = 0; i < n; ++i) {
      const double v = x0h[i];
      if (l[i] > 0 && lb[i] > -ib && l[i] > fabs(v - lb[i])) q->wsB[i] = -1;
      else if (l[i] < 0 && ub[i] < ib && -l[i] > fabs(ub[i] - v)) q->wsB[i] = 1;
    }
    for (size_t r = 0; r < m; ++r) {
      double v = 0.0;
      for (size_t j = 0; j < n; ++j) v += q->hA[j * m + r] * x0h[j];
      const double lr = l[n + r];
      if (lr > 0 && lbA[r] > -ib && lr > fabs(v - lbA[r])) q->wsC[r] = -1;
      else if (lr < 0 && ubA[r] < ib && -lr > fabs(ubA[r] - v)) q->wsC[r] = 1;
    }
  }
  return rc;
}
}  // namespace

int fsaempc_seq_init(int nV, int nC, const double* H, const double* g, const double* A, const double* lb, const double* ub,
                     const double* lbA, const double* ubA, int k, const fsaempc_qp_opts* opts, int* handle,
                     double* x, double* fval, int* exitflag, int* iter, double* lambda) {
  if (!handle || !H || nV <= 0 || nC < 0 || k <= 0 || (nC > 0 && !A)) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): invalid arguments to 'i'");
  if (nV > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_DIM, "nV exceeds FSAEMPC_MAX_NV");
  std::lock_guard<std::mutex> lk(g_seq_mu);
  int idx = -1;
  for (size_t i = 0; i < g_seq.size(); ++i) if (!g_seq[i].used) { idx = (int)i; break; }
  if (idx < 0) { g_seq.emplace_back(); idx = (int)g_seq.size() - 1; }
  SeqQP& q = g_seq[idx];
  q.nV = nV; q.nC = nC; q.used = true;
  *handle = idx + 1;
  int rc = seq_upload_matrices(&q, H, A);
  if (rc == 0) rc = seq_solve(&q, g, lb, ub, lbA, ubA, k, opts, x, fval, exitflag, iter, lambda, true);
  if (rc != 0) { q.release(); *handle = 0; }
  return rc;
}
int fsaempc_seq_hotstart(int handle, int nV, int nC, const double* g, const double* lb, const double* ub, const double* lbA,
                         const double* ubA, int k, const fsaempc_qp_opts* opts, double* x, double* fval, int* exitflag, int* iter, double* lambda) {
  std::lock_guard<std::mutex> lk(g_seq_mu);
  SeqQP* q = seq_get(handle);
  if (!q) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Invalid handle to QP instance!");
  if (nV != q->nV || nC != q->nC) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): QP dimensions must be constant during a sequence!");
  if (k <= 0) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): invalid arguments to 'h'");
  return seq_solve(q, g, lb, ub, lbA, ubA, k, opts, x, fval, exitflag, iter, lambda, true);
}
int fsaempc_seq_hotstart_matrices(int handle, int nV, int nC, const double* H, const double* g, const double* A, const double* lb,
                                  const double* ub, const double* lbA, const double* ubA, int k, const fsaempc_qp_opts* opts,
                                  double* x, double* fval, int* exitflag, int* iter, double* lambda) {
  std::lock_guard<std::mutex> lk(g_seq_mu);
  SeqQP* q = seq_get(handle);
  if (!q) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Invalid handle to QP instance!");
  if (nV != q->nV || nC != q->nC) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): QP dimensions must be constant during a sequence!");
  if (!H || (nC > 0 && !A) || k <= 0) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): invalid arguments to 'm'");
  int rc = seq_upload_matrices(q, H, A);
  if (rc != 0) return rc;
  return seq_solve(q, g, lb, ub, lbA, ubA, k, opts, x, fval, exitflag, iter, lambda, true);
}
// 'e' (qpOASES_sequence.m:64-72): the equality-constrained QP fixed by the working set of the handle's last solve -- sides in the
// working set hold with equality at the new bound values, every other bound / row is dropped ("might be violated").  Does not
// alter the handle.  Solved by the same kernel with lb = ub on the active sides and no bound elsewhere.
int fsaempc_seq_equality(int handle, int nV, int nC, const double* g, const double* lb, const double* ub, const double* lbA,
                         const double* ubA, int k, const fsaempc_qp_opts* opts, double* x, double* lambda, int* workingSetB, int* workingSetC) {
  std::lock_guard<std::mutex> lk(g_seq_mu);
  SeqQP* q = seq_get(handle);
  if (!q) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Invalid handle to QP instance!");
  if (nV != q->nV || nC != q->nC) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): QP dimensions must be constant during a sequence!");
  if (k <= 0 || !g || !lb || !ub || !x || (nC && (!lbA || !ubA))) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): invalid arguments to 'e'");
  if ((int)q->wsB.size() != nV) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): no working set yet (solve with 'i' / 'h' / 'm' first)");
  const size_t n = nV, m = nC, B = k;
  std::vector<double> l2(B * n), u2(B * n), lA2(B * m), uA2(B * m);
  for (size_t j = 0; j < B; ++j) {
    for (size_t i = 0; i < n; ++i) {
      const int w = q->wsB[i]; const double v = w < 0 ? lb[j * n + i] : ub[j * n + i];
      l2[j * n + i] = w ? v : -INFINITY; u2[j * n + i] = w ? v : INFINITY;
    }
    for (size_t i = 0; i < m; ++i) {
      const int w = q->wsC[i]; const double v = w < 0 ? lbA[j * m + i] : ubA[j * m + i];
      lA2[j * m + i] = w ? v : -INFINITY; uA2[j * m + i] = w ? v : INFINITY;
    }
  }
  std::vector<int> fl(B), it(B);
  int rc = seq_solve(q, g, l2.data(), u2.data(), m ? lA2.data() : nullptr, m ? uA2.data() : nullptr, k, opts, x, nullptr, fl.data(), it.data(), lambda, false);
  if (rc != 0) return rc;
  if (workingSetB) for (size_t i = 0; i < n; ++i) workingSetB[i] = q->wsB[i];
  if (workingSetC) for (size_t i = 0; i < m; ++i) workingSetC[i] = q->wsC[i];
  for (size_t j = 0; j < B; ++j) if (fl[j] != 0) return fail(FSAEMPC_ERR_SOLVER, "ERROR (qpOASES): equality-constrained QP could not be solved (working set linearly dependent or infeasible)");
  return 0;
}
int fsaempc_seq_cleanup(int handle) {
  std::lock_guard<std::mutex> lk(g_seq_mu);
  SeqQP* q = seq_get(handle);
  if (!q) return fail(FSAEMPC_ERR_ARG, "ERROR (qpOASES): Invalid handle to QP instance!");   // what main.m:193 would hit with QP == 0
  q->release();
  return 0;
}

/* ---- self-tests, the dump switch, timing ---- */
static int selftest(int (*test)(char* msg, int msglen)) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) return fail(FSAEMPC_ERR_NODEVICE, "no HIP device");
  char msg[256] = "";
  int bad = test(msg, sizeof(msg));
  if (bad != 0) snprintf(g_err, sizeof(g_err), "%s", msg);
  return bad;
}
int fsaempc_selftest_mfma(void) { return selftest(qp_selftest_mfma); }
int fsaempc_selftest_lane_reduce(void) { return selftest(qp_selftest_lane_reduce); }
int fsaempc_selftest_diag_factor(void) { return selftest(qp_selftest_diag_factor); }
int fsaempc_selftest_initial_point(void) { return selftest(qp_selftest_initial_point); }

int fsaempc_debug_set_dump(double* out, int stage) { g_dump.store(out); g_dump_stage.store(stage); return 0; }

int fsaempc_qp_set_timing(int enable) {
  if (enable && !g_ev[0]) {
    for (hipEvent_t& ev : g_ev) if (int rc = launched(hipEventCreate(&ev), "hipEventCreate")) return rc;
    for (hipEvent_t& ev : g_evf) if (int rc = launched(hipEventCreate(&ev), "hipEventCreate")) return rc;
    for (hipEvent_t& ev : g_evs) if (int rc = launched(hipEventCreate(&ev), "hipEventCreate")) return rc;
  }
  g_timing.store(enable != 0);
  return 0;
}

int fsaempc_ltv_get_timing(double* build_ms, double* prep_ms, double* solve_ms, double* post_ms) {
  if (!g_evf[0]) return fail(FSAEMPC_ERR_ARG, "timing was never enabled");
  if (int rc = launched(hipEventSynchronize(g_evf[1]), "hipEventSynchronize (no fused step since timing was enabled?)")) return rc;
  const hipEvent_t ev[5] = {g_evf[0], g_ev[0], g_ev[1], g_ev[2], g_evf[1]};
  float t[4] = {0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) if (int rc = launched(hipEventElapsedTime(&t[i], ev[i], ev[i + 1]), "hipEventElapsedTime")) return rc;
  if (build_ms) *build_ms = t[0];
  if (prep_ms) *prep_ms = t[1];
  if (solve_ms) *solve_ms = t[2];
  if (post_ms) *post_ms = t[3];
  return 0;
}

int fsaempc_qp_get_timing(double* prep_ms, double* solve_ms) {
  if (!g_ev[0]) return fail(FSAEMPC_ERR_ARG, "timing was never enabled");
  if (int rc = launched(hipEventSynchronize(g_ev[2]), "hipEventSynchronize")) return rc;
  float a = 0, b = 0;
  if (int rc = launched(hipEventElapsedTime(&a, g_ev[0], g_ev[1]), "hipEventElapsedTime")) return rc;
  if (int rc = launched(hipEventElapsedTime(&b, g_ev[1], g_ev[2]), "hipEventElapsedTime")) return rc;
  if (prep_ms) *prep_ms = a;
  if (solve_ms) *solve_ms = b;
  return 0;
}

int fsaempc_sqp_get_timing(double* build_ms, double* solve_ms, double* linesearch_ms, double* compact_ms) {
  if (!build_ms || !solve_ms || !linesearch_ms || !compact_ms) return fail(FSAEMPC_ERR_ARG, "null argument");
  *compact_ms = g_sqp_ms[0]; *build_ms = g_sqp_ms[1]; *solve_ms = g_sqp_ms[2]; *linesearch_ms = g_sqp_ms[3];
  return 0;
}

}  // extern "C"
