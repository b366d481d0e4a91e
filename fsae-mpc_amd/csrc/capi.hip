// capi.hip -- the C ABI of libfsaempc.so (include/fsaempc.h).  Host-side glue only: argument checks,
// workspace carving, kernel launches.  There is no CPU compute path: without a gfx950 device every entry
// point fails with FSAEMPC_ERR_NODEVICE / FSAEMPC_ERR_HIP.
// The LTV build and step entries share one host path each (ltv_build_impl, ltv_step_impl) that takes the parameter block, the
// blocking and the corridor as optional descriptors; the entries without a suffix and _aux, _lambda, _p, _b are forwards with NULL
// for what they do not take, plus the one check that is theirs.  The host-buffer QP paths (fsaempc_qp_solve_batch, the
// qpOASES_sequence handles) share the data scans, the checked copies and the layout of the per-call vectors.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <dlfcn.h>
#include <atomic>
#include <mutex>
#include <vector>
#include "fsaempc.h"
#include "qp_solver.h"
#include "ltv_build.h"
#include "reference.h"
#include "plant.h"
#include "cl_latency.h"
#include "cl_estimator.h"
#include "planner.h"
#include "raceline.h"
#include "minlap.h"
#include "corridor.h"
#include "cones.h"
#include "sqp.h"
#include "qp_sens.h"

namespace {
thread_local char g_err[512] = "";
// Diagnostics (fsaempc_debug_set_dump, fsaempc_qp_set_timing): process-wide switches meant for ONE measuring thread (bench.py,
// tools/).  Atomics keep a solve on another thread well-defined while they are flipped; the event triple itself is not
// per-thread, so timing figures are only meaningful when a single thread launches solves.
std::atomic<double*> g_dump{nullptr}; std::atomic<int> g_dump_stage{0};
std::atomic<bool> g_timing{false}; hipEvent_t g_ev[3] = {nullptr, nullptr, nullptr};
hipEvent_t g_evf[2] = {nullptr, nullptr};   // fused step: before the construction kernel, after the post-solve kernel
hipEvent_t g_evs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // SQP sweep: compaction+gather | build | solve | line search
double g_sqp_ms[4] = {0, 0, 0, 0};   // summed over the sweeps of the last SQP call: compaction + gather, build, solve, line search

// roctx ranges around the launches of every phase (rocprofv3 --marker-trace shows them next to the kernel trace).  The roctx library is
// looked up at run time: without it (or with FSAEMPC_ROCTX=0) the ranges are no-ops and the library has no dependency on it.
struct Roctx {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
  Roctx() {
    const char* off = getenv("FSAEMPC_ROCTX");
    if (off && off[0] == '0') return;
    void* h = nullptr;   // rocprofv3 listens to the rocprofiler-sdk flavour; libroctx64 is roctracer's (rocprof v1 / v2)
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
      if ((h = dlopen(name, RTLD_LAZY | RTLD_GLOBAL))) break;
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA"); pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
struct Range {   // RAII: one named range on the calling thread
  static Roctx& api() { static Roctx r; return r; }
  bool on;
  explicit Range(const char* name) : on(api().push != nullptr) { if (on) api().push(name); }
  ~Range() { if (on) api().pop(); }
};

int fail(int code, const char* fmt, const char* a = "") { snprintf(g_err, sizeof(g_err), fmt, a); return code; }
int hipfail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu || e == hipErrorInsufficientDriver)
             ? FSAEMPC_ERR_NODEVICE : FSAEMPC_ERR_HIP;
}
size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }
// the spline half of a kernel parameter struct (the structs spell it with the same four names)
template <class T> void set_spline(T* P, const fsaempc_spline* sp) { P->spM = sp->M; P->spdl = sp->dl; P->xP = sp->xP; P->yP = sp->yP; }
}  // namespace

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
  hipError_t e;
  if (timing) { e = hipEventRecord(g_ev[0], (hipStream_t)stream); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
  { Range r("fsaempc.qp.prep+solve");   // (prep, order and solve kernels are enqueued by one call; the kernel trace separates them)
    e = qp_launch(P, desc->batch, (hipStream_t)stream, timing ? g_ev[1] : nullptr); }
  if (e != hipSuccess) return hipfail(e, "qp_launch");
  if (timing) { e = hipEventRecord(g_ev[2], (hipStream_t)stream); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
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
  hipError_t e;
  { Range r("fsaempc.qp.vjp");
    e = qps_launch(P, (hipStream_t)stream); }
  if (e != hipSuccess) return hipfail(e, "qps_launch");
  return 0;
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
  hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) *rc = hipfail(e, "hipMemcpy H2D");
}
static void to_host(int* rc, void* dst, const void* src, size_t bytes) {
  if (*rc || !dst) return;
  hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) *rc = hipfail(e, "hipMemcpy D2H");
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
  if (rc == 0) { hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) rc = hipfail(e, "solve"); }
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
  hipError_t e = hipMalloc((void**)&dev, (szH + szA + szv) * sizeof(double) + (size_t)wsb + 4096);
  if (e != hipSuccess) return hipfail(e, "hipMalloc");
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
  hipError_t e;
  if (!q->dH) { e = hipMalloc((void**)&q->dH, n * n * sizeof(double)); if (e != hipSuccess) return hipfail(e, "hipMalloc"); }
  if (m && !q->dA) { e = hipMalloc((void**)&q->dA, m * n * sizeof(double)); if (e != hipSuccess) return hipfail(e, "hipMalloc"); }
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
  hipError_t e;
  if (k > q->kcap) {   // grow the per-call buffers (QpVecs) and the workspace
    (void)hipFree(q->dvec); (void)hipFree(q->dws); q->dvec = nullptr; q->dws = nullptr; q->kcap = 0;
    const long long wsb = fsaempc_qp_workspace_bytes(&d);
    if (wsb < 0) return fail((int)wsb, "workspace size");
    e = hipMalloc((void**)&q->dvec, QpVecs::doubles(n, m, B) * sizeof(double)); if (e != hipSuccess) return hipfail(e, "hipMalloc");
    e = hipMalloc(&q->dws, (size_t)wsb); if (e != hipSuccess) return hipfail(e, "hipMalloc");
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

int fsaempc_ltv_nx(int model) { return model == FSAEMPC_MODEL_KINEMATIC ? 5 : 7; }
static int ltv_ns(int model) { return model == FSAEMPC_MODEL_KINEMATIC ? 1 : 4; }
int fsaempc_ltv_nV(int model, int N) { return 2 * N + ltv_ns(model); }
int fsaempc_ltv_nC(int model, int N) { return (model == FSAEMPC_MODEL_KINEMATIC ? 6 : 20) * N; }

static int ltv_check(const fsaempc_ltv_desc* d, const fsaempc_spline* sp) {
  if (!d || !sp || !sp->xP || !sp->yP) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (d->model != FSAEMPC_MODEL_KINEMATIC && d->model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (d->N <= 0 || d->batch < 0 || !(d->dt > 0) || sp->M <= 0 || !(sp->dl > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (d->integrator < FSAEMPC_INT_DEFAULT || d->integrator > FSAEMPC_INT_RK4) return fail(FSAEMPC_ERR_ARG, "unknown integrator");
  if (ltv_build_lds_bytes(fsaempc_ltv_nx(d->model), d->N, 256) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "horizon too long for the LDS staging");
  return 0;
}

static bool pos_finite(double v) { return v > 0 && v < INFINITY; }

static int ltv_integ(const fsaempc_ltv_desc* d) {
  return d->integrator >= 0 ? d->integrator : (d->model == FSAEMPC_MODEL_KINEMATIC ? FSAEMPC_INT_RK2 : FSAEMPC_INT_RK4);   // ltvmpc_*.m:38
}

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
// a NULL block (or NULL values) selects the kernels with the constants compiled in
static const double* par_values(const fsaempc_ltv_params* par) { return par ? par->values : nullptr; }
static int par_stride(const fsaempc_ltv_params* par) { return par && par->per_instance ? FSAEMPC_NPAR : 0; }


/* ---- s-varying track corridors ---- */
// the descriptor as the kernels take it; every refusal names the argument
static int cor_check(const fsaempc_corridor* cor, CorTable* out) {
  if (!cor->n_lo) return fail(FSAEMPC_ERR_ARG, "corridor: n_lo is NULL");
  if (!cor->n_hi) return fail(FSAEMPC_ERR_ARG, "corridor: n_hi is NULL");
  if (cor->N_w < 2) return fail(FSAEMPC_ERR_ARG, "corridor: N_w must be >= 2");
  if (!pos_finite(cor->ds)) return fail(FSAEMPC_ERR_ARG, "corridor: ds must be finite and > 0");
  out->n_lo = cor->n_lo; out->n_hi = cor->n_hi; out->N_w = cor->N_w; out->ds = cor->ds; out->stride = cor->per_instance ? cor->N_w : 0;
  return 0;
}
// the track-row bounds of a built batch (plain or blocked: the rows are the same) from the corridor
static int cor_rows(const fsaempc_ltv_desc* desc, const CorTable& cor, const double* x_lin, const double* pred, double* lbA, double* ubA,
                    void* stream) {
  Range r("fsaempc.ltv.corridor");
  CorRowsParams P; P.nx = fsaempc_ltv_nx(desc->model); P.N = desc->N; P.nC = fsaempc_ltv_nC(desc->model, desc->N); P.batch = desc->batch;
  P.x_lin = x_lin; P.pred = pred; P.lbA = lbA; P.ubA = ubA; P.cor = cor;
  hipError_t e = cor_rows_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cor_rows_launch");
  return 0;
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

/* ---- one build, one carve, one step: every fsaempc_ltv_build_qp_* / _step_* entry below is a forward ---- */
// What the optional descriptors make of a call, worked out once.  Unblocked -- and a trivial blocking (n_blocks == N) is the unblocked
// problem: same kernels, same carve -- the QP has 2N + ns variables and is sized and solved without a slack hint; blocked it has
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
  if (exact && ltv_build_lds_bytes(nx, N, 256, true) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, too_long);
  if (!x0 || !x_ref || (!exact && !x_lin) || !u_lin || !q.H || !q.g || !q.A || !q.lb || !q.ub || !q.lbA || !q.ubA || !q.Bt)
    return fail(FSAEMPC_ERR_ARG, "null argument (Bt is required as scratch)");
  if (s.blocked ? ltv_build_blocked_lds_bytes(nx, N, s.bm.M, 256) > 160 * 1024
                : par_values(par) && ltv_build_lds_bytes(nx, N, 256, exact, true) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, too_long);
  if (desc->batch == 0) return 0;
  LtvParams P = ltv_params(desc, sp, x_lin, u_lin);
  P.x0 = x0; P.x_ref = x_ref;
  P.H = q.H; P.g = q.g; P.A = q.A; P.lb = q.lb; P.ub = q.ub; P.lbA = q.lbA; P.ubA = q.ubA; P.pred = q.pred; P.Bt = q.Bt; P.qconst = q.qconst;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = s.blocked        ? ltv_build_blocked_launch(P, s.bm, par_values(par), par_stride(par), desc->batch, st)
               : par_values(par) ? ltv_build_par_launch(P, par_values(par), par_stride(par), par_idx, desc->batch, st, exact)
                                 : ltv_build_launch(P, desc->batch, st, exact);
  if (e != hipSuccess) return hipfail(e, s.blocked ? "ltv_build_blocked_launch" : "ltv_build_launch");
  return 0;
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

// QP tensors | the solve's point z | the solver's workspace, sized with the slack hint the solve is given
struct LtvCarve { size_t H, g, A, lb, ub, lbA, ubA, pred, Bt, qc, z, qpws, total; };
static void ltv_carve(const fsaempc_ltv_desc* d, int nV_, int slack_hint_, LtvCarve* c) {
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N;
  const size_t nV = nV_, nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  size_t off = 0;
  auto take = [&](size_t cnt) { size_t o = off; off = align64(off + cnt * sizeof(double)); return o; };
  c->H = take(B * nV * nV); c->g = take(B * nV); c->A = take(B * nC * nV); c->lb = take(B * nV); c->ub = take(B * nV);
  c->lbA = take(B * nC); c->ubA = take(B * nC); c->pred = take(B * R); c->Bt = take(B * R * nV); c->qc = take(B); c->z = take(B * nV);
  off = (off + 255) & ~(size_t)255;
  c->qpws = off;
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  long long w = fsaempc_qp_workspace_bytes_s(&q, slack_hint_);
  c->total = off + (w > 0 ? (size_t)w : 0);
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
  LtvCarve c; ltv_carve(desc, nV, hint, &c);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* w = (char*)workspace;
  auto D = [&](size_t off) { return (double*)(w + off); };
  const LtvQp q{D(c.H), D(c.g), D(c.A), D(c.lb), D(c.ub), D(c.lbA), D(c.ubA), D(c.pred), D(c.Bt), D(c.qc)};
  Range whole(s.blocked ? "fsaempc.ltv.step_blocked" : "fsaempc.ltv.step");
  const bool timing = g_timing.load();
  if (timing) { hipError_t e = hipEventRecord(g_evf[0], (hipStream_t)stream); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
  { Range r(s.blocked ? "fsaempc.ltv.build_blocked" : "fsaempc.ltv.build");
    rc = ltv_build_shaped(desc, sp, par, s, x0, x_ref, x_lin, u_lin, q, stream, false, nullptr); }
  if (rc) return rc;
  if (s.corridor) { rc = cor_rows(desc, s.cor, x_lin, q.pred, q.lbA, q.ubA, stream); if (rc) return rc; }
  fsaempc_qp_desc qd{nV, fsaempc_ltv_nC(desc->model, desc->N), desc->batch, 0};
  rc = fsaempc_qp_solve_batch_device_s(&qd, hint, q.H, q.g, q.A, q.lb, q.ub, q.lbA, q.ubA, opts, D(c.z), fval, exitflag, iter,
                                       lambda, aux, w + c.qpws, (long long)(c.total - c.qpws), stream);
  if (rc) return rc;
  hipError_t e;
  { Range r("fsaempc.ltv.post");
    e = s.blocked ? ltv_post_blocked_launch(nx, desc->N, ns, s.bm, desc->batch, D(c.z), q.pred, q.Bt, q.qconst, u_opt, x_opt, slack, fval, (hipStream_t)stream)
                  : ltv_post_launch(nx, desc->N, ns, desc->batch, D(c.z), q.pred, q.Bt, q.qconst, u_opt, x_opt, slack, fval, (hipStream_t)stream); }
  if (e != hipSuccess) return hipfail(e, s.blocked ? "ltv_post_blocked_launch" : "ltv_post_launch");
  if (timing) { e = hipEventRecord(g_evf[1], (hipStream_t)stream); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
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
  LtvCarve c; ltv_carve(desc, fsaempc_ltv_nV(desc->model, desc->N), -1, &c);
  return (long long)c.total;
}
long long fsaempc_ltv_workspace_bytes_b(const fsaempc_ltv_desc* desc, const fsaempc_ltv_blocking* blk) {
  if (!desc || desc->batch < 0) return FSAEMPC_ERR_ARG;
  if (!blk) return fail(FSAEMPC_ERR_ARG, "null argument");
  LtvShape s;
  if (int rc = ltv_shape(desc, blk, nullptr, true, &s)) return rc;
  LtvCarve c; ltv_carve(desc, s.nV(desc), s.slack_hint(desc), &c);
  return (long long)c.total;
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
  hipError_t e = ltv_affine_launch(ltv_params(desc, sp, x_lin, u_lin), desc->batch, Abar, Crow, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "ltv_affine_launch");
  return 0;
}

struct LtvVjpCarve { LtvCarve f; size_t zbar, fb, gbar, lbAbar, ubAbar, Abar, Crow, vjpws, total; };
static void ltv_vjp_carve(const fsaempc_ltv_desc* d, int k, LtvVjpCarve* c) {
  ltv_carve(d, fsaempc_ltv_nV(d->model, d->N), -1, &c->f);
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N, K = k > 0 ? k : 1;
  const size_t nV = fsaempc_ltv_nV(d->model, d->N), nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  size_t off = c->f.qpws;   // the forward's QP tensors stay; the solver's workspace is not needed here
  auto take = [&](size_t cnt) { size_t o = off; off = align64(off + cnt * sizeof(double)); return o; };
  c->zbar = take(B * K * nV); c->fb = take(B * K); c->gbar = take(B * K * nV); c->lbAbar = take(B * K * nC); c->ubAbar = take(B * K * nC);
  c->Abar = take(B * R * nx); c->Crow = take(B * nC * nx);
  off = (off + 255) & ~(size_t)255;
  c->vjpws = off;
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  long long w = fsaempc_qp_vjp_workspace_bytes(&q);
  c->total = off + (w > 0 ? (size_t)w : 0);
}

long long fsaempc_ltv_step_vjp_workspace_bytes(const fsaempc_ltv_desc* desc, int k) {
  if (!desc || desc->N <= 0 || desc->batch < 0 || k < 1) return FSAEMPC_ERR_ARG;
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  LtvVjpCarve c; ltv_vjp_carve(desc, k, &c);
  return (long long)c.total;
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
  LtvVjpCarve c; ltv_vjp_carve(desc, k, &c);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* w = (char*)workspace;
  auto D = [&](size_t off) { return (double*)(w + off); };
  const int nx = fsaempc_ltv_nx(desc->model), N = desc->N, ns = ltv_ns(desc->model);
  const int nV = fsaempc_ltv_nV(desc->model, N), nC = fsaempc_ltv_nC(desc->model, N), B = desc->batch;
  hipStream_t st = (hipStream_t)stream;
  Range whole("fsaempc.ltv.step_vjp");
  // the QP of the step (the build is deterministic: the same QP the forward solved) and the affine maps
  rc = ltv_build_shaped(desc, sp, nullptr, LtvShape(), x0, x_ref, x_lin, u_lin,
                        LtvQp{D(c.f.H), D(c.f.g), D(c.f.A), D(c.f.lb), D(c.f.ub), D(c.f.lbA), D(c.f.ubA), D(c.f.pred), D(c.f.Bt), D(c.f.qc)}, stream, false, nullptr);
  if (rc) return rc;
  rc = fsaempc_ltv_affine_maps_batch_device(desc, sp, x_lin, u_lin, D(c.Abar), D(c.Crow), stream);
  if (rc) return rc;
  hipError_t e = ltv_vjp_pre_launch(nx, N, ns, B, k, D(c.f.Bt), u_opt, slack, io->ubar, io->xbar, io->sbar, D(c.f.z), D(c.zbar), st);
  if (e != hipSuccess) return hipfail(e, "ltv_vjp_pre_launch");
  if (io->fbar) { e = hipMemcpyAsync(D(c.fb), io->fbar, sizeof(double) * (size_t)B * k, hipMemcpyDeviceToDevice, st); if (e != hipSuccess) return hipfail(e, "hipMemcpyAsync"); }
  fsaempc_qp_desc q{nV, nC, B, 0};
  fsaempc_qp_vjp_io qio{D(c.zbar), io->fbar ? D(c.fb) : nullptr, D(c.gbar), nullptr, nullptr, D(c.lbAbar), D(c.ubAbar), nullptr, nullptr};
  rc = fsaempc_qp_vjp_batch_device(&q, k, D(c.f.H), D(c.f.g), D(c.f.A), D(c.f.lb), D(c.f.ub), D(c.f.lbA), D(c.f.ubA), D(c.f.z), lambda,
                                   exitflag, polished, opts, &qio, status, w + c.vjpws, (long long)(c.total - c.vjpws), stream);
  if (rc) return rc;
  e = ltv_vjp_chain_launch(nx, N, B, k, D(c.f.Bt), D(c.f.pred), x_ref, D(c.Abar), D(c.Crow), D(c.gbar), D(c.lbAbar), D(c.ubAbar),
                           io->xbar, io->fbar, status, io->x0bar, io->xrefbar, st);
  if (e != hipSuccess) return hipfail(e, "ltv_vjp_chain_launch");
  return 0;
}

/* ---- batched SQP of the nonlinear MPC step ---- */
void fsaempc_sqp_default_opts(fsaempc_sqp_opts* o) {
  if (!o) return;
  o->max_sweeps = 20; o->trials = 8; o->tol_step = 1e-6; o->tol_feas = 1e-6; o->armijo = 1e-4; o->rho0 = 1.0; o->warm_start = 1;
}

struct SqpCarve { size_t idx, cnt, gx0, gxr, gu, xinit, H, g, A, lb, ub, lbA, ubA, pred, Bt, qc, z, qf, qflag, qit, lam, rho, J, viol, vmax, qpws, total; };
static void sqp_carve(const fsaempc_ltv_desc* d, SqpCarve* c) {
  const size_t B = d->batch > 0 ? d->batch : 1, nx = fsaempc_ltv_nx(d->model), N = d->N;
  const size_t nV = fsaempc_ltv_nV(d->model, d->N), nC = fsaempc_ltv_nC(d->model, d->N), R = nx * N;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align64(off + bytes); return o; };
  const size_t D = sizeof(double), I = sizeof(int);
  c->idx = take(B * I); c->cnt = take(I);
  c->gx0 = take(B * nx * D); c->gxr = take(B * R * D); c->gu = take(B * 2 * N * D); c->xinit = take(B * nV * D);
  c->H = take(B * nV * nV * D); c->g = take(B * nV * D); c->A = take(B * nC * nV * D); c->lb = take(B * nV * D); c->ub = take(B * nV * D);
  c->lbA = take(B * nC * D); c->ubA = take(B * nC * D); c->pred = take(B * R * D); c->Bt = take(B * R * nV * D); c->qc = take(B * D);
  c->z = take(B * nV * D); c->qf = take(B * D); c->qflag = take(B * I); c->qit = take(B * I); c->lam = take(B * (nV + nC) * D);
  c->rho = take(B * D); c->J = take(B * D); c->viol = take(B * D); c->vmax = take(B * D);
  off = (off + 255) & ~(size_t)255;
  c->qpws = off;
  fsaempc_qp_desc q{(int)nV, (int)nC, (int)B, 0};
  long long w = fsaempc_qp_workspace_bytes(&q);
  c->total = off + (w > 0 ? (size_t)w : 0);
}

long long fsaempc_sqp_workspace_bytes(const fsaempc_ltv_desc* desc) {
  if (!desc || desc->N <= 0 || desc->batch < 0) return FSAEMPC_ERR_ARG;
  if (fsaempc_ltv_nV(desc->model, desc->N) > FSAEMPC_MAX_NV) return FSAEMPC_ERR_DIM;
  SqpCarve c; sqp_carve(desc, &c);
  return (long long)c.total;
}

int fsaempc_sqp_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp,
                             const double* x0, const double* x_ref, const double* u_init,
                             const fsaempc_qp_opts* qp_opts, const fsaempc_sqp_opts* sqp_opts,
                             double* u_opt, double* x_opt, double* slack, double* fval, int* status, int* sweeps,
                             const fsaempc_sqp_aux* aux, void* workspace, long long workspace_bytes, void* stream) {
  return fsaempc_sqp_batch_device_p(desc, sp, nullptr, x0, x_ref, u_init, qp_opts, sqp_opts, u_opt, x_opt, slack, fval, status, sweeps, aux,
                                    workspace, workspace_bytes, stream);
}

// (build, initial rollout and line search all read the block: instance i of a compacted sub-batch finds its own through the index list)
int fsaempc_sqp_batch_device_p(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                               const double* x0, const double* x_ref, const double* u_init,
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
  SqpCarve c; sqp_carve(desc, &c);
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* w = (char*)workspace;
  auto D = [&](size_t off) { return (double*)(w + off); };
  auto Iw = [&](size_t off) { return (int*)(w + off); };
  hipStream_t st = (hipStream_t)stream;
  const int nx = fsaempc_ltv_nx(desc->model), N = desc->N, nV = fsaempc_ltv_nV(desc->model, N), nC = fsaempc_ltv_nC(desc->model, N);
  SqpParams P; memset(&P, 0, sizeof(P));
  P.nx = nx; P.N = N; P.integ = ltv_integ(desc); P.B = desc->batch; P.dt = desc->dt; set_spline(&P, sp);
  P.x0 = x0; P.x_ref = x_ref; P.u = u_opt; P.x = x_opt; P.s = slack; P.fval = fval; P.status = status; P.sweeps = sweeps;
  P.rho = D(c.rho); P.J = D(c.J); P.viol = D(c.viol); P.vmax = D(c.vmax);
  if (aux) { P.lambda_out = aux->lambda; P.qp_iter = aux->qp_iter; P.step_norm = aux->step_norm; P.hard_viol = aux->hard_viol; P.merit = aux->merit; }
  P.max_sweeps = o.max_sweeps; P.trials = o.trials; P.tol_step = o.tol_step; P.tol_feas = o.tol_feas; P.armijo = o.armijo; P.rho0 = o.rho0;
  Range whole("fsaempc.sqp");
  const bool timing = g_timing.load();
  for (double& v : g_sqp_ms) v = 0;
  hipError_t e = sqp_init_launch(P, u_init, st, par_values(par), par_stride(par));
  if (e != hipSuccess) return hipfail(e, "sqp_init_launch");
  for (int sweep = 0; sweep < o.max_sweeps; ++sweep) {
    if (timing) { e = hipEventRecord(g_evs[0], st); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
    int cnt = 0;
    { Range r("fsaempc.sqp.compact");
      e = sqp_compact_launch(status, desc->batch, Iw(c.idx), Iw(c.cnt), st);
      if (e == hipSuccess) e = hipMemcpyAsync(&cnt, Iw(c.cnt), sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st); }   // the one read of the sweep
    if (e != hipSuccess) return hipfail(e, "sqp compaction");
    if (cnt == 0) break;
    double* xinit = o.warm_start ? D(c.xinit) : nullptr;
    e = sqp_gather_launch(P, Iw(c.idx), cnt, D(c.gx0), D(c.gxr), D(c.gu), xinit, nV, st);
    if (e != hipSuccess) return hipfail(e, "sqp_gather_launch");
    if (timing) { e = hipEventRecord(g_evs[1], st); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
    fsaempc_ltv_desc sub = *desc; sub.batch = cnt;
    { Range r("fsaempc.sqp.build");
      rc = ltv_build_shaped(&sub, sp, par, LtvShape(), D(c.gx0), D(c.gxr), nullptr, D(c.gu),
                            LtvQp{D(c.H), D(c.g), D(c.A), D(c.lb), D(c.ub), D(c.lbA), D(c.ubA), D(c.pred), D(c.Bt), D(c.qc)}, stream, true, Iw(c.idx)); }
    if (rc) return rc;
    if (timing) { e = hipEventRecord(g_evs[2], st); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
    fsaempc_qp_desc q{nV, nC, cnt, 0};
    fsaempc_qp_aux qa{nullptr, nullptr, xinit, nullptr};
    rc = fsaempc_qp_solve_batch_device_aux(&q, D(c.H), D(c.g), D(c.A), D(c.lb), D(c.ub), D(c.lbA), D(c.ubA), qp_opts, D(c.z), D(c.qf),
                                           Iw(c.qflag), Iw(c.qit), D(c.lam), &qa, w + c.qpws, (long long)(c.total - c.qpws), stream);
    if (rc) return rc;
    if (timing) { e = hipEventRecord(g_evs[3], st); if (e != hipSuccess) return hipfail(e, "hipEventRecord"); }
    { Range r("fsaempc.sqp.linesearch");
      e = sqp_linesearch_launch(P, Iw(c.idx), cnt, sweep, D(c.z), D(c.qf), D(c.qc), Iw(c.qflag), Iw(c.qit), D(c.lam), st,
                                par_values(par), par_stride(par)); }
    if (e != hipSuccess) return hipfail(e, "sqp_linesearch_launch");
    if (timing) {
      e = hipEventRecord(g_evs[4], st); if (e == hipSuccess) e = hipEventSynchronize(g_evs[4]);
      if (e != hipSuccess) return hipfail(e, "hipEventRecord");
      for (int k = 0; k < 4; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, g_evs[k], g_evs[k + 1]) == hipSuccess) g_sqp_ms[k] += ms; }
    }
  }
  return 0;
}

int fsaempc_sqp_get_timing(double* build_ms, double* solve_ms, double* linesearch_ms, double* compact_ms) {
  if (!build_ms || !solve_ms || !linesearch_ms || !compact_ms) return fail(FSAEMPC_ERR_ARG, "null argument");
  *compact_ms = g_sqp_ms[0]; *build_ms = g_sqp_ms[1]; *solve_ms = g_sqp_ms[2]; *linesearch_ms = g_sqp_ms[3];
  return 0;
}

int fsaempc_obtain_reference_batch_device(const double* plan, double ds, int N_s, const double* t, const double* s0, double dt,
                                          int N_t, int batch, double* x_ref, void* stream) {
  if (!plan || !t || !s0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (N_s <= 0 || N_t <= 0 || batch < 0 || !(ds > 0) || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  RefParams P; P.plan = plan; P.t = t; P.s0 = s0; P.x_ref = x_ref; P.ds = ds; P.dt = dt; P.N_s = N_s; P.N_t = N_t; P.batch = batch;
  hipError_t e = obtain_reference_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "obtain_reference_launch");
  return 0;
}

int fsaempc_reference_live_batch_device(int nx, int N, double dt, double target_vel, int batch, const double* x0, double* x_ref, void* stream) {
  if (!x0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if ((nx != 5 && nx != 7) || N <= 0 || batch < 0 || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  hipError_t e = reference_live_launch(nx, N, dt, target_vel, batch, x0, x_ref, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "reference_live_launch");
  return 0;
}

int fsaempc_cl_pre_batch_device(int model, int N, double dt, double target_vel, double L, const fsaempc_spline* sp, const double* cart,
                                const double* s_guess, int batch, double* x0, double* x_ref, int* finished, void* stream) {
  if (!sp || !sp->xP || !sp->yP || !cart || !s_guess || !x0 || !x_ref || !finished) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !(dt > 0) || sp->M <= 0 || !(sp->dl > 0) || !(L > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  ClPreParams P; P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.target_vel = target_vel; P.L = L;
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP; P.cart = cart; P.s_guess = s_guess; P.x0 = x0; P.x_ref = x_ref; P.finished = finished;
  hipError_t e = cl_pre_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cl_pre_launch");
  return 0;
}

int fsaempc_cl_plant_batch_device(int model, int N, double dt, int batch, double* cart, double* pid, const double* x_opt,
                                  const int* finished, const int* exitflag, double* u_last, void* stream) {
  return fsaempc_cl_plant_batch_device_p(model, N, dt, batch, nullptr, cart, pid, x_opt, finished, exitflag, u_last, stream);
}

int fsaempc_cl_plant_batch_device_p(int model, int N, double dt, int batch, const fsaempc_ltv_params* par, double* cart, double* pid,
                                    const double* x_opt, const int* finished, const int* exitflag, double* u_last, void* stream) {
  if (!cart || !pid || !x_opt) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !(dt > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  ClPlantParams P; P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.cart = cart; P.pid = pid; P.x_opt = x_opt;
  P.finished = finished; P.exitflag = exitflag; P.u_last = u_last;
  hipError_t e = cl_plant_launch(P, (hipStream_t)stream, par_values(par), par_stride(par));
  if (e != hipSuccess) return hipfail(e, "cl_plant_launch");
  return 0;
}

int fsaempc_cl_accept_batch_device(int model, int N, int batch, const double* x_new, const double* u_new, const int* exitflag, double* x_keep, double* u_keep, void* stream) {
  if (!x_new || !u_new || !x_keep || !u_keep) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  hipError_t e = cl_accept_launch(fsaempc_ltv_nx(model) * N, 2 * N, batch, x_new, u_new, exitflag, x_keep, u_keep, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cl_accept_launch");
  return 0;
}

/* ---- lap report ---- */
static int cl_metrics(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par, const fsaempc_corridor* cor,
                      const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                      const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  CorTable ct;
  if (cor) { if (int rc = cor_check(cor, &ct)) return rc; }
  if (!x0 || !finished || !exitflag || !iter || !fval || !slack || !u_drive || !cart || !metrics) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!(slack_tol >= 0)) return fail(FSAEMPC_ERR_ARG, "slack_tol must be >= 0");
  if (batch == 0) return 0;
  ClMetricsParams P; P.ns = ltv_ns(model); P.N = N; P.batch = batch; P.tyre = model == FSAEMPC_MODEL_DYNAMIC ? 3 : 0;
  P.dt = dt; P.slack_tol = slack_tol; P.nx = fsaempc_ltv_nx(model); P.x0 = x0; P.finished = finished; P.exitflag = exitflag; P.iter = iter;
  P.fval = fval; P.slack = slack; P.u_drive = u_drive; P.cart = cart; P.metrics = metrics;
  hipError_t e = cor ? cor_metrics_launch(P, ct, (hipStream_t)stream, par_values(par), par_stride(par))
                     : cl_metrics_launch(P, (hipStream_t)stream, par_values(par), par_stride(par));
  if (e != hipSuccess) return hipfail(e, cor ? "cor_metrics_launch" : "cl_metrics_launch");
  return 0;
}
int fsaempc_cl_metrics_batch_device(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                    const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                    const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  return cl_metrics(model, N, dt, slack_tol, batch, par, nullptr, x0, finished, exitflag, iter, fval, slack, u_drive, cart, metrics, stream);
}
int fsaempc_cl_metrics_batch_device_c(int model, int N, double dt, double slack_tol, int batch, const fsaempc_ltv_params* par,
                                      const fsaempc_corridor* cor,
                                      const double* x0, const int* finished, const int* exitflag, const int* iter, const double* fval,
                                      const double* slack, const double* u_drive, const double* cart, double* metrics, void* stream) {
  return cl_metrics(model, N, dt, slack_tol, batch, par, cor, x0, finished, exitflag, iter, fval, slack, u_drive, cart, metrics, stream);
}

// Host.  Every sum runs over the cars in index order.  Means over an empty set are NaN (MATLAB's mean([])).
int fsaempc_cl_report(const double* metrics_host, int batch, double dt, double* out) {
  if (!out || (!metrics_host && batch != 0)) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  double cars[3] = {0, 0, 0}, lap_sum = 0, lap_min = NAN, lap_max = NAN, steps = 0, abn = 0, sl_n = 0, sl_t = 0, obj = 0, obj_cnt = 0;
  double recorded = 0, nv_sum = 0, nv_big = 0, nv_max = 0, el_sum = 0, el_big = 0, el_max = 0, it_sum = 0, it_max = 0, n_abs = 0;
  for (int b = 0; b < batch; ++b) {
    const double* m = metrics_host + (size_t)b * FSAEMPC_NMETRIC;
    const int st = m[FSAEMPC_M_STATUS] == 1.0 ? 1 : (m[FSAEMPC_M_STATUS] == 2.0 ? 2 : 0);
    cars[st] += 1;
    if (st == 1) {
      const double lap = m[FSAEMPC_M_STEPS] * dt;
      lap_sum += lap;
      if (!(lap_min <= lap)) lap_min = lap;
      if (!(lap_max >= lap)) lap_max = lap;
    }
    steps += m[FSAEMPC_M_STEPS]; abn += m[FSAEMPC_M_ABNORMAL]; sl_n += m[FSAEMPC_M_SLACK_N_CNT]; sl_t += m[FSAEMPC_M_SLACK_TYRE_CNT];
    obj += m[FSAEMPC_M_OBJ_SUM]; obj_cnt += m[FSAEMPC_M_OBJ_CNT]; it_sum += m[FSAEMPC_M_ITER_SUM];
    if (m[FSAEMPC_M_STEPS] > 0) { recorded += 1; nv_sum += m[FSAEMPC_M_N_VIOL_INT]; el_sum += m[FSAEMPC_M_ELL_VIOL_INT]; }
    if (m[FSAEMPC_M_N_VIOL_INT] > nv_big) nv_big = m[FSAEMPC_M_N_VIOL_INT];
    if (m[FSAEMPC_M_N_VIOL_MAX] > nv_max) nv_max = m[FSAEMPC_M_N_VIOL_MAX];
    if (m[FSAEMPC_M_ELL_VIOL_INT] > el_big) el_big = m[FSAEMPC_M_ELL_VIOL_INT];
    if (m[FSAEMPC_M_ELL_VIOL_MAX] > el_max) el_max = m[FSAEMPC_M_ELL_VIOL_MAX];
    if (m[FSAEMPC_M_ITER_MAX] > it_max) it_max = m[FSAEMPC_M_ITER_MAX];
    if (m[FSAEMPC_M_N_ABS_MAX] > n_abs) n_abs = m[FSAEMPC_M_N_ABS_MAX];
  }
  out[FSAEMPC_R_CARS_DRIVING] = cars[0]; out[FSAEMPC_R_CARS_FINISHED] = cars[1]; out[FSAEMPC_R_CARS_LOST] = cars[2];
  out[FSAEMPC_R_LAP_MEAN] = cars[1] > 0 ? lap_sum / cars[1] : NAN; out[FSAEMPC_R_LAP_MIN] = lap_min; out[FSAEMPC_R_LAP_MAX] = lap_max;
  out[FSAEMPC_R_STEPS] = steps;
  out[FSAEMPC_R_ABNORMAL_PCT] = steps > 0 ? abn / steps * 100 : NAN;
  out[FSAEMPC_R_SLACK_N_PCT] = steps > 0 ? sl_n / steps * 100 : NAN;
  out[FSAEMPC_R_SLACK_TYRE_PCT] = steps > 0 ? sl_t / steps * 100 : NAN;
  out[FSAEMPC_R_OBJ_MEAN] = obj_cnt > 0 ? obj / obj_cnt : NAN;
  out[FSAEMPC_R_N_VIOL_INT_MEAN] = recorded > 0 ? nv_sum / recorded : NAN; out[FSAEMPC_R_N_VIOL_INT_MAX] = nv_big; out[FSAEMPC_R_N_VIOL_MAX] = nv_max;
  out[FSAEMPC_R_ELL_VIOL_INT_MEAN] = recorded > 0 ? el_sum / recorded : NAN; out[FSAEMPC_R_ELL_VIOL_INT_MAX] = el_big; out[FSAEMPC_R_ELL_VIOL_MAX] = el_max;
  out[FSAEMPC_R_ITER_MEAN] = steps > 0 ? it_sum / steps : NAN; out[FSAEMPC_R_ITER_MAX] = it_max; out[FSAEMPC_R_N_ABS_MAX] = n_abs;
  return 0;
}

/* ---- multi-lap closed loop: the lap gate ---- */
int fsaempc_cl_lap_gate_batch_device(int nx, int N, double dt, double L, int laps, int batch, double* x0, double* x_ref, double* x_keep,
                                     int* finished, double* lap_state, double* lap_times, double* metrics, double* lap_records, void* stream) {
  if (laps < 1 || laps > FSAEMPC_MAX_LAPS) return fail(FSAEMPC_ERR_ARG, "laps must be 1 .. FSAEMPC_MAX_LAPS");
  if (nx != 5 && nx != 7) return fail(FSAEMPC_ERR_ARG, "nx must be 5 or 7");
  if (N < 1 || batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!pos_finite(dt) || !pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "dt and L must be finite and > 0");
  if (!x0 || !x_ref || !x_keep || !finished || !lap_state || !lap_times) return fail(FSAEMPC_ERR_ARG, "null argument");
  if ((metrics == nullptr) != (lap_records == nullptr)) return fail(FSAEMPC_ERR_ARG, "metrics and lap_records are given together or not at all");
  if (batch == 0) return 0;
  ClLapGateParams P; P.nx = nx; P.N = N; P.laps = laps; P.batch = batch; P.dt = dt; P.L = L; P.x0 = x0; P.x_ref = x_ref; P.x_keep = x_keep;
  P.finished = finished; P.lap_state = lap_state; P.lap_times = lap_times; P.metrics = metrics; P.lap_records = lap_records;
  hipError_t e = cl_lap_gate_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cl_lap_gate_launch");
  return 0;
}

// Host.  Every sum runs over the cars in index order; a lap nobody completed has NaN mean, min and max.
int fsaempc_cl_lap_summary(const double* lap_times_host, int batch, int laps, double* out) {
  if (!out || (!lap_times_host && batch != 0)) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (laps < 1 || laps > FSAEMPC_MAX_LAPS) return fail(FSAEMPC_ERR_ARG, "laps must be 1 .. FSAEMPC_MAX_LAPS");
  for (int l = 0; l < laps; ++l) {
    double cnt = 0, sum = 0, lo = NAN, hi = NAN;
    for (int b = 0; b < batch; ++b) {
      const double t = lap_times_host[(size_t)b * laps + l];
      if (t != t) continue;
      cnt += 1; sum += t;
      if (!(lo <= t)) lo = t;
      if (!(hi >= t)) hi = t;
    }
    out[4 * l] = cnt; out[4 * l + 1] = cnt > 0 ? sum / cnt : NAN; out[4 * l + 2] = lo; out[4 * l + 3] = hi;
  }
  return 0;
}

/* ---- closed loop: measurement noise, plan latency and delay compensation ---- */
static int cl_draw_check(long long id0, long long step) {
  if (id0 < 0) return fail(FSAEMPC_ERR_ARG, "id0 must be >= 0");
  if (step < 0 || step >= (1LL << 32)) return fail(FSAEMPC_ERR_ARG, "step must be 0 .. 2^32 - 1");
  return 0;
}

int fsaempc_cl_noise_batch_device(int nx, int batch, unsigned long long seed, long long id0, long long step, double* z, void* stream) {
  if (nx != 5 && nx != 7) return fail(FSAEMPC_ERR_ARG, "nx must be 5 or 7");
  if (batch < 0) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (int rc = cl_draw_check(id0, step)) return rc;
  if (!z) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (batch == 0) return 0;
  hipError_t e = cl_noise_launch(nx, batch, seed, (unsigned long long)id0, (unsigned long long)step, z, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cl_noise_launch");
  return 0;
}

int fsaempc_cl_observe_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                    const fsaempc_cl_latency* lat, long long step, const double* x0_true, const int* finished,
                                    const double* u_hist, double* x0_obs, double* x0_mpc, void* stream) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!lat) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (lat->delay < 0 || lat->delay > FSAEMPC_CL_MAX_DELAY) return fail(FSAEMPC_ERR_ARG, "delay must be 0 .. FSAEMPC_CL_MAX_DELAY");
  if (lat->compensate != 0 && lat->compensate != 1) return fail(FSAEMPC_ERR_ARG, "compensate must be 0 or 1");
  if (int rc = cl_draw_check(lat->id0, step)) return rc;
  if (lat->delay > 0 && !u_hist) return fail(FSAEMPC_ERR_ARG, "null argument (u_hist is required with delay > 0)");
  if (!x0_true || !x0_obs || !x0_mpc) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (desc->batch == 0) return 0;
  ClObserveParams P;
  P.nx = fsaempc_ltv_nx(desc->model); P.N = desc->N; P.batch = desc->batch; P.integ = ltv_integ(desc);
  P.delay = lat->delay; P.compensate = lat->compensate; P.sigma_per_instance = lat->sigma_per_instance ? 1 : 0; P.dt = desc->dt;
  P.seed = lat->seed; P.id0 = (unsigned long long)lat->id0; P.step = (unsigned long long)step;
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP;
  P.sigma = lat->sigma; P.x0_true = x0_true; P.finished = finished; P.u_hist = u_hist; P.x0_obs = x0_obs; P.x0_mpc = x0_mpc;
  hipError_t e = cl_observe_launch(P, (hipStream_t)stream, par_values(par), par_stride(par));
  if (e != hipSuccess) return hipfail(e, "cl_observe_launch");
  return 0;
}

// Host.
int fsaempc_cl_history_slot(int delay, long long step, int lag) {
  if (delay < 0 || delay > FSAEMPC_CL_MAX_DELAY || step < 0 || lag < 0 || lag > delay) return -1;
  return cll_slot(delay, step, lag);
}

/* ---- closed loop: the state estimator ---- */
namespace { struct ByteRange { const char* name; const void* p; size_t bytes; }; }
static bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
  if (!a.p || !b.p || a.bytes == 0 || b.bytes == 0) return false;
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

int fsaempc_cl_estimate_batch_device(const fsaempc_ltv_desc* desc, const fsaempc_spline* sp, const fsaempc_ltv_params* par,
                                     const fsaempc_cl_estimator* est, const double* z, const double* x_start, const double* u_prev,
                                     long long u_stride, const int* finished, double* est_x, double* est_P, int* est_count, double* x0_est,
                                     double* innov, double* nis, double* F_out, double* x_prior, void* stream) {
  if (int rc = ltv_check(desc, sp)) return rc;
  if (!est || !est->q || !est->r || !est->p0) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (!(est->L >= 0 && est->L < INFINITY)) return fail(FSAEMPC_ERR_ARG, "L must be finite and >= 0");
  if (u_stride < 2) return fail(FSAEMPC_ERR_ARG, "u_stride must be >= 2");
  if (!z || !x_start || !u_prev || !est_x || !est_P || !est_count || !x0_est || !innov || !nis) return fail(FSAEMPC_ERR_ARG, "null argument");
  const size_t B = (size_t)desc->batch, nx = (size_t)fsaempc_ltv_nx(desc->model), d = sizeof(double);
  const ByteRange out[] = {{"est_x", est_x, B * nx * d}, {"est_P", est_P, B * nx * nx * d}, {"est_count", est_count, B * 2 * sizeof(int)},
                           {"x0_est", x0_est, B * nx * d}, {"innov", innov, B * nx * d}, {"nis", nis, B * d},
                           {"F_out", F_out, B * nx * nx * d}, {"x_prior", x_prior, B * nx * d}};
  const ByteRange in[] = {{"z", z, B * nx * d}, {"x_start", x_start, B * nx * d},
                          {"u_prev", u_prev, B ? ((B - 1) * (size_t)u_stride + 2) * d : 0}, {"finished", finished, B * sizeof(int)},
                          {"q", est->q, (est->q_per_instance ? B : 1) * nx * d}, {"r", est->r, (est->r_per_instance ? B : 1) * nx * d},
                          {"p0", est->p0, nx * d}};
  const int n_out = (int)(sizeof(out) / sizeof(out[0])), n_in = (int)(sizeof(in) / sizeof(in[0]));
  for (int i = 0; i < n_out; ++i) {
    for (int k = i + 1; k < n_out; ++k)
      if (ranges_overlap(out[i], out[k])) return fail(FSAEMPC_ERR_ARG, "overlapping outputs");
    for (int k = 0; k < n_in; ++k)
      if (ranges_overlap(out[i], in[k])) return fail(FSAEMPC_ERR_ARG, "an output overlaps an input");
  }
  if (desc->batch == 0) return 0;
  ClEstimateParams P;
  P.nx = (int)nx; P.batch = desc->batch; P.integ = ltv_integ(desc); P.q_per_instance = est->q_per_instance ? 1 : 0;
  P.r_per_instance = est->r_per_instance ? 1 : 0; P.dt = desc->dt; P.L = est->L;
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP;
  P.q = est->q; P.r = est->r; P.p0 = est->p0; P.z = z; P.x_start = x_start; P.u_prev = u_prev; P.u_stride = u_stride; P.finished = finished;
  P.est_x = est_x; P.est_P = est_P; P.est_count = est_count; P.x0_est = x0_est; P.innov = innov; P.nis = nis; P.F_out = F_out; P.x_prior = x_prior;
  hipError_t e = cl_estimate_launch(P, (hipStream_t)stream, par_values(par), par_stride(par));
  if (e != hipSuccess) return hipfail(e, "cl_estimate_launch");
  return 0;
}

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
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP; P.table = table; P.t = t;
  hipError_t e = plan_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "plan_profile_launch");
  return 0;
}

int fsaempc_plan_reference_batch_device(int model, const fsaempc_plan* plan, const double* s0, double dt, int N, int batch, double* x_ref,
                                        void* stream) {
  PlanRefParams P;
  if (int rc = plan_check(plan, &P.plan)) return rc;
  if (!s0 || !x_ref) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (model != FSAEMPC_MODEL_KINEMATIC && model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (N <= 0 || batch < 0 || !pos_finite(dt)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  P.nx = fsaempc_ltv_nx(model); P.N = N; P.batch = batch; P.dt = dt; P.s0 = s0; P.x_ref = x_ref;
  hipError_t e = plan_reference_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "plan_reference_launch");
  return 0;
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
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP; P.cart = cart; P.s_guess = s_guess; P.x0 = x0; P.x_ref = x_ref; P.finished = finished;
  hipError_t e = cl_pre_plan_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cl_pre_plan_launch");
  return 0;
}

/* ---- minimum-curvature racing line ---- */
static int line_check(const fsaempc_spline* sp, double L, int N_s, int N_c) {
  if (!sp || !sp->xP || !sp->yP) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (sp->M <= 0 || !(sp->dl > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (!pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "L must be finite and > 0");
  if (N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_ARG, "N_c must be FSAEMPC_LINE_MIN_NC .. FSAEMPC_MAX_NV");
  if (N_s < 2 * N_c || N_s > FSAEMPC_LINE_MAX_NS) return fail(FSAEMPC_ERR_ARG, "N_s must be 2 N_c .. FSAEMPC_LINE_MAX_NS");
  return 0;
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
  RacelineQpParams Q; Q.N_s = N_s; Q.N_c = N_c; Q.ds = L / N_s; Q.spM = sp->M; Q.spdl = sp->dl; Q.xP = sp->xP; Q.yP = sp->yP; Q.H = H; Q.g = g;
  return Q;
}
static PlanLineParams line_profile_params(int model, const fsaempc_spline* sp, double L, int n_plans, int N_s, int N_c, double v_cap, double grip,
                                          double* table, double* t) {
  PlanLineParams P; memset(&P, 0, sizeof(P));
  P.dynamic = model == FSAEMPC_MODEL_DYNAMIC; P.n_plans = n_plans; P.N_s = N_s; P.N_c = N_c; P.ds = L / N_s; P.h = L / N_c; P.v_cap = v_cap; P.grip = grip;
  P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP; P.table = table; P.t = t;
  return P;
}

int fsaempc_raceline_build_qp_device(const fsaempc_spline* sp, double L, int N_s, int N_c, double* H, double* g, void* stream) {
  if (!H || !g) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  hipError_t e = raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, H, g), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "raceline_qp_launch");
  return 0;
}

int fsaempc_plan_line_profile_batch_device(int model, const fsaempc_spline* sp, double L, const fsaempc_ltv_params* par, int n_plans, int N_s,
                                           int N_c, const double* line, int line_per_plan, double v_cap, double grip, double* table, double* t,
                                           void* stream) {
  if (!line || !table || !t) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_check(sp, L, N_s, N_c)) return rc;
  if (int rc = line_profile_check(model, par, n_plans, v_cap, grip)) return rc;
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = line_per_plan ? N_c : 0;
  hipError_t e = plan_line_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "plan_line_profile_launch");
  return 0;
}

// workspace of fsaempc_plan_raceline_batch_device: H | g, lb, ub (n_plans x N_c each) | fval | iter | the solver's own
struct LineCarve { size_t H, g, lb, ub, fval, iter, qp, total; long long qp_bytes; };
static int line_carve(int n_plans, int N_c, LineCarve* c) {
  if (n_plans < 1 || N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV) return FSAEMPC_ERR_ARG;
  const fsaempc_qp_desc d = {N_c, 0, n_plans, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, 0);
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = align64((size_t)n_plans * N_c * sizeof(double));
  size_t off = 0;
  c->H = off; off += align64((size_t)N_c * N_c * sizeof(double));
  c->g = off; off += vec;
  c->lb = off; off += vec;
  c->ub = off; off += vec;
  c->fval = off; off += align64((size_t)n_plans * sizeof(double));
  c->iter = off; off += align64((size_t)n_plans * sizeof(int));
  c->qp = off; off += (size_t)c->qp_bytes;
  c->total = off;
  return 0;
}
long long fsaempc_plan_raceline_workspace_bytes(int n_plans, int N_c) {
  LineCarve c;
  if (int rc = line_carve(n_plans, N_c, &c)) return rc;
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
  if (!(margin >= 0 && margin < INFINITY)) return fail(FSAEMPC_ERR_ARG, "margin must be finite and >= 0");
  LineCarve c;
  if (int rc = line_carve(n_plans, N_c, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  double *H = (double*)(ws + c.H), *g = (double*)(ws + c.g), *lb = (double*)(ws + c.lb), *ub = (double*)(ws + c.ub);
  hipError_t e = raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, H, g), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "raceline_qp_launch");
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = g; CL.lb = lb; CL.ub = ub; CL.line = line; CL.flag = flag;
  if (cor) {
    e = cor_line_bounds_launch(CL, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "cor_line_bounds_launch");
  } else if (boxed) {
    MinlapBoxParams B; B.n_plans = n_plans; B.N_c = N_c; B.lo = start->lo; B.hi = start->hi; B.g = g; B.lb = lb; B.ub = ub;
    e = minlap_box_launch(B, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "minlap_box_launch");
  } else {
    RacelineBoundsParams B; B.n_plans = n_plans; B.N_c = N_c; B.margin = margin; B.g = g; B.lb = lb; B.ub = ub;
    e = raceline_bounds_launch(B, par_values(par), par_stride(par), (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "raceline_bounds_launch");
  }
  if (given) {   // the caller's control points: no solve, every flag 0
    e = hipMemcpyAsync(line, start->c_init, sizeof(double) * (size_t)n_plans * N_c, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(int) * (size_t)n_plans, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "copy of c_init");
  } else {
    const fsaempc_qp_desc d = {N_c, 0, n_plans, 1};
    if (int rc = fsaempc_qp_solve_batch_device_s(&d, 0, H, g, nullptr, lb, ub, nullptr, nullptr, opts, line, (double*)(ws + c.fval), flag,
                                                 (int*)(ws + c.iter), nullptr, nullptr, ws + c.qp, c.qp_bytes, stream)) return rc;
    if (cor || boxed) {   // a plan whose QP was not solved (no box: flag -1, or any other flag but 0): NaN control points, which the profile turns into a NaN plan
      e = cor_line_void_launch(CL, (hipStream_t)stream);
      if (e != hipSuccess) return hipfail(e, "cor_line_void_launch");
    }
  }
  const bool fallback = !cor && !boxed && !given;   // (in a corridor or a box: no centre-line fallback)
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = N_c; P.flag = fallback ? flag : nullptr; P.line_out = line; P.check_width = (cor || boxed) ? 0 : 1; P.margin = margin;
  e = plan_line_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "plan_line_profile_launch");
  return 0;
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
  if (!pos_finite(L)) return fail(FSAEMPC_ERR_ARG, "L must be finite and > 0");
  if (N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV) return fail(FSAEMPC_ERR_ARG, "N_c must be FSAEMPC_LINE_MIN_NC .. FSAEMPC_MAX_NV");
  if (N_s < 2 * N_c || N_s > FSAEMPC_LINE_MAX_NS) return fail(FSAEMPC_ERR_ARG, "N_s must be 2 N_c .. FSAEMPC_LINE_MAX_NS");
  if (n_plans < 1) return fail(FSAEMPC_ERR_ARG, "n_plans must be >= 1");
  if (!(margin >= 0 && margin < INFINITY)) return fail(FSAEMPC_ERR_ARG, "margin must be finite and >= 0");
  return 0;
}

int fsaempc_corridor_line_bounds_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                        double* lb, double* ub, void* stream) {
  CorLineParams CL;
  if (!cor) return fail(FSAEMPC_ERR_ARG, "null argument (corridor)");
  if (int rc = cor_check(cor, &CL.cor)) return rc;
  if (!lb || !ub) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_rows_check(L, n_plans, N_s, N_c, margin)) return rc;
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = nullptr; CL.lb = lb; CL.ub = ub; CL.line = nullptr; CL.flag = nullptr;
  hipError_t e = cor_line_bounds_launch(CL, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cor_line_bounds_launch");
  return 0;
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
  P.v_cap = v_cap; P.grip = grip; P.spM = sp->M; P.spdl = sp->dl; P.xP = sp->xP; P.yP = sp->yP; P.T_stride = 1;
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
  hipError_t e = minlap_lapgrad_launch(P, par_values(par), par_stride(par), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "minlap_lapgrad_launch");
  return 0;
}

// workspace of fsaempc_plan_minlap_batch_device: that of fsaempc_plan_raceline_batch_device for n_plans (H, the boxes and the initial
// solve) | grad (n_plans x N_c) | per candidate (n_plans J): g, lb, ub, x (N_c each), T, fval, iter, flag | gradc (n_plans J x N_c) |
// the solver's own for n_plans J instances
struct MinlapCarve { LineCarve line; size_t grad, g, lb, ub, x, T, fval, iter, flag, gradc, qp, total; long long qp_bytes; };
static int minlap_carve(int n_plans, int N_c, int J, MinlapCarve* c) {
  if (J < 1 || J > FSAEMPC_MINLAP_MAX_RHO) return FSAEMPC_ERR_ARG;
  if (int rc = line_carve(n_plans, N_c, &c->line)) return rc;
  if ((long long)n_plans * J > 0x7fffffffLL) return FSAEMPC_ERR_ARG;
  const int nJ = n_plans * J;
  const fsaempc_qp_desc d = {N_c, 0, nJ, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, 0);
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = align64((size_t)nJ * N_c * sizeof(double)), one = align64((size_t)nJ * sizeof(double));
  size_t off = align64(c->line.total);
  c->grad = off; off += align64((size_t)n_plans * N_c * sizeof(double));
  c->g = off; off += vec;
  c->lb = off; off += vec;
  c->ub = off; off += vec;
  c->x = off; off += vec;
  c->T = off; off += one;
  c->fval = off; off += one;
  c->iter = off; off += one;
  c->flag = off; off += one;
  c->gradc = off; off += vec;
  c->qp = off; off += (size_t)c->qp_bytes;
  c->total = off;
  return 0;
}
long long fsaempc_plan_minlap_workspace_bytes(int n_plans, int N_c, int n_rho) {
  MinlapCarve c;
  if (int rc = minlap_carve(n_plans, N_c, n_rho, &c)) return rc;
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
  if (!(margin >= 0 && margin < INFINITY)) return fail(FSAEMPC_ERR_ARG, "margin must be finite and >= 0");
  if (iters < 0) return fail(FSAEMPC_ERR_ARG, "iters must be >= 0");
  if (iters > 0 && !step_hist) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (n_rho < 1 || n_rho > FSAEMPC_MINLAP_MAX_RHO) return fail(FSAEMPC_ERR_ARG, "n_rho must be 1 .. FSAEMPC_MINLAP_MAX_RHO");
  for (int j = 0; j < n_rho; ++j)
    if (!pos_finite(rho[j])) return fail(FSAEMPC_ERR_ARG, "every rho must be finite and > 0");
  if ((lo != nullptr) != (hi != nullptr)) return fail(FSAEMPC_ERR_ARG, "lo and hi come together");
  MinlapCarve c;
  if (int rc = minlap_carve(n_plans, N_c, n_rho, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  // the start: fsaempc_plan_raceline_batch_device itself (with K = 0 and neither boxes nor c_init this call is that entry)
  const LineStart start = {lo, hi, c_init};
  if (int rc = plan_raceline(model, sp, L, par, nullptr, n_plans, N_s, N_c, margin, v_cap, grip, opts, line, flag, table, t, ws,
                             (long long)c.line.total, stream, (lo || c_init) ? &start : nullptr)) return rc;
  const double *H = (const double*)(ws + c.line.H), *blo = (const double*)(ws + c.line.lb), *bhi = (const double*)(ws + c.line.ub);
  double *grad = (double*)(ws + c.grad), *xc = (double*)(ws + c.x), *Tc = (double*)(ws + c.T), *gradc = (double*)(ws + c.gradc);
  int* flagc = (int*)(ws + c.flag);
  const int nJ = n_plans * n_rho, check_width = lo ? 0 : 1;
  MinlapGradParams G = minlap_grad_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip);
  G.check_width = check_width; G.margin = margin; G.line = line; G.line_stride = N_c; G.T = lap_hist; G.T_stride = iters + 1; G.grad = grad;
  hipError_t e = minlap_lapgrad_launch(G, par_values(par), par_stride(par), st);
  if (e != hipSuccess) return hipfail(e, "minlap_lapgrad_launch");
  for (int it = 0; it < iters; ++it) {
    MinlapCandParams Q; memset(&Q, 0, sizeof(Q));
    Q.n_plans = n_plans; Q.J = n_rho; Q.N_c = N_c; Q.grad = grad; Q.c = line; Q.lo = blo; Q.hi = bhi;
    for (int j = 0; j < n_rho; ++j) Q.rho[j] = rho[j];
    Q.g = (double*)(ws + c.g); Q.lb = (double*)(ws + c.lb); Q.ub = (double*)(ws + c.ub);
    e = minlap_candidates_launch(Q, st);
    if (e != hipSuccess) return hipfail(e, "minlap_candidates_launch");
    const fsaempc_qp_desc d = {N_c, 0, nJ, 1};
    if (int rc = fsaempc_qp_solve_batch_device_s(&d, 0, H, Q.g, nullptr, Q.lb, Q.ub, nullptr, nullptr, opts, xc, (double*)(ws + c.fval), flagc,
                                                 (int*)(ws + c.iter), nullptr, nullptr, ws + c.qp, c.qp_bytes, stream)) return rc;
    MinlapGradParams C = minlap_grad_params(model, sp, L, nJ, N_s, N_c, v_cap, grip);   // the candidates: clamp(c + d, lo, hi), each with its plan's block
    C.cand = n_rho; C.check_width = check_width; C.margin = margin; C.line = xc; C.line_stride = N_c; C.base = line; C.lo = blo; C.hi = bhi;
    C.line_out = xc; C.T = Tc; C.grad = gradc;
    e = minlap_lapgrad_launch(C, par_values(par), par_stride(par), st);
    if (e != hipSuccess) return hipfail(e, "minlap_lapgrad_launch");
    MinlapSelectParams S; S.n_plans = n_plans; S.J = n_rho; S.N_c = N_c; S.it = it; S.K = iters; S.Tc = Tc; S.flagc = flagc; S.cc = xc; S.gradc = gradc;
    S.c = line; S.grad = grad; S.lap_hist = lap_hist; S.step_hist = step_hist;
    e = minlap_select_launch(S, st);
    if (e != hipSuccess) return hipfail(e, "minlap_select_launch");
  }
  if (iters > 0) {   // the table of the final control points, by the line-profile path
    PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
    P.line = line; P.line_stride = N_c; P.flag = nullptr; P.line_out = line; P.check_width = check_width; P.margin = margin;
    e = plan_line_profile_launch(P, par_values(par), par_stride(par), st);
    if (e != hipSuccess) return hipfail(e, "plan_line_profile_launch");
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
struct CellsCarve { size_t H, A, g, lb, ub, lbA, ubA, fval, iter, lambda, qp, total; long long qp_bytes; };
static int cells_carve(int n_plans, int N_s, int N_c, CellsCarve* c) {
  if (n_plans < 1 || N_c < FSAEMPC_LINE_MIN_NC || N_c > FSAEMPC_MAX_NV || N_s < 2 * N_c || N_s > FSAEMPC_LINE_MAX_NS) return FSAEMPC_ERR_ARG;
  const fsaempc_qp_desc d = {N_c, N_s, n_plans, 1};
  c->qp_bytes = fsaempc_qp_workspace_bytes_s(&d, cells_n_slack(N_c));
  if (c->qp_bytes < 0) return (int)c->qp_bytes;
  const size_t vec = align64((size_t)n_plans * N_c * sizeof(double)), row = align64((size_t)n_plans * N_s * sizeof(double));
  size_t off = 0;
  c->H = off; off += align64((size_t)N_c * N_c * sizeof(double));
  c->A = off; off += align64((size_t)N_s * N_c * sizeof(double));
  c->g = off; off += vec;
  c->lb = off; off += vec;
  c->ub = off; off += vec;
  c->lbA = off; off += row;
  c->ubA = off; off += row;
  c->fval = off; off += align64((size_t)n_plans * sizeof(double));
  c->iter = off; off += align64((size_t)n_plans * sizeof(int));
  c->lambda = off; off += align64((size_t)n_plans * ((size_t)N_c + N_s) * sizeof(double));
  c->qp = off; off += (size_t)c->qp_bytes;
  c->total = off;
  return 0;
}
long long fsaempc_plan_raceline_cells_workspace_bytes(int n_plans, int N_s, int N_c) {
  CellsCarve c;
  if (int rc = cells_carve(n_plans, N_s, N_c, &c)) return rc;
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
  if (!(margin >= 0 && margin < INFINITY)) return fail(FSAEMPC_ERR_ARG, "margin must be finite and >= 0");
  if (int rc = cells_shape_check(N_s, N_c)) return rc;
  CellsCarve c;
  if (int rc = cells_carve(n_plans, N_s, N_c, &c)) return fail(rc, "bad dimensions");
  if ((long long)c.total > workspace_bytes) return fail(FSAEMPC_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  double *H = (double*)(ws + c.H), *g = (double*)(ws + c.g), *lambda = row_lambda ? (double*)(ws + c.lambda) : nullptr;
  hipError_t e = raceline_qp_launch(line_qp_params(sp, L, N_s, N_c, H, g), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "raceline_qp_launch");
  R.n_plans = n_plans; R.N_s = N_s; R.N_c = N_c; R.L = L; R.margin = margin; R.A = (double*)(ws + c.A); R.lbA = (double*)(ws + c.lbA); R.ubA = (double*)(ws + c.ubA);
  R.g = g; R.lb = (double*)(ws + c.lb); R.ub = (double*)(ws + c.ub);
  e = cor_line_rows_launch(R, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cor_line_rows_launch");
  const fsaempc_qp_desc d = {N_c, N_s, n_plans, 1};
  if (int rc = fsaempc_qp_solve_batch_device_s(&d, cells_n_slack(N_c), H, g, R.A, R.lb, R.ub, R.lbA, R.ubA, opts, line, (double*)(ws + c.fval), flag,
                                               (int*)(ws + c.iter), lambda, nullptr, ws + c.qp, c.qp_bytes, stream)) return rc;
  if (row_lambda) {
    e = cor_line_lambda_launch(lambda, row_lambda, n_plans, N_s, N_c, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "cor_line_lambda_launch");
  }
  CorLineParams CL; CL.cor = R.cor;
  CL.n_plans = n_plans; CL.N_s = N_s; CL.N_c = N_c; CL.L = L; CL.margin = margin; CL.g = g; CL.lb = R.lb; CL.ub = R.ub; CL.line = line; CL.flag = flag;
  e = cor_line_void_launch(CL, (hipStream_t)stream);   // (no centre-line fallback: every plan whose flag is not 0 is NaN)
  if (e != hipSuccess) return hipfail(e, "cor_line_void_launch");
  PlanLineParams P = line_profile_params(model, sp, L, n_plans, N_s, N_c, v_cap, grip, table, t);
  P.line = line; P.line_stride = N_c; P.flag = nullptr; P.line_out = line; P.check_width = 0; P.margin = margin;
  e = plan_line_profile_launch(P, par_values(par), par_stride(par), (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "plan_line_profile_launch");
  return 0;
}

int fsaempc_corridor_line_rows_device(const fsaempc_corridor* cor, double L, int n_plans, int N_s, int N_c, double margin,
                                      double* A, double* lbA, double* ubA, void* stream) {
  CorLineRowsParams R;
  if (!cor) return fail(FSAEMPC_ERR_ARG, "null argument (corridor)");
  if (int rc = cor_check(cor, &R.cor)) return rc;
  if (!A || !lbA || !ubA) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (int rc = line_rows_check(L, n_plans, N_s, N_c, margin)) return rc;
  R.n_plans = n_plans; R.N_s = N_s; R.N_c = N_c; R.L = L; R.margin = margin; R.A = A; R.lbA = lbA; R.ubA = ubA; R.g = nullptr; R.lb = nullptr; R.ub = nullptr;
  hipError_t e = cor_line_rows_launch(R, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cor_line_rows_launch");
  return 0;
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
  if (!(margin >= 0 && margin < INFINITY)) return fail(FSAEMPC_ERR_ARG, "cones: margin must be finite and >= 0");
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
  hipError_t e = cor_from_cones_launch(P, (hipStream_t)stream);
  if (e != hipSuccess) return hipfail(e, "cor_from_cones_launch");
  return 0;
}

int fsaempc_selftest_mfma(void) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) return fail(FSAEMPC_ERR_NODEVICE, "no HIP device");
  char msg[256] = "";
  int bad = qp_selftest_mfma(msg, sizeof(msg));
  if (bad != 0) snprintf(g_err, sizeof(g_err), "%s", msg);
  return bad;
}

int fsaempc_selftest_lane_reduce(void) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) return fail(FSAEMPC_ERR_NODEVICE, "no HIP device");
  char msg[256] = "";
  int bad = qp_selftest_lane_reduce(msg, sizeof(msg));
  if (bad != 0) snprintf(g_err, sizeof(g_err), "%s", msg);
  return bad;
}

int fsaempc_selftest_diag_factor(void) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) return fail(FSAEMPC_ERR_NODEVICE, "no HIP device");
  char msg[256] = "";
  int bad = qp_selftest_diag_factor(msg, sizeof(msg));
  if (bad != 0) snprintf(g_err, sizeof(g_err), "%s", msg);
  return bad;
}

int fsaempc_selftest_initial_point(void) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) return fail(FSAEMPC_ERR_NODEVICE, "no HIP device");
  char msg[256] = "";
  int bad = qp_selftest_initial_point(msg, sizeof(msg));
  if (bad != 0) snprintf(g_err, sizeof(g_err), "%s", msg);
  return bad;
}

int fsaempc_debug_set_dump(double* out, int stage) { g_dump.store(out); g_dump_stage.store(stage); return 0; }

int fsaempc_qp_set_timing(int enable) {
  if (enable && !g_ev[0]) {
    for (int i = 0; i < 3; ++i) { hipError_t e = hipEventCreate(&g_ev[i]); if (e != hipSuccess) return hipfail(e, "hipEventCreate"); }
    for (int i = 0; i < 2; ++i) { hipError_t e = hipEventCreate(&g_evf[i]); if (e != hipSuccess) return hipfail(e, "hipEventCreate"); }
    for (int i = 0; i < 5; ++i) { hipError_t e = hipEventCreate(&g_evs[i]); if (e != hipSuccess) return hipfail(e, "hipEventCreate"); }
  }
  g_timing.store(enable != 0);
  return 0;
}

int fsaempc_ltv_get_timing(double* build_ms, double* prep_ms, double* solve_ms, double* post_ms) {
  if (!g_evf[0]) return fail(FSAEMPC_ERR_ARG, "timing was never enabled");
  hipError_t e = hipEventSynchronize(g_evf[1]);
  if (e != hipSuccess) return hipfail(e, "hipEventSynchronize (no fused step since timing was enabled?)");
  float t[4] = {0, 0, 0, 0};
  e = hipEventElapsedTime(&t[0], g_evf[0], g_ev[0]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  e = hipEventElapsedTime(&t[1], g_ev[0], g_ev[1]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  e = hipEventElapsedTime(&t[2], g_ev[1], g_ev[2]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  e = hipEventElapsedTime(&t[3], g_ev[2], g_evf[1]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  if (build_ms) *build_ms = t[0];
  if (prep_ms) *prep_ms = t[1];
  if (solve_ms) *solve_ms = t[2];
  if (post_ms) *post_ms = t[3];
  return 0;
}

int fsaempc_qp_get_timing(double* prep_ms, double* solve_ms) {
  if (!g_ev[0]) return fail(FSAEMPC_ERR_ARG, "timing was never enabled");
  hipError_t e = hipEventSynchronize(g_ev[2]);
  if (e != hipSuccess) return hipfail(e, "hipEventSynchronize");
  float a = 0, b = 0;
  e = hipEventElapsedTime(&a, g_ev[0], g_ev[1]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  e = hipEventElapsedTime(&b, g_ev[1], g_ev[2]); if (e != hipSuccess) return hipfail(e, "hipEventElapsedTime");
  if (prep_ms) *prep_ms = a;
  if (solve_ms) *solve_ms = b;
  return 0;
}

}  // extern "C"
