// capi_common.h -- what the units of the C ABI (capi_qp.hip, capi_ltv.hip, capi_cl.hip, capi_plan.hip) share: the error text, the
// roctx ranges, the workspace allocator and the checks more than one unit makes.  Everything here lives in one namespace with hidden
// visibility: it crosses the units, but never becomes a dynamic symbol of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <dlfcn.h>
#include <atomic>
#include "fsaempc.h"
#include "ltv_build.h"
#include "corridor.h"

namespace capi __attribute__((visibility("hidden"))) {
// One buffer per thread, whichever unit wrote it (defined in capi_qp.hip, as all of these).  __thread, not thread_local: across units
// a thread_local is reached through an init wrapper whose weak, hidden, never-defined init function does not resolve to NULL in a
// shared library, and the first fail() outside capi_qp.hip would jump into it.
extern __thread char g_err[512];
// Diagnostics (fsaempc_debug_set_dump, fsaempc_qp_set_timing): process-wide switches meant for ONE measuring thread (bench.py,
// tools/).  Atomics keep a solve on another thread well-defined while they are flipped; the event triple itself is not
// per-thread, so timing figures are only meaningful when a single thread launches solves.
extern std::atomic<double*> g_dump; extern std::atomic<int> g_dump_stage;
extern std::atomic<bool> g_timing; extern hipEvent_t g_ev[3];
extern hipEvent_t g_evf[2];   // fused step: before the construction kernel, after the post-solve kernel
extern hipEvent_t g_evs[5];   // SQP sweep: compaction+gather | build | solve | line search
extern double g_sqp_ms[4];    // summed over the sweeps of the last SQP call: compaction + gather, build, solve, line search

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

inline int fail(int code, const char* fmt, const char* a = "") { snprintf(g_err, sizeof(g_err), fmt, a); return code; }
inline int hipfail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu || e == hipErrorInsufficientDriver)
             ? FSAEMPC_ERR_NODEVICE : FSAEMPC_ERR_HIP;
}
// the return code of a launch (or any HIP call): `if (int rc = launched(x_launch(...), "x_launch")) return rc;`
inline int launched(hipError_t e, const char* where) { return e == hipSuccess ? 0 : hipfail(e, where); }

inline size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }
// the spline half of a kernel parameter struct (the structs spell it with the same four names)
template <class T> void set_spline(T* P, const fsaempc_spline* sp) { P->spM = sp->M; P->spdl = sp->dl; P->xP = sp->xP; P->yP = sp->yP; }

// One bump allocator behind every workspace layout.  A layout is written once, as a function that walks it: without a base the walk
// yields the size (the *_workspace_bytes functions), with the caller's buffer the same walk yields the pointers.  Addresses are
// integers here, so the size query does no arithmetic on a null pointer (its pointers are all NULL).
struct Bump {
  uintptr_t base; size_t off;
  explicit Bump(void* base_, size_t start = 0) : base((uintptr_t)base_), off(start) {}
  // cnt elements of T at the next multiple of `align` bytes
  template <class T> T* take(size_t cnt, size_t align = 64) {
    off = (off + align - 1) & ~(align - 1);
    const size_t at = off;
    off += cnt * sizeof(T);
    return base ? (T*)(base + at) : nullptr;
  }
};

// a NULL block (or NULL values) selects the kernels with the constants compiled in
inline const double* par_values(const fsaempc_ltv_params* par) { return par ? par->values : nullptr; }
inline int par_stride(const fsaempc_ltv_params* par) { return par && par->per_instance ? FSAEMPC_NPAR : 0; }
inline bool pos_finite(double v) { return v > 0 && v < INFINITY; }
inline int margin_check(double margin, const char* prefix = "") {
  return margin >= 0 && margin < INFINITY ? 0 : fail(FSAEMPC_ERR_ARG, "%smargin must be finite and >= 0", prefix);
}

inline int ltv_ns(int model) { return model == FSAEMPC_MODEL_KINEMATIC ? 1 : 4; }
inline int ltv_integ(const fsaempc_ltv_desc* d) {
  return d->integrator >= 0 ? d->integrator : (d->model == FSAEMPC_MODEL_KINEMATIC ? FSAEMPC_INT_RK2 : FSAEMPC_INT_RK4);   // ltvmpc_*.m:38
}
inline int ltv_check(const fsaempc_ltv_desc* d, const fsaempc_spline* sp) {
  if (!d || !sp || !sp->xP || !sp->yP) return fail(FSAEMPC_ERR_ARG, "null argument");
  if (d->model != FSAEMPC_MODEL_KINEMATIC && d->model != FSAEMPC_MODEL_DYNAMIC) return fail(FSAEMPC_ERR_ARG, "unknown model");
  if (d->N <= 0 || d->batch < 0 || !(d->dt > 0) || sp->M <= 0 || !(sp->dl > 0)) return fail(FSAEMPC_ERR_ARG, "bad dimensions");
  if (d->integrator < FSAEMPC_INT_DEFAULT || d->integrator > FSAEMPC_INT_RK4) return fail(FSAEMPC_ERR_ARG, "unknown integrator");
  if (ltv_build_lds_bytes(fsaempc_ltv_nx(d->model), d->N, 256) > 160 * 1024) return fail(FSAEMPC_ERR_DIM, "horizon too long for the LDS staging");
  return 0;
}

/* ---- s-varying track corridors ---- */
// the descriptor as the kernels take it; every refusal names the argument
inline int cor_check(const fsaempc_corridor* cor, CorTable* out) {
  if (!cor->n_lo) return fail(FSAEMPC_ERR_ARG, "corridor: n_lo is NULL");
  if (!cor->n_hi) return fail(FSAEMPC_ERR_ARG, "corridor: n_hi is NULL");
  if (cor->N_w < 2) return fail(FSAEMPC_ERR_ARG, "corridor: N_w must be >= 2");
  if (!pos_finite(cor->ds)) return fail(FSAEMPC_ERR_ARG, "corridor: ds must be finite and > 0");
  out->n_lo = cor->n_lo; out->n_hi = cor->n_hi; out->N_w = cor->N_w; out->ds = cor->ds; out->stride = cor->per_instance ? cor->N_w : 0;
  return 0;
}
}  // namespace capi
