// planner.h -- the s-domain plan of the closed loop: the walk that resamples a plan in time, written once for the
// host and the device, and the internal interface between the C ABI and the kernels of planner.hip.
//
//   plan_walk   util/obtain_reference.m:18-48 for one car: cell index / ratio walk over the per-cell traversal times and the linear
//               interpolation of the six planner states, in the state layout of the model.  Same operations in the same order as
//               obtain_reference_kernel (reference.hip), so on a valid plan the seven rows are bit for bit the oracle's.
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLAN_HD __host__ __device__ __forceinline__
#else
#define PLAN_HD inline
#endif

PLAN_HD double plan_mod_floor(double a, double b) {   // MATLAB mod for b > 0
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a - floor(a / b) * b;
}

PLAN_HD bool plan_time_ok(double t) { return t > 0.0 && t < INFINITY; }   // a traversal time is finite and positive

// plan: 8 values per cell (n, mu, x_d, y_d, theta_d, delta, a, delta_d), t: traversal time per cell, Ns cells of length ds.
// xr: nx x Nt column-major.  nx = 7: the rows of obtain_reference.m:41-47; nx = 5: [s, n, mu, hypot(x_d, y_d), delta] (main.m:95's
// rule for the kinematic x0).
// The reference's inner `while (rto > 1)` never ends on a table whose times are all zero; here it advances at most Ns cells per
// horizon step, and a step that would need more (a lap in less than dt: no plan of a car) ends the walk.  So does the first cell the
// walk meets whose time is zero, negative, Inf or NaN: that column and every later one are NaN (the columns before it, walked over
// usable cells only, stay as they are).  The checks compare only; on a valid plan the arithmetic is the reference's.
// A non-finite s0 (a car whose state blew up) is walked from s0 = 0: finite placeholder rows, as the live generator gives them.
PLAN_HD void plan_walk(const double* plan, const double* t, int Ns, double ds, double s0, double dt, int Nt, int nx, double* xr) {
#if defined(__clang__)
#pragma clang fp contract(off)   // plain IEEE operations in source order: compared bit for bit with the oracle
#endif
  if (!(fabs(s0) < INFINITY)) s0 = 0.0;
  const double L = ds * Ns;
  // idx is kept 0-based here (MATLAB idx-1); rto as in the reference
  const double pos = plan_mod_floor(s0, L) / ds;                    // obtain_reference.m:21-22
  int idx = (pos >= 0 && pos < (double)Ns) ? (int)floor(pos) : 0;
  if (idx >= Ns) idx = Ns - 1;
  double rto = plan_mod_floor(pos, 1.0);
  const int idx1 = idx; const double rto1 = rto;
  for (int i = 0; i < Nt; ++i) {                                    // obtain_reference.m:24-35
    double t_rem = dt;
    const int idx_prev = idx; const double rto_prev = rto;
    bool ok = plan_time_ok(t[idx]);
    rto = rto_prev + t_rem / t[idx];
    t_rem -= t[idx_prev] * (1.0 - rto_prev);
    int adv = 0;
    while (ok && rto > 1.0 && adv < Ns) {
      idx = (idx + 1) % Ns;                                         // nxt()
      ok = plan_time_ok(t[idx]);
      rto = t_rem / t[idx];
      t_rem -= t[idx];
      ++adv;
    }
    if (!ok || rto > 1.0) {                                         // a cell without a usable time, or the bound: no finite row from here on
      for (int k = i * nx; k < Nt * nx; ++k) xr[k] = NAN;
      return;
    }
    const int nx_ = (idx + 1) % Ns;
    double* col = xr + (size_t)i * nx;
    // obtain_reference.m:41: mod(idx(i) + rto(i) - idx(1) - rto(1), N_s) * ds, same operands and order as the 1-based original
    col[0] = s0 + plan_mod_floor((double)(idx + 1) + rto - (double)(idx1 + 1) - rto1, (double)Ns) * ds;
    double v[6];
    for (int c = 0; c < 6; ++c) {                                   // n, mu, x_d, y_d, theta_d, delta  (:42-47)
      const double a0 = plan[(size_t)idx * 8 + c], a1 = plan[(size_t)nx_ * 8 + c];
      v[c] = a0 + (a1 - a0) * rto;
    }
    if (nx == 7) {
      for (int c = 0; c < 6; ++c) col[1 + c] = v[c];
    } else {
      col[1] = v[0]; col[2] = v[1]; col[3] = hypot(v[2], v[3]); col[4] = v[5];
    }
  }
}

#if defined(__HIPCC__)
// ---- internal interface between the C ABI (capi_plan.hip) and planner.hip ----
struct PlanProfileParams {
  int dynamic, n_plans, N_s;
  double ds, v_cap, grip;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  double* table;            // n_plans x N_s x 8
  double* t;                // n_plans x N_s
};
// par (optional): parameter blocks, plan p reads par + p * par_stride; null: the constants compiled in
hipError_t plan_profile_launch(const PlanProfileParams& P, const double* par, int par_stride, hipStream_t st);

struct PlanTable { const double* table; const double* t; int N_s; double ds; int per_instance; };
struct PlanRefParams {
  PlanTable plan;
  int nx, N, batch;
  double dt;
  const double* s0;         // batch
  double* x_ref;            // batch x (nx x N)
};
hipError_t plan_reference_launch(const PlanRefParams& P, hipStream_t st);

struct ClPrePlanParams {
  PlanTable plan;
  int nx, N, batch;
  double dt, L;
  int spM; double spdl; const double* xP; const double* yP;
  const double* cart;       // batch x 7
  const double* s_guess;    // batch
  double* x0;               // batch x nx
  double* x_ref;            // batch x (nx x N)
  int* finished;            // batch
};
hipError_t cl_pre_plan_launch(const ClPrePlanParams& P, hipStream_t st);
#endif
