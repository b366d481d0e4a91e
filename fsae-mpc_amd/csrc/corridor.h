// corridor.h -- s-varying track corridors: the table of include/fsaempc.h's fsaempc_corridor as the kernels see it,
// its lookup, and the internal interface between the C ABI and the kernels of corridor.hip.
//
// A corridor is two periodic tables over arc length, n_lo (right edge) and n_hi (left edge) at s_i = i ds, i = 0 .. N_w - 1,
// ds = L / N_w, linear in between.  Lookup at a finite s (negative values and values past L included):
//   q = s / ds wrapped into [0, N_w), i = floor(q), u = q - i, value = t[i] + u (t[(i + 1) mod N_w] - t[i])
// in this form and not (1 - u) a + u b, so that a constant table returns the constant exactly (u * 0 = 0).  No FMA contraction:
// tests/corridor_numpy.py restates the lookup operation for operation.
// A non-finite s, or one of the two cells read where n_lo < n_hi does not hold, gives NaN for both limits of that lookup only.
//
// What the corridor replaces is a width and nothing else:
//   MPC rows      lbA[2N + k] = n_lo(s_k) - pred_n,k, ubA[3N + k] = n_hi(s_k) - pred_n,k at s_k = x_lin[k nx], the point the row's
//                 coefficients and kappa are linearised at (quirk C-8).  The first-order term -n_hi'(s) (s_k - s_lin,k) is left out:
//                 the stated approximation of 6l.  The matrix A and the 1e10 / -1e10 fillers of the rows' other sides stay.
//   lap report    v = max(n - n_hi(s), n_lo(s) - n) in place of |n| - N_MAX
//   racing line   per control point the tightest limits of the cells whose basis touches it, minus the margin; or, opt-in, one
//                 general constraint row per cell with the control points free (cor_line_rows_launch)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "plant.h"

// stride: doubles between the tables of consecutive instances / plans (N_w, or 0 for one shared corridor)
struct CorTable { const double* n_lo; const double* n_hi; int N_w; double ds; int stride; };

#if defined(__HIPCC__)
__device__ __forceinline__ void cor_lookup(const CorTable& c, int inst, double s, double& lo, double& hi) {
#pragma clang fp contract(off)
  lo = NAN; hi = NAN;
  const double Nw = (double)c.N_w;
  double q = s / c.ds;
  if (!(fabs(q) < INFINITY)) return;
  q = q - Nw * floor(q / Nw);
  if (!(q >= 0.0) || q >= Nw) q = 0.0;   // (the wrap's own rounding: the point N_w is the point 0)
  const int i = (int)q;
  const int i1 = i + 1 < c.N_w ? i + 1 : 0;
  const double u = q - (double)i;
  const double* tl = c.n_lo + (size_t)inst * (size_t)c.stride;
  const double* th = c.n_hi + (size_t)inst * (size_t)c.stride;
  const double l0 = tl[i], l1 = tl[i1], h0 = th[i], h1 = th[i1];
  if (!(l0 < h0) || !(l1 < h1)) return;
  lo = l0 + u * (l1 - l0);
  hi = h0 + u * (h1 - h0);
}
#endif

// the 2N track-row bounds of a built QP, one thread per (instance, step); pred: the build's output (batch x nx N)
struct CorRowsParams {
  int nx, N, nC, batch;
  const double* x_lin;   // batch x (nx x N)
  const double* pred;    // batch x (nx x N)
  double* lbA;           // batch x nC
  double* ubA;
  CorTable cor;
};
hipError_t cor_rows_launch(const CorRowsParams& P, hipStream_t st);

// cl_metrics_launch (plant.h) with the track violation taken against the corridor at the recorded (s, n) = (x0[0], x0[1])
hipError_t cor_metrics_launch(const ClMetricsParams& P, const CorTable& cor, hipStream_t st, const double* par = nullptr, int par_stride = 0);

// Bounds of the line QP per plan from the corridor: for control point j
//   lb_j = max (n_lo(s_i) + margin), ub_j = min (n_hi(s_i) - margin) over the plan's cells i with floor(i N_c / N_s) in
//   {j - 2, j - 1, j, j + 1} (cyclic), s_i = i L / N_s
// and the plan's copy of g, as raceline_bounds_launch.  A control point with lb_j >= ub_j (or a NaN limit) gets NaN for both bounds:
// the QP of that plan then has non-finite data and the solve answers -1 before its first iteration, for that plan alone.
// cor_line_void_launch, after the solve, writes NaN into the control points of every plan whose flag is not 0; the profile kernel
// (given no flags, so it has no centre-line fallback: the centre line may lie outside a corridor) turns those into NaN plans.
struct CorLineParams {
  int n_plans, N_s, N_c;
  double L, margin;
  double* g; double* lb; double* ub;   // n_plans x N_c each (g: row 0 filled by raceline_qp_launch; NULL: bounds only)
  double* line;                        // n_plans x N_c: the solve's output (cor_line_void_launch only)
  const int* flag;                     // n_plans: the solve's exit flags (cor_line_void_launch only)
  CorTable cor;
};
hipError_t cor_line_bounds_launch(const CorLineParams& P, hipStream_t st);
hipError_t cor_line_void_launch(const CorLineParams& P, hipStream_t st);

// The cell-wise form of the line QP's corridor: one general constraint row per cell, lbA_i <= n_i <= ubA_i with
//   n_i = sum_m w_m(u_i) c[(j_i - 1 + m) mod N_c]  (rl_offset_row of raceline.h),  lbA_i = n_lo(s_i) + margin,  ubA_i = n_hi(s_i) - margin,
// s_i = i L / N_s.  The matrix depends on (N_s, N_c) alone: one A (N_s x N_c, column-major) for the batch, lbA / ubA per plan.  A cell
// whose lookup is NaN, or where lbA_i < ubA_i does not hold, gets NaN for both: that plan's QP has non-finite data and the solve
// answers -1 before its first iteration, for that plan alone.  The control points are free: lb = -1e10, ub = 1e10 (the filler of the
// LTV rows, beyond the solver's inf_bound).  Every element of every output given is written.
struct CorLineRowsParams {
  int n_plans, N_s, N_c;
  double L, margin;
  double* A;                           // N_s x N_c, column-major
  double* lbA; double* ubA;            // n_plans x N_s each
  double* g; double* lb; double* ub;   // n_plans x N_c each (g: row 0 filled by raceline_qp_launch); all three NULL: rows only
  CorTable cor;
};
hipError_t cor_line_rows_launch(const CorLineRowsParams& P, hipStream_t st);
// row_lambda[p][i] = lambda[p][N_c + i]: the multipliers of the cell rows out of the solver's nV + nC per plan
hipError_t cor_line_lambda_launch(const double* lambda, double* row_lambda, int n_plans, int N_s, int N_c, hipStream_t st);
