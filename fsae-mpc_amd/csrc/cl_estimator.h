// cl_estimator.h -- the state estimator of the closed loop: the scalar rules of the extended Kalman filter of
// cl_estimator.hip, written once for the host and the device, and the internal interface between the C ABI and the kernel.
//
//   cle_finite        |v| < Inf (false for NaN)
//   cle_measured      component i is measured iff r_i is finite and >= 0 (-0.0 counts as 0); +Inf, a negative value and NaN mean
//                     "not measured"
//   cle_rebase        the arc length of the prior brought to the lap the measurement is in: x + L rint((z - x) / L), rint to the
//                     nearest whole number with ties to even (so z - x = +-L/2 moves nothing); x itself with L == 0 (no re-basing)
//                     or s unmeasured
//   cle_prior_bad     an entry of x-, or of P- (diag: it lies on the diagonal), that forces a re-initialisation before the update:
//                     not finite, or a diagonal entry <= 0
//   cle_post_bad      the same after the update: not finite, or a diagonal entry < 0 (an exact measurement, r_i = 0, leaves P_ii = 0)
//   cle_gain_ok       the scalar update of a component is applied only with an innovation variance s_i = P_ii + r_i > 0
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction in it:
// tests/estimator_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include "fsaempc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLE_HD __host__ __device__ __forceinline__
#else
#define CLE_HD inline
#endif

CLE_HD int cle_finite(double v) { return fabs(v) < INFINITY; }

CLE_HD int cle_measured(double r) { return r >= 0.0 && r < INFINITY; }

CLE_HD double cle_rebase(double x, double z, double L, int s_measured) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(L > 0.0) || !s_measured) return x;
  const double laps = rint((z - x) / L);
  const double shift = L * laps;
  return x + shift;
}

CLE_HD int cle_prior_bad(double v, int diag) { return !cle_finite(v) || (diag && !(v > 0.0)); }

CLE_HD int cle_post_bad(double v, int diag) { return !cle_finite(v) || (diag && v < 0.0); }

CLE_HD int cle_gain_ok(double s) { return s > 0.0; }

#if defined(__HIPCC__)
struct ClEstimateParams {
  int nx, batch, integ;           // integ: 0 Euler, 1 RK2, 2 RK4 (resolved by the caller)
  int q_per_instance, r_per_instance;
  double dt, L;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double* q; const double* r; const double* p0;         // nx or batch x nx; nx or batch x nx; nx
  const double* z;                // batch x nx
  const double* x_start;          // batch x nx
  const double* u_prev;           // car b reads u_prev[b * u_stride + 0 .. 1]
  long long u_stride;
  const int* finished;            // optional
  double* est_x;                  // batch x nx
  double* est_P;                  // batch x nx x nx
  int* est_count;                 // batch x 2: periods since the last (re-)initialisation, resets
  double* x0_est; double* innov;  // batch x nx each
  double* nis;                    // batch
  double* F_out;                  // optional, batch x nx x nx
  double* x_prior;                // optional, batch x nx
};
// par (optional): the controller's parameter blocks, car b reads par + b * par_stride; null: the constants compiled in
hipError_t cl_estimate_launch(const ClEstimateParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
#endif
