// cl_sensors.h -- Cartesian sensor models of the closed loop: what a car measures -- position, heading, body
// velocities, yaw rate and steering angle in the Cartesian frame -- and the measurement function of the filter that reads it, written
// once for the host and the device, and the internal interface between the C ABI and the kernels of cl_sensors.hip.
//
//   sensor layout     the model's state layout with (s, n, mu) replaced by (X, Y, psi): kinematic [X, Y, psi, v, delta], dynamic
//                     [X, Y, psi, x_d, y_d, theta_d, delta]
//   cls_y_true        the exact measurement out of the plant's 7 Cartesian states, as cl_pre_frame assembles x0: kinematic
//                     [c0, c1, c2, sqrt(c3^2 + c4^2), c6], dynamic c itself
//   cls_cart_from_y   the Cartesian vector a measurement stands for: kinematic (y0, y1, y2, y3, 0, 0, y4), dynamic y itself
//   ClsD              forward-mode dual number (value, derivative along one seeded direction), the formulas of nlp_model.h's Dl
//   cls_h             the measurement function h(x) (vehicle_models/curvilinear_to_cartesian.m:16-28) on doubles or on dual numbers:
//                     with the two Bezier tables at s, t = (-Y', X') / sqrt(X'^2 + Y'^2), h0 = X + n t_x, h1 = Y + n t_y,
//                     h2 = atan2(Y', X') + mu, h_i = x_i for i >= 3.  Seeded in state direction j it ends with column j of
//                     H = dh/dx, the second derivatives of the tables included (d tau / ds = 1 / dl inside a segment)
//   cls_angdiff       MATLAB's angdiff(alpha, beta), beta - alpha wrapped to [-pi, pi]: the text of cl_frame.h's angdiff (the heading
//                     innovation is cls_angdiff(h2, y2))
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction in it:
// tests/sensors_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include "fsaempc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLS_HD __host__ __device__ __forceinline__
#else
#define CLS_HD inline
#endif
#if defined(__clang__)
#define CLS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CLS_NO_CONTRACT
#endif

struct ClsD { double v, d; };

CLS_HD ClsD cls_mk(double v, double d) { ClsD r; r.v = v; r.d = d; return r; }
CLS_HD ClsD operator+(ClsD a, ClsD b) { CLS_NO_CONTRACT return cls_mk(a.v + b.v, a.d + b.d); }
CLS_HD ClsD operator-(ClsD a, ClsD b) { CLS_NO_CONTRACT return cls_mk(a.v - b.v, a.d - b.d); }
CLS_HD ClsD operator-(ClsD a) { return cls_mk(-a.v, -a.d); }
CLS_HD ClsD operator*(ClsD a, ClsD b) { CLS_NO_CONTRACT const double l = a.d * b.v, r = a.v * b.d; return cls_mk(a.v * b.v, l + r); }
CLS_HD ClsD operator/(ClsD a, ClsD b) { CLS_NO_CONTRACT const double q = a.v / b.v, t = q * b.d; return cls_mk(q, (a.d - t) / b.v); }
CLS_HD ClsD operator+(ClsD a, double b) { CLS_NO_CONTRACT return cls_mk(a.v + b, a.d); }
CLS_HD ClsD operator+(double a, ClsD b) { CLS_NO_CONTRACT return cls_mk(b.v + a, b.d); }
CLS_HD ClsD operator-(ClsD a, double b) { CLS_NO_CONTRACT return cls_mk(a.v - b, a.d); }
CLS_HD ClsD operator-(double a, ClsD b) { CLS_NO_CONTRACT return cls_mk(a - b.v, -b.d); }
CLS_HD ClsD operator*(ClsD a, double b) { CLS_NO_CONTRACT return cls_mk(a.v * b, a.d * b); }
CLS_HD ClsD operator*(double a, ClsD b) { CLS_NO_CONTRACT return cls_mk(b.v * a, b.d * a); }
CLS_HD ClsD operator/(ClsD a, double b) { CLS_NO_CONTRACT return cls_mk(a.v / b, a.d / b); }
CLS_HD double cls_sqrt(double a) { return sqrt(a); }
CLS_HD ClsD cls_sqrt(ClsD a) { CLS_NO_CONTRACT const double r = sqrt(a.v); return cls_mk(r, a.d / (2.0 * r)); }
CLS_HD double cls_atan2(double y, double x) { return atan2(y, x); }
CLS_HD ClsD cls_atan2(ClsD y, ClsD x) {
  CLS_NO_CONTRACT
  const double num = x.v * y.d - y.v * x.d, den = x.v * x.v + y.v * y.v;
  return cls_mk(atan2(y.v, x.v), num / den);
}
CLS_HD double cls_val(double a) { return a; }
CLS_HD double cls_val(ClsD a) { return a.v; }
// the local parameter of a segment as a function of the arc length s: d tau / ds = 1 / dl
CLS_HD double cls_tau(double tau, double, double) { return tau; }
CLS_HD ClsD cls_tau(double tau, ClsD s, double dl) { return cls_mk(tau, s.d / dl); }

// segment and local parameter of arc length t: the text of nlp_model.h's seg_lookup (a non-finite t indexes row 0)
CLS_HD void cls_seg_lookup(int M, double dl, double t, int& seg, double& tau) {
  CLS_NO_CONTRACT
  const double per = dl * (double)M;
  const double wraps = floor(t / per) * per;
  double r = t - wraps;
  if (r < 0) r += per;
  if (r >= per) r -= per;
  int i = 0;
  if (r >= 0 && r < per) i = (int)floor(r / dl);
  if (i >= M) i = M - 1;
  if (i < 0) i = 0;
  seg = i; tau = r / dl - (double)i;
}

// value and first derivative of one Bezier spline at the local parameter u of segment i (interpolate_spline{,_d}.m; the expressions of
// cl_frame.h's spline3)
template <class T> CLS_HD void cls_spline2(const double* P, int M, double dl, int i, T u, T& v, T& d) {
  CLS_NO_CONTRACT
  const double p0 = P[i], p1 = P[i + M], p2 = P[i + 2 * M], p3 = P[i + 3 * M];
  const T w = 1 - u;
  v = p0 * (w * w * w) + 3 * p1 * (w * w) * u + 3 * p2 * w * (u * u) + p3 * (u * u * u);
  d = (-3 * w * w * p0 + 3 * (3 * u * u - 4 * u + 1) * p1 + 3 * (2 * u - 3 * u * u) * p2 + 3 * u * u * p3) / dl;
}

// h(x): x and h hold nx entries (h must not alias x)
template <class T> CLS_HD void cls_h(int M, double dl, const double* xP, const double* yP, int nx, const T* x, T* h) {
  CLS_NO_CONTRACT
  int i; double tau;
  cls_seg_lookup(M, dl, cls_val(x[0]), i, tau);
  const T u = cls_tau(tau, x[0], dl);
  T X, Xd, Y, Yd;
  cls_spline2<T>(xP, M, dl, i, u, X, Xd);
  cls_spline2<T>(yP, M, dl, i, u, Y, Yd);
  T tx = -Yd, ty = Xd;
  const T nrm = cls_sqrt(tx * tx + ty * ty);
  tx = tx / nrm; ty = ty / nrm;
  h[0] = X + x[1] * tx;
  h[1] = Y + x[1] * ty;
  h[2] = cls_atan2(Yd, Xd) + x[2];
  for (int k = 3; k < nx; ++k) h[k] = x[k];
}

CLS_HD double cls_angdiff(double alpha, double beta) {
  CLS_NO_CONTRACT
  const double d = beta - alpha;
  const double a = d + M_PI, b = 2 * M_PI;
  const double wraps = floor(a / b) * b;
  double w = (a - wraps) - M_PI;
  if (w == -M_PI && d > 0) w = M_PI;
  return w;
}

CLS_HD void cls_y_true(int nx, const double* c, double* y) {
  CLS_NO_CONTRACT
  y[0] = c[0]; y[1] = c[1]; y[2] = c[2];
  if (nx == 5) { const double a = c[3] * c[3], b = c[4] * c[4]; y[3] = sqrt(a + b); y[4] = c[6]; }
  else { y[3] = c[3]; y[4] = c[4]; y[5] = c[5]; y[6] = c[6]; }
}

CLS_HD void cls_cart_from_y(int nx, const double* y, double* c) {
  c[0] = y[0]; c[1] = y[1]; c[2] = y[2];
  if (nx == 5) { c[3] = y[3]; c[4] = 0.0; c[5] = 0.0; c[6] = y[4]; }
  else { c[3] = y[3]; c[4] = y[4]; c[5] = y[5]; c[6] = y[6]; }
}

#if defined(__HIPCC__)
struct ClSenseParams {
  int nx, batch, sigma_per_instance;
  unsigned long long seed, id0, step;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double* sigma;            // nx, or batch x nx (sensor layout)
  const double* cart;             // batch x 7
  const double* x0_true;          // batch x nx
  const int* finished;            // optional
  double* y;                      // batch x nx (sensor layout)
  double* x_proj;                 // batch x nx (state layout)
  int* proj_lost;                 // batch: projections that lost the track so far
};
hipError_t cl_sense_launch(const ClSenseParams& P, hipStream_t st);

struct ClEstimateCartParams {
  int nx, batch, integ;           // integ: 0 Euler, 1 RK2, 2 RK4 (resolved by the caller)
  int q_per_instance, r_per_instance;
  double dt, L;
  int spM; double spdl; const double* xP; const double* yP;   // spline table (device)
  const double* q; const double* r; const double* p0;         // state layout; sensor layout; state layout
  const double* y;                // batch x nx (sensor layout)
  const double* x_proj;           // batch x nx
  const double* u_prev;           // car b reads u_prev[b * u_stride + 0 .. 1]
  long long u_stride;
  const int* finished;            // optional
  double* est_x;                  // batch x nx
  double* est_P;                  // batch x nx x nx
  int* est_count;                 // batch x 2
  double* x0_est; double* innov;  // batch x nx each
  double* nis;                    // batch
  double* F_out;                  // optional, batch x nx x nx
  double* x_prior;                // optional, batch x nx
  double* H_out;                  // optional, batch x nx x nx
};
// par (optional): the controller's parameter blocks, car b reads par + b * par_stride; null: the constants compiled in
hipError_t cl_estimate_cart_launch(const ClEstimateCartParams& P, hipStream_t st, const double* par = nullptr, int par_stride = 0);
#endif
