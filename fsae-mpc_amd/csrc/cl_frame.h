// cl_frame.h -- device helpers of the closed loop's frame transform, shared by cl_pre_kernel (plant.hip) and cl_pre_plan_kernel
// (planner.hip): the Bezier table with its derivatives, the Newton search of spline/closest_point.m, MATLAB's angdiff, and
// main.m:93-104 for one car.  Internal header: anonymous namespace (device code of each translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "nlp_model.h"   // Spl, seg_lookup

namespace {

DEVINL double mmod(double a, double b) { return a - floor(a / b) * b; }
// value, first and second derivative of one Bezier spline at t (interpolate_spline{,_d,_dd}.m)
DEVINL void spline3(const double* P, int M, double dl, double t, double& v, double& d, double& dd) {
  int i; double u;
  seg_lookup(M, dl, t, i, u);
  const double p0 = P[i], p1 = P[i + M], p2 = P[i + 2 * M], p3 = P[i + 3 * M];
  const double w = 1 - u;
  v = p0 * (w * w * w) + 3 * p1 * (w * w) * u + 3 * p2 * w * (u * u) + p3 * (u * u * u);
  d = (-3 * w * w * p0 + 3 * (3 * u * u - 4 * u + 1) * p1 + 3 * (2 * u - 3 * u * u) * p2 + 3 * u * u * p3) / dl;
  dd = (6 * w * p0 + 6 * (3 * u - 2) * p1 + 6 * (1 - 3 * u) * p2 + 6 * u * p3) / (dl * dl);
}

DEVINL double closest_point(const Spl& sp, double x0, double y0, double s, double epsilon) {
  double delta = epsilon * 2;
  int guard = 0;
  while (fabs(delta) > epsilon && guard++ < 1000) {   // bounded: every thread leaves the loop (the reference spins on NaN)
    double X, Xd, Xdd, Y, Yd, Ydd;
    spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
    spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
    const double dist_d = 2 * (X - x0) * Xd + 2 * (Y - y0) * Yd;
    const double dist_dd = 2 * (X - x0) * Xdd + 2 * Xd * Xd + 2 * (Y - y0) * Ydd + 2 * Yd * Yd;
    delta = dist_d / dist_dd;
    s = s - delta;
  }
  return s;
}

DEVINL double angdiff(double alpha, double beta) {   // MATLAB angdiff: beta - alpha wrapped to [-pi, pi]
  const double d = beta - alpha;
  double w = mmod(d + M_PI, 2 * M_PI) - M_PI;
  if (w == -M_PI && d > 0) w = M_PI;
  return w;
}

// main.m:93-104 for one car: Cartesian -> curvilinear frame, x0 assembly for the model, lap check, out-of-race rule.
// c: the car's 7 Cartesian states; x0: nx; fin: the car's entry of `finished`.
// (cl_pre_kernel keeps these lines in its own body: routed through this function the compiler schedules its loads differently, and
//  that kernel's code is not to change.  The two must stay the same text.)
DEVINL void cl_pre_frame(const Spl& sp, int nx, double L, const double* c, double s_guess, double* x0, int* fin) {
  const double s = closest_point(sp, c[0], c[1], s_guess, 0.01);
  double X, Xd, Xdd, Y, Yd, Ydd;
  spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
  spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
  double tx = -Yd, ty = Xd;
  const double nrm = sqrt(tx * tx + ty * ty);
  tx /= nrm; ty /= nrm;
  const double n = (c[0] - X) * tx + (c[1] - Y) * ty;
  const double mu = angdiff(atan2(Yd, Xd), c[2]);
  x0[0] = s; x0[1] = n; x0[2] = mu;
  if (nx == 5) { x0[3] = sqrt(c[3] * c[3] + c[4] * c[4]); x0[4] = c[6]; }   // main.m:95
  else { x0[3] = c[3]; x0[4] = c[4]; x0[5] = c[5]; x0[6] = c[6]; }           // main.m:97
  if (s >= L) *fin = 1;                                                      // main.m:101-104
  {   // the car is out when the frame transform lost the track (Newton diverged) or its state left every physical range
    bool okc = fabs(s) < INFINITY && fabs(n) < 3.0 && fabs(c[3]) < 100.0 && fabs(c[4]) < 100.0;   // 3 m off a 1.5 m wide track: out of the race
    for (int j = 0; j < 7; ++j) okc = okc && fabs(c[j]) < 1e6;
    if (!okc) {
      *fin = 2;
      for (int j = 0; j < nx; ++j) x0[j] = 0.0;   // finite placeholder data for the (ignored) QP of this car
    }
  }
}

}  // namespace
