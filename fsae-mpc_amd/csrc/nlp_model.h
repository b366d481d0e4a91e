// nlp_model.h -- device-side model of the LTV-MPC / NLP path shared by ltv_build.hip and sqp.hip: the track curvature of the spline
// table, the two continuous models f(x, u) (templated on the scalar type: double, or the dual number Dl of the exact Jacobians)
// and the integrator step of the NLP's rollout.  Internal header: everything lives in an anonymous namespace (device code of each
// translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "mpc_params.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

struct Spl { int M; double dl; const double* xP; const double* yP; };

DEVINL void seg_lookup(int M, double dl, double t, int& seg, double& tau) {
  const double per = dl * (double)M;
  double r = t - floor(t / per) * per;  // MATLAB mod()
  if (r < 0) r += per;
  if (r >= per) r -= per;
  int i = 0;
  if (r >= 0 && r < per) i = (int)floor(r / dl);   // a non-finite arc length (a car whose state blew up) must not index the table
  if (i >= M) i = M - 1;
  if (i < 0) i = 0;
  seg = i; tau = r / dl - (double)i;
}
// Forward-mode dual number (value, derivative along one direction): the exact Jacobians of the NLP build (EXACT = true) are the
// derivatives of the very model functions below, kappa'(s) of the spline table included.
struct Dl {
  double v, d;
  Dl() = default;
  DEVINL Dl(double a, double b) : v(a), d(b) {}
  DEVINL explicit Dl(double a) : v(a), d(0.0) {}   // a constant
};
using ::sin; using ::cos; using ::tan; using ::atan; using ::exp; using ::pow;
DEVINL Dl operator+(Dl a, Dl b) { return {a.v + b.v, a.d + b.d}; }
DEVINL Dl operator-(Dl a, Dl b) { return {a.v - b.v, a.d - b.d}; }
DEVINL Dl operator-(Dl a) { return {-a.v, -a.d}; }
DEVINL Dl operator*(Dl a, Dl b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
DEVINL Dl operator/(Dl a, Dl b) { const double q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
DEVINL Dl operator+(Dl a, double b) { return {a.v + b, a.d}; }
DEVINL Dl operator+(double a, Dl b) { return {a + b.v, b.d}; }
DEVINL Dl operator-(Dl a, double b) { return {a.v - b, a.d}; }
DEVINL Dl operator-(double a, Dl b) { return {a - b.v, -b.d}; }
DEVINL Dl operator*(Dl a, double b) { return {a.v * b, a.d * b}; }
DEVINL Dl operator*(double a, Dl b) { return {a * b.v, a * b.d}; }
DEVINL Dl operator/(Dl a, double b) { return {a.v / b, a.d / b}; }
DEVINL Dl operator/(double a, Dl b) { const double q = a / b.v; return {q, -q * b.d / b.v}; }
DEVINL Dl sin(Dl a) { return {::sin(a.v), ::cos(a.v) * a.d}; }
DEVINL Dl cos(Dl a) { return {::cos(a.v), -::sin(a.v) * a.d}; }
DEVINL Dl tan(Dl a) { const double t = ::tan(a.v); return {t, (1 + t * t) * a.d}; }
DEVINL Dl atan(Dl a) { return {::atan(a.v), a.d / (1 + a.v * a.v)}; }
DEVINL Dl exp(Dl a) { const double e = ::exp(a.v); return {e, e * a.d}; }
DEVINL Dl pow(Dl a, double p) { return {::pow(a.v, p), p * ::pow(a.v, p - 1) * a.d}; }
DEVINL double val(double a) { return a; }
DEVINL double val(Dl a) { return a.v; }

template <class T> DEVINL T kappa(const Spl& sp, T s) {
  int i; double ut;
  seg_lookup(sp.M, sp.dl, val(s), i, ut);
  T u;
  if constexpr (sizeof(T) == sizeof(double)) u = T(ut);
  else u = T(ut, s.d / sp.dl);          // d(tau)/ds = 1/dl inside a segment
  const int M = sp.M;
  const double x0 = sp.xP[i], x1 = sp.xP[i + M], x2 = sp.xP[i + 2 * M], x3 = sp.xP[i + 3 * M];
  const double y0 = sp.yP[i], y1 = sp.yP[i + M], y2 = sp.yP[i + 2 * M], y3 = sp.yP[i + 3 * M];
  const T b0 = -3 * (1 - u) * (1 - u), b1 = 3 * (3 * u * u - 4 * u + 1), b2 = 3 * (2 * u - 3 * u * u), b3 = 3 * u * u;
  const T c0 = 6 * (1 - u), c1 = 6 * (3 * u - 2), c2 = 6 * (1 - 3 * u), c3 = 6 * u;
  const T Xd = (b0 * x0 + b1 * x1 + b2 * x2 + b3 * x3) / sp.dl, Yd = (b0 * y0 + b1 * y1 + b2 * y2 + b3 * y3) / sp.dl;
  const T Xdd = (c0 * x0 + c1 * x1 + c2 * x2 + c3 * x3) / (sp.dl * sp.dl), Ydd = (c0 * y0 + c1 * y1 + c2 * y2 + c3 * y3) / (sp.dl * sp.dl);
  return (Xd * Ydd - Xdd * Yd) / pow(Xd * Xd + Yd * Yd, 1.5);
}

// ---- kinematic model (f_curv_kin.m:13-29, A_curv_kin.m:15-55) ----
// (every model function takes the constants from a policy object p: mpc_params.h)
template <class T, class PAR> DEVINL void f_kin(const PAR p, const T* x, const T* u, const Spl& sp, T* f) {
  const double lr_ratio = p.LR_RATIO, LR = p.LR;
  const T k = kappa(sp, x[0]);
  const T beta = atan(lr_ratio * tan(x[4]));
  const T s_mb = sin(x[2] + beta), c_mb = cos(x[2] + beta);
  const T denom_nk = 1.0 / (1.0 - x[1] * k);
  f[0] = x[3] * c_mb * denom_nk;
  f[1] = x[3] * s_mb;
  f[2] = x[3] * sin(beta) / LR - x[3] * c_mb * denom_nk * k;
  f[3] = u[0];
  f[4] = u[1];
}
// ---- dynamic model (f_curv_dyn.m:13-62, A_curv_dyn.m:15-106) ----
template <class T, class PAR> DEVINL void f_dyn(const PAR p, const T* x, const T* u, const Spl& sp, T* f) {
  const double VM = p.M, VI = p.IZ, LF = p.LF, LR = p.LR, PB = p.PB, PC = p.PC, PD = p.PD, PE = p.PE;
  const T n = x[1], mu = x[2], x_d = x[3], y_d = x[4], th_d = x[5], delta = x[6];
  const T Fx = u[0] * VM;
  const T x_d_hat = x_d + 5 * exp(-x_d / 5);
  const T k = kappa(sp, x[0]);
  const T denom_nk = 1.0 / (1.0 - n * k);
  const T alpha_f = delta - atan((y_d + LF * th_d) / x_d_hat);
  const T alpha_r = -atan((y_d - LR * th_d) / x_d_hat);
  const double Fzf = p.FZF, Fzr = p.FZR;
  const T Fcf = Fzf * PD * sin(PC * atan(PB * alpha_f - PE * (PB * alpha_f - atan(PB * alpha_f))));
  const T Fcr = Fzr * PD * sin(PC * atan(PB * alpha_r - PE * (PB * alpha_r - atan(PB * alpha_r))));
  f[0] = (x_d * cos(mu) - y_d * sin(mu)) * denom_nk;
  f[1] = x_d * sin(mu) + y_d * cos(mu);
  f[2] = th_d - (x_d * cos(mu) - y_d * sin(mu)) * denom_nk * k;
  f[3] = (Fx - Fcf * sin(delta) + VM * y_d * th_d) / VM;
  f[4] = (Fcr + Fcf * cos(delta) - VM * x_d * th_d) / VM;
  f[5] = (LF * Fcf * cos(delta) - LR * Fcr) / VI;
  f[6] = u[1];
}
template <int NX, class T, class PAR> DEVINL void model_f(const PAR p, const T* x, const T* u, const Spl& sp, T* f) {
  if (NX == 5) f_kin(p, x, u, sp, f); else f_dyn(p, x, u, sp, f);
}
// One step of the NLP's rollout x+ = Psi(x, u) (integ: 0 Euler, 1 midpoint RK2, 2 classical RK4).  T = Dl gives the derivative of
// the step along the seeded direction: the exact linearisation of the NLP build (ltv_build.hip, EXACT = true).
template <int NX, class T, class PAR> DEVINL void psi_step(const PAR p, const T* x, const T* u, const Spl& sp, double dt, int integ, T* xn) {
  T k1[NX], xs[NX];
  model_f<NX>(p, x, u, sp, k1);
  if (integ == 0) {
    for (int j = 0; j < NX; ++j) xn[j] = x[j] + dt * k1[j];
  } else if (integ == 1) {
    T k2[NX];
    for (int j = 0; j < NX; ++j) xs[j] = x[j] + k1[j] * dt / 2;
    model_f<NX>(p, xs, u, sp, k2);
    for (int j = 0; j < NX; ++j) xn[j] = x[j] + dt * k2[j];
  } else {
    T k2[NX], k3[NX], k4[NX];
    for (int j = 0; j < NX; ++j) xs[j] = x[j] + k1[j] * dt / 2;
    model_f<NX>(p, xs, u, sp, k2);
    for (int j = 0; j < NX; ++j) xs[j] = x[j] + k2[j] * dt / 2;
    model_f<NX>(p, xs, u, sp, k3);
    for (int j = 0; j < NX; ++j) xs[j] = x[j] + k3[j] * dt;
    model_f<NX>(p, xs, u, sp, k4);
    for (int j = 0; j < NX; ++j) xn[j] = x[j] + dt * ((k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]) / 6);
  }
}

}  // namespace
