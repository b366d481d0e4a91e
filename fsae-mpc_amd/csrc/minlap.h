// minlap.h -- the minimum-time racing line of the s-domain plans: the lap time T(c) of the profile on a line and its
// gradient in the control points c by the adjoint of that profile, written once for the host and the device, and the internal
// interface between the C ABI and the kernels of minlap.hip.
//
// Forward (the profile on a line, plan_profile.h; what plan_profile_kernel<.., LINE = true> runs): per cell n, n', a = 1 - n kappa, r, mu (rl_point), dl = ds r,
// m = kappa + (mu_next - mu_prev) / (2 ds), k = m / r, K = max(|k|, 1e-12), vlat = min(v_cap, sqrt(A_lat / K)); from the first minimum
// i0 of vlat one forward pass (acceleration out of the predecessor over the predecessor's cell) and one backward pass (braking into
// the successor over the cell's own length); T = sum dl / v.
//
//   (plan_profile.h)  pp_ax<DYN, true>: the longitudinal limit with its partials in v and K; pp_passes with PpRecord: the two passes,
//                     keeping the speeds after the forward pass and, per cell and pass, whether the recurrence won the min
//   ml_cell_seed      the adjoints T puts on a cell's speed and length
//   ml_reverse        the two passes undone in reverse order: adjoints of vlat, K and dl
//   ml_cell_kbar      vlat and K = max(|k|, 1e-12) undone: the adjoint of k
//   ml_cell_mr        k = m / r and dl = ds r undone: the adjoints of m and r
//   ml_cell_n         r, mu and a undone: the adjoints of n and of the basis sum of n' (n' = that sum / h)
//   ml_grad_entry     grad_j = sum over the cells whose window holds control point j, in ascending cell order (no atomics)
//   ml_lapgrad_host   all of it for one plan on plain arrays (the stand-alone host program of tests/test_minlap_cpu.py)
//
// The first part compiles as plain C++ (a host program may include this file without the HIP headers).  No FMA contraction:
// tests/minlap_numpy.py restates every function operation for operation.
#pragma once
#include <math.h>
#include <stddef.h>
#include "raceline.h"
#include "plan_profile.h"

#define ML_HD RL_HD

// T = sum dl_i / v_i: what it puts on v_i and dl_i
ML_HD void ml_cell_seed(double dl, double v, double& vbar, double& dlbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  vbar = -dl / (v * v);
  dlbar = 1.0 / v;
}

// The backward pass undone from its last step to its first, then the forward pass the same way.  In: vbar, dlbar of ml_cell_seed,
// Kbar = 0; v, vf, won of pp_passes (PpRecord); v0 = vlat[i0] (the source of the first forward step).  Out: vbar the adjoint of vlat, Kbar of
// K, dlbar of dl.  A step's source is the cell's final speed (backward) or its speed after the forward pass (forward), except the
// first step of each pass, which read cell i0 before that pass set it.
template <bool DYN> ML_HD void ml_reverse(const MlCar& p, int Ns, int i0, double A_lat, double grip, double v0, const double* k,
                                          const double* dl, const double* v, const double* vf, const int* won, double* vbar,
                                          double* Kbar, double* dlbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double dv, dK;
  int i = i0;                                        // step j set cell (i0 - j) mod Ns: j = Ns is cell i0
  for (int j = Ns; j >= 1; --j) {
    const int nx = i + 1 < Ns ? i + 1 : 0;
    if (won[i] & ML_WON_BWD) {
      const double vn = j == 1 ? vf[nx] : v[nx];
      const double Kn = fmax(fabs(k[nx]), 1e-12);
      const double a = pp_ax<DYN, true>(p, vn, Kn, A_lat, grip, &dv, &dK);
      const double qbar = vbar[i] / (2.0 * v[i]);
      vbar[i] = 0.0;
      vbar[nx] += qbar * (2.0 * vn + 2.0 * dl[i] * dv);
      Kbar[nx] += qbar * (2.0 * dl[i] * dK);
      dlbar[i] += qbar * (2.0 * a);
    }
    i = nx;
  }
  i = i0;                                            // step j set cell (i0 + j) mod Ns: j = Ns is cell i0
  for (int j = Ns; j >= 1; --j) {
    const int pr = i > 0 ? i - 1 : Ns - 1;
    if (won[i] & ML_WON_FWD) {
      const double vp = j == 1 ? v0 : vf[pr];
      const double Kp = fmax(fabs(k[pr]), 1e-12);
      const double a = pp_ax<DYN, true>(p, vp, Kp, A_lat, grip, &dv, &dK);
      const double qbar = vbar[i] / (2.0 * vf[i]);
      vbar[i] = 0.0;
      vbar[pr] += qbar * (2.0 * vp + 2.0 * dl[pr] * dv);
      Kbar[pr] += qbar * (2.0 * dl[pr] * dK);
      dlbar[pr] += qbar * (2.0 * a);
    }
    i = pr;
  }
}

// vlat = min(v_cap, sqrt(A_lat / K)) and K = max(|k|, 1e-12) undone: the adjoint of the line's curvature k
ML_HD double ml_cell_kbar(double A_lat, double v_cap, double k, double vbar, double Kbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double K = fmax(fabs(k), 1e-12);
  const double s = sqrt(A_lat / K);
  if (s < v_cap) Kbar += vbar * (-0.5 * s / K);
  if (!(fabs(k) > 1e-12)) return 0.0;
  return k < 0.0 ? -Kbar : Kbar;
}

// k = m / r and dl = ds r undone
ML_HD void ml_cell_mr(double kbar, double m, double r, double ds, double dlbar, double& mbar, double& rbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  mbar = kbar / r;
  rbar = -kbar * m / (r * r) + ds * dlbar;
}

// r = sqrt(a^2 + n'^2), mu = atan(n' / a) and a = 1 - n kappa undone.  nbar: the adjoint of n; ndbar: the adjoint of n', already
// divided by h (n' = (sum of dweights times control points) / h).
ML_HD void ml_cell_n(double rbar, double mubar, double a, double nd, double r, double kappa, double h, double& nbar, double& ndbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q = a * a + nd * nd;
  const double abar = rbar * a / r - mubar * nd / q;
  ndbar = (rbar * nd / r + mubar * a / q) / h;
  nbar = -abar * kappa;
}

// grad_j = sum_i B_ij nbar_i + B'_ij ndbar_i.  Control point j is in the window of the cells of the knot spans j - 2 .. j + 1
// (cyclic), with weight index 3 .. 0; span jj holds the cells ceil(jj N_s / N_c) .. ceil((jj + 1) N_s / N_c) - 1.  The spans are
// visited so that the cells ascend: those that wrapped to the start of the lap, those in range, those that wrapped to its end.
ML_HD double ml_grad_entry(int j, int Ns, int Nc, const double* nbar, const double* ndbar) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double g = 0.0;
  for (int part = 0; part < 3; ++part) {
    for (int d = 0; d < 4; ++d) {
      const int raw = j - 2 + d;
      const int which = raw >= Nc ? 0 : (raw >= 0 ? 1 : 2);
      if (which != part) continue;
      const int jj = raw >= Nc ? raw - Nc : (raw >= 0 ? raw : raw + Nc);
      const int i0 = (int)(((long long)jj * Ns + Nc - 1) / Nc), i1 = (int)(((long long)(jj + 1) * Ns + Nc - 1) / Nc);
      for (int i = i0; i < i1; ++i) {
        int ji; double u, w[4], wd[4];
        rl_basis(i, Ns, Nc, ji, u);
        rl_weights(u, w);
        rl_dweights(u, wd);
        g += rl_pick<4>(w, 3 - d) * nbar[i] + rl_pick<4>(wd, 3 - d) * ndbar[i];
      }
    }
  }
  return g;
}

// One plan on plain arrays: T and grad (N_c) of control points c on a track whose centre-line curvature at the cells is kap.  work:
// 11 N_s doubles, won: N_s ints.  Returns 0, or 1 for a NaN plan (a < 0.1 in a cell: T and grad are NaN).
template <bool DYN> inline int ml_lapgrad_host(const MlCar& p, double A_lat, double grip, double v_cap, int Ns, int Nc, double L,
                                               const double* kap, const double* c, double* work, int* won, double* T, double* grad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ds = L / Ns, h = L / Nc;
  double *k = work, *mu = work + Ns, *dl = work + 2 * Ns, *v = work + 3 * Ns, *vf = work + 4 * Ns, *vbar = work + 5 * Ns,
         *Kbar = work + 6 * Ns, *dlbar = work + 7 * Ns, *av = work + 8 * Ns, *ndv = work + 9 * Ns, *rv = work + 10 * Ns;
  bool ok = true;
  for (int i = 0; i < Ns; ++i) {
    const RlPoint q = rl_point(c, i, Ns, Nc, h, kap[i]);
    ok = ok && (q.a >= 0.1);
    mu[i] = q.mu; rv[i] = q.r; av[i] = q.a; ndv[i] = q.nd;
  }
  if (!ok) {
    *T = NAN;
    for (int j = 0; j < Nc; ++j) grad[j] = NAN;
    return 1;
  }
  for (int i = 0; i < Ns; ++i) {
    const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
    k[i] = (kap[i] + (mu[nx] - mu[pr]) / (2.0 * ds)) / rv[i];
    dl[i] = ds * rv[i];
  }
  for (int i = 0; i < Ns; ++i) v[i] = pp_corner_speed(k[i], A_lat, v_cap);
  const int i0 = pp_first_min(v, Ns);
  const double v0 = v[i0];
  pp_passes<DYN>(p, Ns, i0, A_lat, grip, k, (const double*)dl, v, PpRecord{vf, won});
  double sum = 0.0;
  for (int i = 0; i < Ns; ++i) {
    sum += dl[i] / v[i];
    ml_cell_seed(dl[i], v[i], vbar[i], dlbar[i]);
    Kbar[i] = 0.0;
  }
  *T = sum;
  ml_reverse<DYN>(p, Ns, i0, A_lat, grip, v0, k, dl, v, vf, won, vbar, Kbar, dlbar);
  for (int i = 0; i < Ns; ++i) {
    const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
    const double kbar = ml_cell_kbar(A_lat, v_cap, k[i], vbar[i], Kbar[i]);
    const double m = kap[i] + (mu[nx] - mu[pr]) / (2.0 * ds);
    ml_cell_mr(kbar, m, rv[i], ds, dlbar[i], Kbar[i], dlbar[i]);   // (mbar over Kbar, rbar over dlbar)
  }
  for (int i = 0; i < Ns; ++i) {
    const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
    const double mubar = (Kbar[pr] - Kbar[nx]) / (2.0 * ds);
    ml_cell_n(dlbar[i], mubar, av[i], ndv[i], rv[i], kap[i], h, vbar[i], vf[i]);   // (nbar over vbar, ndbar over vf)
  }
  for (int j = 0; j < Nc; ++j) grad[j] = ml_grad_entry(j, Ns, Nc, vbar, vf);
  return 0;
}

#if defined(__HIPCC__)
// ---- internal interface between the C ABI (capi_plan.hip) and minlap.hip ----
struct MinlapGradParams {
  int dynamic, n_waves, N_s, N_c;
  int cand;                 // waves per plan: wave w belongs to plan w / cand (its block, width check, base, lo, hi)
  double ds, h, v_cap, grip;
  int check_width; double margin;   // check_width: a plan with N_MAX_p - margin <= 0 is NaN
  int spM; double spdl; const double* xP; const double* yP;
  const double* line; int line_stride;   // wave w reads line + w * line_stride (0: shared)
  const double* base;       // optional, per plan x N_c: the wave's control points are clamp(base + line, lo, hi) ...
  const double* lo;         // ... with lo, hi per plan x N_c
  const double* hi;
  double* line_out;         // optional, n_waves x N_c: the control points the wave ran on (NaN for a NaN plan); may be `line`
  double* T; int T_stride;  // wave w writes T[w * T_stride]
  double* grad;             // n_waves x N_c
};
hipError_t minlap_lapgrad_launch(const MinlapGradParams& P, const double* par, int par_stride, hipStream_t st);
size_t minlap_lapgrad_lds_bytes(int N_s, int N_c);

// per plan p and candidate j: g = grad_p / rho_j, lb = lo_p - c_p, ub = hi_p - c_p
struct MinlapCandParams { int n_plans, J, N_c; double rho[16]; const double* grad; const double* c; const double* lo; const double* hi;
                          double* g; double* lb; double* ub; };
hipError_t minlap_candidates_launch(const MinlapCandParams& P, hipStream_t st);

// per plan: the least finite T among the candidates whose QP flag is 0 (first index on ties) replaces the incumbent if strictly
// smaller; the winner's control points and gradient become the plan's.  lap_hist[p * hist_stride + it + 1], step_hist[p * K + it].
struct MinlapSelectParams { int n_plans, J, N_c, it, K; const double* Tc; const int* flagc; const double* cc; const double* gradc;
                            double* c; double* grad; double* lap_hist; int* step_hist; };
hipError_t minlap_select_launch(const MinlapSelectParams& P, hipStream_t st);

// a user's boxes as the bounds of the initial line QP: lb = lo, ub = hi (both NaN where !(lo < hi)) and the plan's copy of g
struct MinlapBoxParams { int n_plans, N_c; const double* lo; const double* hi; double* g; double* lb; double* ub; };
hipError_t minlap_box_launch(const MinlapBoxParams& P, hipStream_t st);
#endif
