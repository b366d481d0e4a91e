// ltv_model.h -- device functions shared by the LTV-MPC construction kernels (ltv_build_kernel.h; the sensitivity kernels of ltv_build.hip): the model
// Jacobians, the linearisation of one step and the per-step coefficients of the linearised constraint rows.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "nlp_model.h"

namespace {

template <class PAR> DEVINL void A_kin(const PAR p, const double* x, const Spl& sp, double* A) {  // 5x5 column-major
  const double lr_ratio = p.LR_RATIO, LR = p.LR;
  const double k = kappa(sp, x[0]);
  const double td = tan(x[4]);
  const double beta = atan(lr_ratio * td);
  const double s_mb = sin(x[2] + beta), c_mb = cos(x[2] + beta);
  const double sec = 1.0 / cos(x[4]);
  const double beta_d = lr_ratio * sec * sec / (1 + (lr_ratio * td) * (lr_ratio * td));
  const double denom_nk = 1.0 / (1.0 - x[1] * k);
  const double s_n = x[3] * c_mb * denom_nk * denom_nk * k;
  const double s_mu = -x[3] * s_mb * denom_nk;
  const double s_v = c_mb * denom_nk;
  const double s_delta = -x[3] * s_mb * denom_nk * beta_d;
  for (int i = 0; i < 25; ++i) A[i] = 0.0;
  A[0 + 1 * 5] = s_n; A[0 + 2 * 5] = s_mu; A[0 + 3 * 5] = s_v; A[0 + 4 * 5] = s_delta;
  A[1 + 2 * 5] = x[3] * c_mb; A[1 + 3 * 5] = s_mb; A[1 + 4 * 5] = x[3] * c_mb * beta_d;
  A[2 + 1 * 5] = -s_n * k; A[2 + 2 * 5] = -s_mu * k; A[2 + 3 * 5] = sin(beta) / LR - s_v * k;
  A[2 + 4 * 5] = x[3] * cos(beta) * beta_d / LR - s_delta * k;
}

// byp = {Fcr, Fcr_d, vr, denom_vr2, x_d_hat, x_d_hat_d, vf, denom_vf2}; A may be null
template <class PAR> DEVINL void A_dyn(const PAR p, const double* x, const Spl& sp, double* A, double* byp) {
  const double LF = p.LF, LR = p.LR, PB = p.PB, PC = p.PC, PD = p.PD, PE = p.PE;
  const double n = x[1], mu = x[2], x_d = x[3], y_d = x[4], th_d = x[5], delta = x[6];
  const double m = p.M, I = p.IZ;
  const double x_d_hat = x_d + 5 * exp(-x_d / 5);
  const double x_d_hat_d = 1 - exp(-x_d / 5);
  const double alpha_f = delta - atan((y_d + LF * th_d) / x_d_hat);
  const double alpha_r = -atan((y_d - LR * th_d) / x_d_hat);
  const double Fzf = p.FZF, Fzr = p.FZR;
  const double af_arg = PB * alpha_f - PE * (PB * alpha_f - atan(PB * alpha_f));
  const double ar_arg = PB * alpha_r - PE * (PB * alpha_r - atan(PB * alpha_r));
  const double Fcf = Fzf * PD * sin(PC * atan(af_arg));
  const double Fcr = Fzr * PD * sin(PC * atan(ar_arg));
  const double Fcf_d = Fzf * PD * cos(PC * atan(af_arg)) * PC / (1 + af_arg * af_arg) * (PB - PE * (PB - PB / (1 + PB * PB * alpha_f * alpha_f)));
  const double Fcr_d = Fzr * PD * cos(PC * atan(ar_arg)) * PC / (1 + ar_arg * ar_arg) * (PB - PE * (PB - PB / (1 + PB * PB * alpha_r * alpha_r)));
  const double vf = (y_d + LF * th_d) / x_d_hat, vr = (y_d - LR * th_d) / x_d_hat;
  const double denom_vf2 = 1.0 / (1 + vf * vf), denom_vr2 = 1.0 / (1 + vr * vr);
  if (A) {
    const double k = kappa(sp, x[0]);
    const double denom_nk = 1.0 / (1.0 - n * k);
    const double cm = cos(mu), sm = sin(mu), cd = cos(delta), sd = sin(delta);
    const double s_n = (x_d * cm - y_d * sm) * denom_nk * denom_nk * k;
    const double s_mu = (-x_d * sm - y_d * cm) * denom_nk;
    const double s_xd = cm * denom_nk, s_yd = -sm * denom_nk;
    for (int i = 0; i < 49; ++i) A[i] = 0.0;
    A[0 + 1 * 7] = s_n; A[0 + 2 * 7] = s_mu; A[0 + 3 * 7] = s_xd; A[0 + 4 * 7] = s_yd;
    A[1 + 2 * 7] = x_d * cm - y_d * sm; A[1 + 3 * 7] = sm; A[1 + 4 * 7] = cm;
    A[2 + 1 * 7] = -s_n * k; A[2 + 2 * 7] = -s_mu * k; A[2 + 3 * 7] = -s_xd * k; A[2 + 4 * 7] = -s_yd * k; A[2 + 5 * 7] = 1;
    A[3 + 3 * 7] = -Fcf_d * denom_vf2 * vf * sd * x_d_hat_d / (m * x_d_hat);
    A[3 + 4 * 7] = (Fcf_d * denom_vf2 * sd / x_d_hat + m * th_d) / m;
    A[3 + 5 * 7] = (Fcf_d * denom_vf2 * LF * sd / x_d_hat + m * y_d) / m;
    A[3 + 6 * 7] = (-Fcf * cd - Fcf_d * sd) / m;
    A[4 + 3 * 7] = (Fcr_d * denom_vr2 * vr * x_d_hat_d / x_d_hat + Fcf_d * denom_vf2 * vf * cd * x_d_hat_d / x_d_hat - m * th_d) / m;
    A[4 + 4 * 7] = (-Fcr_d * denom_vr2 / x_d_hat - Fcf_d * denom_vf2 / x_d_hat * cd) / m;
    A[4 + 5 * 7] = (Fcr_d * denom_vr2 * LR / x_d_hat - Fcf_d * denom_vf2 * LF / x_d_hat * cd - m * x_d_hat) / m;
    A[4 + 6 * 7] = (-Fcf * sd + Fcf_d * cd) / m;
    A[5 + 3 * 7] = (LF * Fcf_d * denom_vf2 * vf * cd * x_d_hat_d / x_d_hat - LR * Fcr_d * denom_vr2 * vr * x_d_hat_d / x_d_hat) / I;
    A[5 + 4 * 7] = (-LF * Fcf_d * denom_vf2 * cd / x_d_hat + LR * Fcr_d * denom_vr2 / x_d_hat) / I;
    A[5 + 5 * 7] = (-LF * Fcf_d * denom_vf2 * LF * cd / x_d_hat - LR * Fcr_d * denom_vr2 * LR / x_d_hat) / I;
    A[5 + 6 * 7] = (-LF * Fcf * sd + LF * Fcf_d * cd) / I;
  }
  if (byp) { byp[0] = Fcr; byp[1] = Fcr_d; byp[2] = vr; byp[3] = denom_vr2; byp[4] = x_d_hat; byp[5] = x_d_hat_d; byp[6] = vf; byp[7] = denom_vf2; }
}

template <int NX> DEVINL void mmul(const double* A, const double* B, double* C, int ncol) {  // C = A(NXxNX) B(NX x ncol)
  for (int j = 0; j < ncol; ++j)
    for (int i = 0; i < NX; ++i) {
      double s = 0;
      for (int p = 0; p < NX; ++p) s += A[i + p * NX] * B[p + j * NX];
      C[i + j * NX] = s;
    }
}
template <int NX, class PAR> DEVINL void model_A(const PAR p, const double* x, const Spl& sp, double* A) {
  if (NX == 5) A_kin(p, x, sp, A); else A_dyn(p, x, sp, A, nullptr);
}

// Linearise step k about (xi, ui): writes Ad = I + dt*A, Bd = dt*B, dd = dt*d   (sequential_integration.m:16-18)
// integ: 0 Euler (euler_*_curvilinear.m:24-30), 1 midpoint rule (rk2_*_curvilinear.m:25-50), 2 classical RK4
// (rk4_*_curvilinear.m:25-59).  The reference drivers use rk2 for the kinematic and rk4 for the dynamic model
// (ltvmpc_kinetmatic_curvilinear.m:38, ltvmpc_dynamic_curvilinear.m:38); the others are the alternates kept beside them.
template <int NX, class PAR> DEVINL void linearise_step(const PAR p, const double* xi, const double* ui, const Spl& sp, double dt, int integ,
                                             double* Ad, double* Bd, double* dd) {
  constexpr int NN = NX * NX;
  double Bc[NX * 2];
  for (int i = 0; i < NX * 2; ++i) Bc[i] = 0.0;
  Bc[3] = 1.0; Bc[(NX - 1) + NX] = 1.0;  // B_curv_kin.m:12-16 / B_curv_dyn.m:12-18
  double f[NX], Ai[NN], Bi[NX * 2];
  if (integ == 0) {
    model_f<NX>(p, xi, ui, sp, f);
    model_A<NX>(p, xi, sp, Ai);
    for (int j = 0; j < NX * 2; ++j) Bi[j] = Bc[j];
  } else if (integ == 1) {
    double k1[NX], xs[NX], F1[NN], F2[NN], Tm[NN], TB[NX * 2];
    model_f<NX>(p, xi, ui, sp, k1);
    for (int j = 0; j < NX; ++j) xs[j] = xi[j] + k1[j] * dt / 2;
    model_f<NX>(p, xs, ui, sp, f);
    model_A<NX>(p, xi, sp, F1);
    model_A<NX>(p, xs, sp, F2);
    for (int j = 0; j < NN; ++j) Tm[j] = F1[j] * dt / 2;
    for (int j = 0; j < NX; ++j) Tm[j + j * NX] += 1;
    mmul<NX>(F2, Tm, Ai, NX);
    mmul<NX>(F2, Bc, TB, 2);
    for (int j = 0; j < NX * 2; ++j) Bi[j] = Bc[j] + TB[j] * dt / 2;
  } else {
    double k1[NX], k2[NX], k3[NX], k4[NX], xs[NX];
    double F[NN], K[NN], Tm[NN], Ks[NN], U[NX * 2], Us[NX * 2], TB[NX * 2];
    model_f<NX>(p, xi, ui, sp, k1);
    model_A<NX>(p, xi, sp, K);                       // dkdx1
    for (int j = 0; j < NN; ++j) Ks[j] = K[j];
    for (int j = 0; j < NX * 2; ++j) { U[j] = Bc[j]; Us[j] = Bc[j]; }
    for (int j = 0; j < NX; ++j) xs[j] = xi[j] + k1[j] * dt / 2;
    model_f<NX>(p, xs, ui, sp, k2);
    model_A<NX>(p, xs, sp, F);
    for (int j = 0; j < NN; ++j) Tm[j] = K[j] * dt / 2;
    for (int j = 0; j < NX; ++j) Tm[j + j * NX] += 1;
    mmul<NX>(F, Tm, K, NX);                        // dkdx2
    mmul<NX>(F, U, TB, 2);
    for (int j = 0; j < NX * 2; ++j) U[j] = Bc[j] + TB[j] * dt / 2;   // dkdu2
    for (int j = 0; j < NN; ++j) Ks[j] += 2 * K[j];
    for (int j = 0; j < NX * 2; ++j) Us[j] += 2 * U[j];
    for (int j = 0; j < NX; ++j) xs[j] = xi[j] + k2[j] * dt / 2;
    model_f<NX>(p, xs, ui, sp, k3);
    model_A<NX>(p, xs, sp, F);
    for (int j = 0; j < NN; ++j) Tm[j] = K[j] * dt / 2;
    for (int j = 0; j < NX; ++j) Tm[j + j * NX] += 1;
    mmul<NX>(F, Tm, K, NX);                        // dkdx3
    mmul<NX>(F, U, TB, 2);
    for (int j = 0; j < NX * 2; ++j) U[j] = Bc[j] + TB[j] * dt / 2;   // dkdu3
    for (int j = 0; j < NN; ++j) Ks[j] += 2 * K[j];
    for (int j = 0; j < NX * 2; ++j) Us[j] += 2 * U[j];
    for (int j = 0; j < NX; ++j) xs[j] = xi[j] + k3[j] * dt;
    model_f<NX>(p, xs, ui, sp, k4);
    model_A<NX>(p, xs, sp, F);
    for (int j = 0; j < NN; ++j) Tm[j] = K[j] * dt;
    for (int j = 0; j < NX; ++j) Tm[j + j * NX] += 1;
    mmul<NX>(F, Tm, K, NX);                        // dkdx4
    mmul<NX>(F, U, TB, 2);
    for (int j = 0; j < NX * 2; ++j) U[j] = Bc[j] + TB[j] * dt / 2;   // dkdu4: dt/2 as in rk4_*.m:52 (quirk C-3)
    for (int j = 0; j < NN; ++j) Ai[j] = (Ks[j] + K[j]) / 6;
    for (int j = 0; j < NX * 2; ++j) Bi[j] = (Us[j] + U[j]) / 6;
    for (int j = 0; j < NX; ++j) f[j] = (k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]) / 6;
  }
  for (int r = 0; r < NX; ++r) {
    double s = f[r];
    for (int c = 0; c < NX; ++c) s -= Ai[r + c * NX] * xi[c];
    for (int c = 0; c < 2; ++c) s -= Bi[r + c * NX] * ui[c];
    dd[r] = s * dt;
  }
  for (int j = 0; j < NN; ++j) Ad[j] = Ai[j] * dt;
  for (int j = 0; j < NX; ++j) Ad[j + j * NX] += 1;
  for (int j = 0; j < NX * 2; ++j) Bd[j] = Bi[j] * dt;
}

// Step 4a of the build: the coefficients of step k's linearised constraint rows, at the state xl they are linearised at
// (kinematic: 3 values; dynamic: 16).  Shared by the build and by the affine maps of the sensitivities (ltv_affine_kernel).
template <int NX, class PAR> DEVINL void step_coef(const PAR p, const double* xl, const Spl& sp, double* ck) {
  const double LF = p.LF, LR = p.LR;
  if (NX == 5) {
    // kinematic_tyre_linearise_constraints.m:18-32 ; g = v^2 delta/(lr+lf)
    ck[0] = 2 * xl[3] * xl[4] / p.WB;
    ck[1] = xl[3] * xl[3] / p.WB;
    ck[2] = xl[3] * xl[3] * xl[4] / p.WB;  // g0
  } else {
    double byp[8];
    A_dyn(p, xl, sp, nullptr, byp);
    const double Fcr = byp[0], Fcr_d = byp[1], vr = byp[2], dvr2 = byp[3], xh = byp[4], xhd = byp[5], vf = byp[6], dvf2 = byp[7];
    // dynamic_slip_linearise_constraints.m:26-30 : rows (alpha_r, alpha_f) coefficients on states 4..7
    ck[0] = dvr2 * vr * xhd / xh; ck[1] = -dvr2 / xh; ck[2] = dvr2 * LR / xh; ck[3] = 0.0;
    ck[4] = dvf2 * vf * xhd / xh; ck[5] = -dvf2 / xh; ck[6] = -dvf2 * LF / xh; ck[7] = 1.0;
    ck[8] = -atan(vr); ck[9] = xl[6] - atan(vf);
    // dynamic_tyre_linearise_constraints.m:41-49 : C_j = dal_j * ck[10..12] on states 4..6
    ck[10] = -Fcr_d * dvr2 * vr * xhd / xh / p.M; ck[11] = Fcr_d * dvr2 / xh / p.M; ck[12] = -Fcr_d * dvr2 * LR / xh / p.M;
    ck[13] = Fcr; ck[14] = 0; ck[15] = 0;
  }
}

}  // namespace
