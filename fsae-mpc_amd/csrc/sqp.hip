// sqp.hip -- the per-sweep kernels of the batched SQP of the nonlinear MPC step (DESIGN.md "Nonlinear MPC: batched SQP").
//
// The NLP: z = (u_1..u_N, s); x_k = Psi(x_{k-1}, u_k), x_0 = x0 (nlp_model.h psi_step); cost = the one generate_qp encodes
// (Q, 10 Q at k = N, R = 10 I, linear slack costs R_soft, constant included: ltvmpc_*.m:32-35, :60); the rows of the LTV build in
// nonlinear form, row k evaluated at (x_k, u_k).  Hard rows: v_k >= 0 and |delta_k| <= 0.4.  Soft rows (kinematic: |n_k| <= 0.75 + s,
// |v_k^2 delta_k / (lr + lf)| <= 5 + s, one shared slack; dynamic: |n_k| <= 0.75 + s_1, |alpha_r| <= 0.1 + s_2, |alpha_f| <= 0.1 + s_3,
// 12-gon rows in (u_k(1), Fcr(x_k) / 280) <= s_4).  Input bounds and s >= 0 are boxes.
//
// Kernels: init (rollout of u_init, minimal slacks, merit), compaction of the instances still running into an index list,
// gather of their inputs, and the line search: one 64-lane wavefront per running instance, lane i < T evaluates the trial step
// alpha_i = 2^-i (rollout, slack reset, l1 merit) at the same time as the others; the largest alpha that satisfies Armijo is taken.
#include <hip/hip_runtime.h>
#include <math.h>
#include "sqp.h"
#include "nlp_model.h"

namespace {

// slack costs (ltvmpc_*.m:35); every constant comes from the policy object p (mpc_params.h)
template <class PAR> DEVINL double rsoft(const PAR p, int nx, int j) {
  return (nx == 5 || j == 0) ? p.R_SOFT0 : (j == 3 ? p.R_SOFT3 : (j == 1 ? p.R_SOFT1 : p.R_SOFT2));
}

struct Eval { double J, viol1, vmax; };

// Objective, hard violation (l1 sum and max) and reset slacks of the point u = clamp(uc + alpha (zu - uc)), s = max(s_in, s_min(x(u))).
// uout / xout (may be null) receive u and the rollout; uout may alias uc (each entry is read before it is written).
// ell0 (runtime constants only): ac0[12], al0[12], dac[12], dal[12] of the instance's tyre ellipse (sqp_ellipse).
template <int NX, class PAR> DEVINL Eval nlp_eval(const PAR p, const double* ell0, const SqpParams& P, const Spl& sp, int i, const double* uc, const double* zu, double alpha,
                                       const double* s_in, double* s_out, double* uout, double* xout) {
  constexpr int NS = NX == 5 ? 1 : 4;
  const int N = P.N, R = NX * N;
  const double* x0 = P.x0 + (size_t)i * NX;
  const double* xr = P.x_ref + (size_t)i * R;
  double x[NX], xn[NX], smin[NS];
  for (int j = 0; j < NX; ++j) x[j] = x0[j];
  for (int j = 0; j < NS; ++j) smin[j] = 0.0;
  double Jx = 0, Ju = 0, v1 = 0, vm = 0;
  for (int k = 0; k < N; ++k) {
    double u[2];
    for (int c = 0; c < 2; ++c) {
      const double lim = c ? p.U_STEER_MAX : p.U_ACC_MAX;   // input boxes (ltvmpc_*.m:28-29)
      const double v = uc[2 * k + c] + alpha * (zu[2 * k + c] - uc[2 * k + c]);
      u[c] = fmin(fmax(v, -lim), lim);
      Ju += (c ? p.R_STEER : p.R_ACC) * u[c] * u[c];   // R = [10, 10] (ltvmpc_*.m:34)
    }
    if (uout) { uout[2 * k] = u[0]; uout[2 * k + 1] = u[1]; }
    psi_step<NX>(p, x, u, sp, P.dt, P.integ, xn);
    for (int j = 0; j < NX; ++j) x[j] = xn[j];
    if (xout) for (int j = 0; j < NX; ++j) xout[(size_t)k * NX + j] = x[j];
    const double wq = (k == N - 1) ? p.Q_TERMINAL : 1.0;   // ltvmpc_*.m:32 (Q_terminal = 10 Q, :33)
    for (int r = 0; r < 3; ++r) { const double d = x[r] - xr[(size_t)k * NX + r]; Jx += wq * p.QW[r] * d * d; }
    const double h1 = fmax(0.0, p.below_vmin(x[3])), h2 = fmax(0.0, fabs(x[NX - 1]) - p.DELTA_MAX);
    v1 += h1 + h2; vm = fmax(vm, fmax(h1, h2));
    smin[0] = fmax(smin[0], fabs(x[1]) - p.N_MAX);
    if constexpr (NX == 5) {
      smin[0] = fmax(smin[0], fabs(x[3] * x[3] * x[4] / p.WB) - p.ALAT_MAX);
    } else {
      const double LF = p.LF, LR = p.LR, PB = p.PB, PC = p.PC, PD = p.PD, PE = p.PE;
      const double xh = x[3] + 5 * exp(-x[3] / 5);
      const double ar = -atan((x[4] - LR * x[5]) / xh), af = x[6] - atan((x[4] + LF * x[5]) / xh);
      smin[1] = fmax(smin[1], fabs(ar) - p.SLIP_MAX);
      smin[2] = fmax(smin[2], fabs(af) - p.SLIP_MAX);
      const double Fzr = p.FZR;
      const double Fcr = Fzr * PD * sin(PC * atan(PB * ar - PE * (PB * ar - atan(PB * ar))));
      for (int j = 0; j < 12; ++j) {   // dynamic_tyre_linearise_constraints.m:33-39, as in ltv_build.hip
        double ac0, al0, dac, dal;
        if constexpr (PAR::RT) {
          ac0 = ell0[j]; al0 = ell0[12 + j]; dac = ell0[24 + j]; dal = ell0[36 + j];
        } else {
          const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
          ac0 = p.ELL_LAT * sin(th0); al0 = p.ELL_LONG * cos(th0);
          dac = p.ELL_LAT * sin(th1) - ac0; dal = p.ELL_LONG * cos(th1) - al0;
        }
        smin[3] = fmax(smin[3], (u[0] - al0) * dac - (Fcr / p.M - ac0) * dal);
      }
    }
  }
  double Js = 0;
  for (int j = 0; j < NS; ++j) { s_out[j] = fmax(fmax(s_in[j], smin[j]), 0.0); Js += rsoft(p, NX, j) * s_out[j]; }
  // (a non-finite rollout makes Jx NaN: such a point is never accepted)
  return Eval{Jx + Ju + Js, v1, vm};
}

// The 48 constants of an instance's tyre ellipse, once per wavefront (LDS; dynamic model, runtime constants only)
template <int NX, class PAR> DEVINL void sqp_ellipse(const PAR p, int lane, double* ell0) {
  if constexpr (PAR::RT && NX == 7) {
    if (lane < 12) {
      const int j = lane;
      const double th0 = 2 * M_PI * (double)j / 12, th1 = (j + 1 == 12) ? 2 * M_PI : 2 * M_PI * (double)(j + 1) / 12;
      const double ac0 = p.ELL_LAT * sin(th0), al0 = p.ELL_LONG * cos(th0);
      ell0[j] = ac0; ell0[12 + j] = al0; ell0[24 + j] = p.ELL_LAT * sin(th1) - ac0; ell0[36 + j] = p.ELL_LONG * cos(th1) - al0;
    }
    __syncthreads();
  }
}

DEVINL double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

template <int NX, class PAR> __global__ __launch_bounds__(64) void sqp_init_kernel(SqpParams P, const double* u_init, typename PAR::Args pa) {
  constexpr int NS = NX == 5 ? 1 : 4;
  const int i = blockIdx.x, lane = threadIdx.x, N = P.N;
  const PAR p = par_get<PAR>(pa, i);
  __shared__ double ell0[PAR::RT ? 48 : 1];
  sqp_ellipse<NX>(p, lane, ell0);
  if (P.merit) for (int k = lane; k < P.max_sweeps; k += 64) P.merit[(size_t)i * P.max_sweeps + k] = NAN;
  if (lane != 0) return;
  Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double* u0 = u_init + (size_t)i * 2 * N;
  double s0[NS];
  for (int j = 0; j < NS; ++j) s0[j] = 0.0;
  const Eval e = nlp_eval<NX>(p, ell0, P, sp, i, u0, u0, 0.0, s0, P.s + (size_t)i * NS, P.u + (size_t)i * 2 * N, P.x + (size_t)i * NX * N);
  P.J[i] = e.J; P.viol[i] = e.viol1; P.vmax[i] = e.vmax; P.fval[i] = e.J; P.rho[i] = P.rho0;
  P.status[i] = SQP_RUNNING; P.sweeps[i] = 0;
  if (P.hard_viol) P.hard_viol[i] = e.vmax;
  if (P.step_norm) P.step_norm[i] = NAN;
  if (P.qp_iter) P.qp_iter[i] = 0;
}

// Index list of the running instances, in batch order (one workgroup; the host reads `count` once per sweep).
__global__ __launch_bounds__(1024) void sqp_compact_kernel(const int* status, int B, int* idx, int* count) {
  __shared__ int cnt[1024];
  const int t = threadIdx.x, chunk = (B + 1023) / 1024, lo = t * chunk, hi = min(B, lo + chunk);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += status[i] == SQP_RUNNING;
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int j = 0; j < 1024; ++j) { const int v = cnt[j]; cnt[j] = s; s += v; }
    count[0] = s;
  }
  __syncthreads();
  int o = cnt[t];
  for (int i = lo; i < hi; ++i) if (status[i] == SQP_RUNNING) idx[o++] = i;
}

__global__ __launch_bounds__(64) void sqp_gather_kernel(SqpParams P, const int* idx, double* gx0, double* gxref, double* gu, double* xinit, int nV) {
  const int b = blockIdx.x, i = idx[b], lane = threadIdx.x, nx = P.nx, N = P.N, R = nx * N, ns = nV - 2 * N;
  for (int j = lane; j < nx; j += 64) gx0[(size_t)b * nx + j] = P.x0[(size_t)i * nx + j];
  for (int j = lane; j < R; j += 64) gxref[(size_t)b * R + j] = P.x_ref[(size_t)i * R + j];
  for (int j = lane; j < 2 * N; j += 64) gu[(size_t)b * 2 * N + j] = P.u[(size_t)i * 2 * N + j];
  if (xinit) {
    for (int j = lane; j < 2 * N; j += 64) xinit[(size_t)b * nV + j] = P.u[(size_t)i * 2 * N + j];
    for (int j = lane; j < ns; j += 64) xinit[(size_t)b * nV + 2 * N + j] = P.s[(size_t)i * ns + j];
  }
}

// PAR = RtPar: pa.idx is idx, so the constants are those of instance i (one wavefront per instance: loaded once, uniform)
template <int NX, class PAR> __global__ __launch_bounds__(64) void sqp_linesearch_kernel(SqpParams P, const int* idx, int sweep, const double* z,
                                                                            const double* fval_qp, const double* qconst, const int* flag,
                                                                            const int* iter, const double* lambda, typename PAR::Args pa) {
  constexpr int NS = NX == 5 ? 1 : 4;
  const int b = blockIdx.x, i = idx[b], lane = threadIdx.x, N = P.N;
  const PAR p = par_get<PAR>(pa, b);
  __shared__ double ell0[PAR::RT ? 48 : 1];
  sqp_ellipse<NX>(p, lane, ell0);
  const int nV = 2 * N + NS, nC = (NX == 5 ? 6 : 20) * N;
  const double* zb = z + (size_t)b * nV;
  double* u = P.u + (size_t)i * 2 * N;
  double* s = P.s + (size_t)i * NS;
  const double* lam = lambda + (size_t)b * (nV + nC);
  double dn = 0, un = 0, lm = 0;
  for (int j = lane; j < 2 * N; j += 64) {
    dn = fmax(dn, fabs(zb[j] - u[j]));
    un = fmax(un, fabs(u[j]));
    lm = fmax(lm, fabs(lam[nV + j]));     // rows 0 .. 2N-1: the hard rows (v_k >= 0, |delta_k| <= 0.4)
  }
  if (P.lambda_out) for (int j = lane; j < nV + nC; j += 64) P.lambda_out[(size_t)i * (nV + nC) + j] = lam[j];
  dn = wave_max(dn); un = wave_max(un); lm = wave_max(lm);
  const int fl = flag[b];
  const double rho = fmax(P.rho[i], 1.1 * lm + 1e-6);
  const double phi0 = P.J[i] + rho * P.viol[i];
  const double pred = fmax(P.J[i] - (fval_qp[b] + qconst[b]) + rho * P.viol[i], 0.0);
  Spl sp{P.spM, P.spdl, P.xP, P.yP};
  bool ok = false;
  Eval e{0, 0, 0};
  double st[NS];
  const double alpha = ldexp(1.0, -lane);
  if (fl == 0 && lane < P.trials) {
    double strial[NS];
    for (int j = 0; j < NS; ++j) strial[j] = s[j] + alpha * (zb[2 * N + j] - s[j]);
    e = nlp_eval<NX>(p, ell0, P, sp, i, u, zb, alpha, strial, st, nullptr, nullptr);
    ok = e.J + rho * e.viol1 <= phi0 - P.armijo * alpha * pred;   // false for a NaN trial
  }
  const unsigned long long acc = __ballot(ok);
  const int win = acc ? __ffsll(acc) - 1 : -1;    // lowest lane = largest step
  const bool small = dn <= P.tol_step * (1.0 + un);
  if (lane == win) {   // the winner writes the accepted iterate (the same arithmetic as its trial)
    double strial[NS];
    for (int j = 0; j < NS; ++j) strial[j] = s[j] + alpha * (zb[2 * N + j] - s[j]);
    e = nlp_eval<NX>(p, ell0, P, sp, i, u, zb, alpha, strial, s, u, P.x + (size_t)i * NX * N);
    P.J[i] = e.J; P.viol[i] = e.viol1; P.vmax[i] = e.vmax; P.fval[i] = e.J;
    if (P.hard_viol) P.hard_viol[i] = e.vmax;
  }
  if (lane == 0) {
    P.sweeps[i] = sweep + 1;
    if (P.qp_iter) P.qp_iter[i] += iter[b];
    if (P.step_norm) P.step_norm[i] = dn;
    P.rho[i] = rho;
  }
  __syncthreads();
  if (lane != 0) return;
  int status;
  if (fl != 0) status = fl == -2 ? -2 : -1;
  else {
    const bool done = small && P.vmax[i] <= P.tol_feas;
    if (win >= 0) status = done ? 0 : SQP_RUNNING;
    else status = done ? 0 : 2;   // no step accepted, but a negligible QP step at a feasible point: stationary there
  }
  if (status == SQP_RUNNING && sweep + 1 >= P.max_sweeps) status = 1;
  P.status[i] = status;
  if (P.merit) P.merit[(size_t)i * P.max_sweeps + sweep] = P.J[i] + rho * P.viol[i];
}

}  // namespace

hipError_t sqp_init_launch(const SqpParams& P, const double* u_init, hipStream_t st, const double* par, int par_stride) {
  if (par) {
    const ParArgs pa{par, par_stride, nullptr};
    if (P.nx == 5) hipLaunchKernelGGL((sqp_init_kernel<5, RtPar>), dim3(P.B), dim3(64), 0, st, P, u_init, pa);
    else hipLaunchKernelGGL((sqp_init_kernel<7, RtPar>), dim3(P.B), dim3(64), 0, st, P, u_init, pa);
  } else {
    if (P.nx == 5) hipLaunchKernelGGL((sqp_init_kernel<5, FixedPar>), dim3(P.B), dim3(64), 0, st, P, u_init, NoParArgs{});
    else hipLaunchKernelGGL((sqp_init_kernel<7, FixedPar>), dim3(P.B), dim3(64), 0, st, P, u_init, NoParArgs{});
  }
  return hipGetLastError();
}

hipError_t sqp_compact_launch(const int* status, int B, int* idx, int* count, hipStream_t st) {
  hipLaunchKernelGGL(sqp_compact_kernel, dim3(1), dim3(1024), 0, st, status, B, idx, count);
  return hipGetLastError();
}

hipError_t sqp_gather_launch(const SqpParams& P, const int* idx, int cnt, double* gx0, double* gxref, double* gu, double* xinit, int nV,
                             hipStream_t st) {
  hipLaunchKernelGGL(sqp_gather_kernel, dim3(cnt), dim3(64), 0, st, P, idx, gx0, gxref, gu, xinit, nV);
  return hipGetLastError();
}

hipError_t sqp_linesearch_launch(const SqpParams& P, const int* idx, int cnt, int sweep, const double* z, const double* fval_qp,
                                 const double* qconst, const int* flag, const int* iter, const double* lambda, hipStream_t st,
                                 const double* par, int par_stride) {
  if (par) {
    const ParArgs pa{par, par_stride, idx};
    if (P.nx == 5) hipLaunchKernelGGL((sqp_linesearch_kernel<5, RtPar>), dim3(cnt), dim3(64), 0, st, P, idx, sweep, z, fval_qp, qconst, flag, iter, lambda, pa);
    else hipLaunchKernelGGL((sqp_linesearch_kernel<7, RtPar>), dim3(cnt), dim3(64), 0, st, P, idx, sweep, z, fval_qp, qconst, flag, iter, lambda, pa);
  } else {
    const NoParArgs pa{};
    if (P.nx == 5) hipLaunchKernelGGL((sqp_linesearch_kernel<5, FixedPar>), dim3(cnt), dim3(64), 0, st, P, idx, sweep, z, fval_qp, qconst, flag, iter, lambda, pa);
    else hipLaunchKernelGGL((sqp_linesearch_kernel<7, FixedPar>), dim3(cnt), dim3(64), 0, st, P, idx, sweep, z, fval_qp, qconst, flag, iter, lambda, pa);
  }
  return hipGetLastError();
}
