// corridor.hip -- s-varying track corridors: every place that knew the track's width as the one number N_MAX, with
// the width read from a table over arc length instead (corridor.h).  No kernel of the other units changes: these run beside them.
//
//   cor_rows_kernel         after the LTV build (plain or blocked): the 2N track-row bounds of every instance, one thread per
//                           (instance, step), from the corridor at the row's own linearisation point and the build's pred
//   cor_metrics_kernel      cl_metrics_kernel (plant.hip, the same text) with the track violation taken against the corridor
//   cor_line_bounds_kernel  raceline_bounds_kernel (raceline.hip) with the box of every control point from the corridor's cells; a
//                           control point without a box gets NaN bounds, which the solve answers with flag -1 before its first iteration
//   cor_line_void_kernel    after the line solve: NaN control points for every plan whose QP did not end with flag 0
//   cor_line_rows_kernel    the cell-wise form of the line's corridor: the one matrix of the cells' offsets in the control points,
//                           the bounds of its rows per plan from the corridor, free control points and the plan's copy of g
//   cor_line_lambda_kernel  the cell rows' multipliers out of the solver's lambda
#include <hip/hip_runtime.h>
#include <math.h>
#include "fsaempc.h"
#include "corridor.h"
#include "raceline.h"
#include "mpc_params.h"

namespace {

__global__ void __launch_bounds__(256) cor_rows_kernel(CorRowsParams P) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)P.batch * P.N) return;
  const int b = (int)(t / P.N), k = (int)(t % P.N), N = P.N;
  const size_t at = ((size_t)b * N + k) * P.nx;
  const double s = P.x_lin[at], pn = P.pred[at + 1];
  double lo, hi;
  cor_lookup(P.cor, b, s, lo, hi);
  P.lbA[(size_t)b * P.nC + 2 * N + k] = lo - pn;
  P.ubA[(size_t)b * P.nC + 3 * N + k] = hi - pn;
}

// cl_metrics_kernel of plant.hip (the same text: that kernel is not to change) but for the track violation
template <class PAR> __global__ void cor_metrics_kernel(ClMetricsParams P, CorTable cor, typename PAR::Args pa) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  PAR p;
  if constexpr (PAR::RT) {
    p = par_load(pa.values + (size_t)b * (size_t)pa.stride);
    if (p.bad) return;
  }
  double* m = P.metrics + (size_t)b * FSAEMPC_NMETRIC;
  if (m[FSAEMPC_M_STATUS] != 0.0) return;                     // latched: later steps touch nothing
  const int fin = P.finished[b];
  if (fin == 2) { m[FSAEMPC_M_STATUS] = 2.0; return; }        // lost: x0 is a placeholder
  const double s = P.x0[(size_t)b * P.nx], n = P.x0[(size_t)b * P.nx + 1], an = fabs(n);
  if (an > m[FSAEMPC_M_N_ABS_MAX]) m[FSAEMPC_M_N_ABS_MAX] = an;                 // main.m:101: n_list(i) precedes the lap check
  double lo, hi;
  cor_lookup(cor, b, s, lo, hi);
  const double v = fmax(n - hi, lo - n);                                         // (NaN limits: no violation is recorded)
  if (v > 0.0) {                                                                // main.m:204-205 against the edges at s
    m[FSAEMPC_M_N_VIOL_INT] += v * P.dt;
    if (v > m[FSAEMPC_M_N_VIOL_MAX]) m[FSAEMPC_M_N_VIOL_MAX] = v;
  }
  if (fin != 0) { m[FSAEMPC_M_STATUS] = 1.0; return; }        // main.m:102-104: the break; i - 1 steps were solved
  if (m[FSAEMPC_M_STEPS] == 0.0) m[FSAEMPC_M_S_START] = s;
  m[FSAEMPC_M_S_LAST] = s;
  m[FSAEMPC_M_STEPS] += 1.0;
  const int ef = P.exitflag[b];
  if (ef != 0) m[FSAEMPC_M_ABNORMAL] += 1.0;                                    // main.m:209
  const double it = (double)P.iter[b];
  m[FSAEMPC_M_ITER_SUM] += it;
  if (it > m[FSAEMPC_M_ITER_MAX]) m[FSAEMPC_M_ITER_MAX] = it;
  const bool use_n = P.slack[(size_t)b * P.ns] > P.slack_tol;                   // main.m:132-133 (NaN: not in use)
  const bool use_t = P.slack[(size_t)b * P.ns + P.tyre] > P.slack_tol;
  if (use_n) m[FSAEMPC_M_SLACK_N_CNT] += 1.0;
  if (use_t) m[FSAEMPC_M_SLACK_TYRE_CNT] += 1.0;
  if (ef == 0 && !use_n && !use_t) { m[FSAEMPC_M_OBJ_SUM] += P.fval[b]; m[FSAEMPC_M_OBJ_CNT] += 1.0; }   // main.m:198, 210
  // main.m:180-182, 199: rear lateral force of f_curv_dyn.m:32-53 at the post-plant state, acceleration of the driven plan
  const double* c = P.cart + (size_t)b * 7;
  const double x_d = c[3], y_d = c[4], theta_d = c[5];
  const double x_d_hat = x_d + 5 * exp(-x_d / 5);
  const double alpha_r = -atan((y_d - p.LR * theta_d) / x_d_hat);
  const double B = p.PB, C = p.PC, D = p.PD, E = p.PE;
  const double Fcr = p.FZR * D * sin(C * atan(B * alpha_r - E * (B * alpha_r - atan(B * alpha_r))));
  const double a = P.u_drive[(size_t)b * 2 * P.N];
  const double el = Fcr / (p.M * p.ELL_LAT), ea = a / p.ELL_LONG;
  const double e = el * el + ea * ea;
  if (e > 1.0) {                                                                // main.m:212-213
    m[FSAEMPC_M_ELL_VIOL_INT] += (e - 1.0) * P.dt;
    if (e - 1.0 > m[FSAEMPC_M_ELL_VIOL_MAX]) m[FSAEMPC_M_ELL_VIOL_MAX] = e - 1.0;
  }
}

// The box of control point j of `plan`: the tightest limits over the cells of the four knot spans whose basis touches c_j.  Span jj
// holds the cells i with floor(i N_c / N_s) == jj: ceil(jj N_s / N_c) .. ceil((jj + 1) N_s / N_c) - 1 (never empty: N_s >= 2 N_c).
// A NaN limit in any of them makes both bounds NaN.
__device__ __forceinline__ void cor_cp_box(const CorLineParams& P, int plan, int j, double& lb, double& ub) {
#pragma clang fp contract(off)
  const int Ns = P.N_s, Nc = P.N_c;
  bool nan = false;
  lb = -INFINITY; ub = INFINITY;
  for (int d = -2; d <= 1; ++d) {
    int jj = j + d;
    if (jj < 0) jj += Nc;
    if (jj >= Nc) jj -= Nc;
    const int i0 = (int)(((long long)jj * Ns + Nc - 1) / Nc), i1 = (int)(((long long)(jj + 1) * Ns + Nc - 1) / Nc);
    for (int i = i0; i < i1; ++i) {
      const double s = (double)i * P.L / (double)Ns;
      double lo, hi;
      cor_lookup(P.cor, plan, s, lo, hi);
      const double l = lo + P.margin, h = hi - P.margin;
      nan = nan || !(l == l) || !(h == h);
      lb = fmax(lb, l); ub = fmin(ub, h);
    }
  }
  if (nan) { lb = NAN; ub = NAN; }
}

__global__ void __launch_bounds__(64) cor_line_bounds_kernel(CorLineParams P) {
  const int plan = blockIdx.x, Nc = P.N_c;
  for (int j = threadIdx.x; j < Nc; j += 64) {
    double lb, ub;
    cor_cp_box(P, plan, j, lb, ub);
    if (!(lb < ub)) { lb = NAN; ub = NAN; }   // (no box: the QP of this plan has non-finite data and is not solved)
    P.lb[(size_t)plan * Nc + j] = lb;
    P.ub[(size_t)plan * Nc + j] = ub;
    if (P.g && plan > 0) P.g[(size_t)plan * Nc + j] = P.g[j];
  }
}

__global__ void __launch_bounds__(64) cor_line_void_kernel(CorLineParams P) {
  const int plan = blockIdx.x, Nc = P.N_c;
  if (P.flag[plan] == 0) return;   // (uniform over the workgroup)
  for (int j = threadIdx.x; j < Nc; j += 64) P.line[(size_t)plan * Nc + j] = NAN;
}

// The grid is nA = ceil(N_s N_c / 256) workgroups for the matrix, then nP = ceil((N_s + N_c) / 256) workgroups per plan.
//   matrix   element e = k N_s + i of the column-major A: consecutive lanes are consecutive cells i of one column k, so a wavefront
//            stores 512 contiguous bytes.  The cell's four columns are distinct (N_c >= 8); every other entry is written as 0.
//   plan p   item r < N_s: the bounds of row r; item N_s + j: the free box of control point j and the plan's copy of g_j
__global__ void __launch_bounds__(256) cor_line_rows_kernel(CorLineRowsParams P, int nA, int nP) {
#pragma clang fp contract(off)
  const int Ns = P.N_s, Nc = P.N_c;
  if ((int)blockIdx.x < nA) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)Ns * Nc) return;
    const int k = (int)(e / Ns), i = (int)(e % Ns);
    int col0; double w[4];
    rl_offset_row(i, Ns, Nc, col0, w);
    int m = k - col0;
    if (m < 0) m += Nc;
    P.A[e] = m < 4 ? rl_pick<4>(w, m) : 0.0;
    return;
  }
  const int rel = (int)blockIdx.x - nA, plan = rel / nP, r = (rel % nP) * 256 + (int)threadIdx.x;
  if (r < Ns) {
    const double s = (double)r * P.L / (double)Ns;
    double lo, hi;
    cor_lookup(P.cor, plan, s, lo, hi);
    double l = lo + P.margin, h = hi - P.margin;
    if (!(l < h)) { l = NAN; h = NAN; }   // (a NaN lookup included: the QP of this plan has non-finite data and is not solved)
    P.lbA[(size_t)plan * Ns + r] = l;
    P.ubA[(size_t)plan * Ns + r] = h;
  } else if (r < Ns + Nc && P.lb) {
    const int j = r - Ns;
    P.lb[(size_t)plan * Nc + j] = -1e10;
    P.ub[(size_t)plan * Nc + j] = 1e10;
    if (plan > 0) P.g[(size_t)plan * Nc + j] = P.g[j];
  }
}

__global__ void __launch_bounds__(256) cor_line_lambda_kernel(const double* lambda, double* row_lambda, int n_plans, int Ns, int Nc) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n_plans * Ns) return;
  const long long p = t / Ns, i = t % Ns;
  row_lambda[t] = lambda[p * (Nc + Ns) + Nc + i];
}

}  // namespace

hipError_t cor_line_rows_launch(const CorLineRowsParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  const int nA = (int)(((long long)P.N_s * P.N_c + 255) / 256), nP = (P.N_s + P.N_c + 255) / 256;
  hipLaunchKernelGGL(cor_line_rows_kernel, dim3((unsigned)(nA + (long long)P.n_plans * nP)), dim3(256), 0, st, P, nA, nP);
  return hipGetLastError();
}
hipError_t cor_line_lambda_launch(const double* lambda, double* row_lambda, int n_plans, int N_s, int N_c, hipStream_t st) {
  if (n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(cor_line_lambda_kernel, dim3((unsigned)(((long long)n_plans * N_s + 255) / 256)), dim3(256), 0, st, lambda, row_lambda, n_plans, N_s, N_c);
  return hipGetLastError();
}

hipError_t cor_rows_launch(const CorRowsParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  const long long rows = (long long)P.batch * P.N;
  hipLaunchKernelGGL(cor_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, P);
  return hipGetLastError();
}
hipError_t cor_metrics_launch(const ClMetricsParams& P, const CorTable& cor, hipStream_t st, const double* par, int par_stride) {
  if (P.batch == 0) return hipSuccess;
  if (par) hipLaunchKernelGGL(cor_metrics_kernel<RtPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, cor, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL(cor_metrics_kernel<FixedPar>, dim3((P.batch + 63) / 64), dim3(64), 0, st, P, cor, NoParArgs{});
  return hipGetLastError();
}
hipError_t cor_line_bounds_launch(const CorLineParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(cor_line_bounds_kernel, dim3(P.n_plans), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t cor_line_void_launch(const CorLineParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(cor_line_void_kernel, dim3(P.n_plans), dim3(64), 0, st, P);
  return hipGetLastError();
}
