// minlap.hip -- the minimum-time racing line of the s-domain plans, batched on the device.
//
//   plan_line_lapgrad_kernel   lap time T(c) of the profile on a line and dT/dc by the adjoint of that profile: up to and including
//                              the two passes the phases of plan_profile.h that plan_profile_kernel<.., LINE = true> (raceline.hip)
//                              runs, with the passes recorded (PpRecord), then the adjoint half of minlap.h.  One wavefront per
//                              line, cells dealt to the lanes for the parallel phases,
//                              the four serial chains (two passes, two passes undone) run by lane 0 out of LDS between barriers, the
//                              gradient gathered per control point over its cells in ascending order (no atomics: the same bits on
//                              every call).  A wave may run on clamp(base + step, lo, hi) (the candidates of one iteration).
//   minlap_candidates_kernel   per plan and rho_j: g = grad / rho_j and the box of the step, lb = lo - c, ub = hi - c
//   minlap_select_kernel       per plan: the best solved candidate replaces the incumbent if its lap is strictly shorter
//   minlap_box_kernel          a user's boxes as the bounds of the initial line QP
// The solves between them are the library's own (fsaempc_qp_solve_batch_device_s: nC = 0, one shared H, the H of the line QP).
#include <hip/hip_runtime.h>
#include <math.h>
#include "minlap.h"
#include "mpc_params.h"
#include "cl_frame.h"   // (compiled as in raceline.hip: the pragma below comes after it, so kappa() has that unit's arithmetic)

// plain IEEE operations in source order (no FMA contraction): restated operation for operation in tests/minlap_numpy.py
#pragma clang fp contract(off)

namespace {

template <bool DYN, class PAR> __global__ void __launch_bounds__(64) plan_line_lapgrad_kernel(MinlapGradParams P, typename PAR::Args pa) {
  extern __shared__ double lds[];
  const int wave = blockIdx.x, plan = wave / P.cand, lane = threadIdx.x, Ns = P.N_s, Nc = P.N_c;
  const int per = (Ns + 63) / 64;   // cells per lane: the loops over cells below run `per` times on every lane
  double* kq = lds;                 // Ns: curvature of the centre line, then of the line; after the chains a
  double* mq = lds + Ns;            // Ns: heading offset
  double* dq = lds + 2 * Ns;        // Ns: |dp/ds|, then the cell's length on the line; after the chains kappa
  double* vq = lds + 3 * Ns;        // Ns: corner speed, then speed; after the chains n'
  double* vf = lds + 4 * Ns;        // Ns: speed after the forward pass; at the end the adjoint of n' over h
  double* vb = lds + 5 * Ns;        // Ns: adjoint of the speed; at the end the adjoint of n
  double* Kb = lds + 6 * Ns;        // Ns: adjoint of K, then of m
  double* db = lds + 7 * Ns;        // Ns: adjoint of the length, then of r
  double* cq = lds + 8 * Ns;        // Nc: control points
  int* won = (int*)(lds + 8 * Ns + Nc);   // Ns: ML_WON_* per cell
  double* gout = P.grad + (size_t)wave * Nc;
  double* lout = P.line_out ? P.line_out + (size_t)wave * Nc : nullptr;
  const PAR p = par_get<PAR>(pa, plan);
  bool nan_plan = p.bad || (P.check_width && !(p.N_MAX - P.margin > 0.0));   // (uniform over the wave)
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double ds = P.ds, grip = P.grip;

  if (!nan_plan) {
    const size_t o = (size_t)plan * Nc;
    pp_load_points(cq, P.line + (size_t)wave * P.line_stride, Nc, lane, false, P.base ? P.base + o : nullptr, P.lo + o, P.hi + o);
    __syncthreads();
    nan_plan = pp_line_geometry(sp, cq, Ns, Nc, ds, P.h, lane, per, kq, mq, dq);
  }
  if (nan_plan) {   // (uniform over the wave) this line is NaN, the others are unaffected
    for (int j = lane; j < Nc; j += 64) {
      gout[j] = NAN;
      if (lout) lout[j] = NAN;
    }
    if (lane == 0) P.T[(size_t)wave * P.T_stride] = NAN;
    return;
  }
  if (lout) for (int j = lane; j < Nc; j += 64) lout[j] = cq[j];
  __syncthreads();
  pp_line_curvature(kq, mq, dq, Ns, ds, lane, per);
  __syncthreads();

  const double A_lat = grip * (DYN ? p.ELL_LAT : p.ALAT_MAX);
  const MlCar car{p.U_ACC_MAX, p.ELL_LONG};
  double best; int ibest;
  pp_corner_phase<false>(sp, ds, kq, vq, Ns, lane, A_lat, P.v_cap, best, ibest);
  const int i0 = pp_wave_first_min(best, ibest, Ns);   // (best: vlat[i0], the source of the first forward step)
  __syncthreads();

  if (lane == 0) pp_passes<DYN>(car, Ns, i0, A_lat, grip, kq, (const double*)dq, vq, PpRecord{vf, won});
  __syncthreads();

  // T = sum dl / v: each lane sums its cells in ascending order, then the wave; the seeds of the reverse sweep
  double tsum = 0.0;
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const double dl = dq[i], v = vq[i];
      tsum += dl / v;
      double vbar, dlbar;
      ml_cell_seed(dl, v, vbar, dlbar);
      vb[i] = vbar; db[i] = dlbar; Kb[i] = 0.0;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) tsum += __shfl_xor(tsum, m, 64);   // (the same value on every lane: both operands of each add are swapped copies)
  __syncthreads();

  if (lane == 0) ml_reverse<DYN>(car, Ns, i0, A_lat, grip, best, kq, dq, vq, vf, won, vb, Kb, db);
  __syncthreads();

  // per cell: the adjoints of m and r; a, n' and kappa are kept for the next phase (own cell only)
  for (int it = 0; it < per; ++it) {
    const int i = lane + 64 * it;
    if (i < Ns) {
      const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
      const double kbar = ml_cell_kbar(A_lat, P.v_cap, kq[i], vb[i], Kb[i]);
      const double k = kappa(sp, (double)i * ds);
      const RlPoint q = rl_point(cq, i, Ns, Nc, P.h, k);
      const double m = k + (mq[nx] - mq[pr]) / (2.0 * ds);
      double mbar, rbar;
      ml_cell_mr(kbar, m, q.r, ds, db[i], mbar, rbar);
      Kb[i] = mbar; db[i] = rbar;
      kq[i] = q.a; vq[i] = q.nd; dq[i] = k;
    }
  }
  __syncthreads();

  for (int it = 0; it < per; ++it) {   // neighbours' adjoints of m read, own adjoints of n and n' written
    const int i = lane + 64 * it;
    if (i < Ns) {
      const int pr = i > 0 ? i - 1 : Ns - 1, nx = i + 1 < Ns ? i + 1 : 0;
      const double mubar = (Kb[pr] - Kb[nx]) / (2.0 * ds);
      const double a = kq[i], nd = vq[i];
      double nbar, ndbar;
      ml_cell_n(db[i], mubar, a, nd, sqrt(a * a + nd * nd), dq[i], P.h, nbar, ndbar);
      vb[i] = nbar; vf[i] = ndbar;
    }
  }
  __syncthreads();

  for (int j = lane; j < Nc; j += 64) gout[j] = ml_grad_entry(j, Ns, Nc, vb, vf);
  if (lane == 0) P.T[(size_t)wave * P.T_stride] = tsum;
}

__global__ void __launch_bounds__(64) minlap_candidates_kernel(MinlapCandParams P) {
  const int w = blockIdx.x, plan = w / P.J, Nc = P.N_c;
  const int jr = w - plan * P.J;
  double rho = P.rho[0];
#pragma unroll
  for (int q = 1; q < 16; ++q) rho = jr == q ? P.rho[q] : rho;   // (no dynamic index into the kernel's arguments)
  for (int j = threadIdx.x; j < Nc; j += 64) {
    const size_t a = (size_t)plan * Nc + j, o = (size_t)w * Nc + j;
    const double c = P.c[a];
    P.g[o] = P.grad[a] / rho;
    P.lb[o] = P.lo[a] - c;
    P.ub[o] = P.hi[a] - c;
  }
}

__global__ void __launch_bounds__(64) minlap_select_kernel(MinlapSelectParams P) {
  const int plan = blockIdx.x, Nc = P.N_c, J = P.J;
  double* hist = P.lap_hist + (size_t)plan * (P.K + 1);
  const double Tcur = hist[P.it];
  int pick = -1;
  if (fabs(Tcur) < INFINITY) {   // (uniform over the workgroup: every lane reads the same values) a NaN incumbent never moves
    double Tbest = Tcur;
    for (int j = 0; j < J; ++j) {
      const double Tj = P.Tc[(size_t)plan * J + j];
      if (P.flagc[(size_t)plan * J + j] == 0 && fabs(Tj) < INFINITY && Tj < Tbest) { Tbest = Tj; pick = j; }
    }
  }
  if (pick >= 0) {
    const size_t src = ((size_t)plan * J + pick) * Nc;
    for (int j = threadIdx.x; j < Nc; j += 64) {
      P.c[(size_t)plan * Nc + j] = P.cc[src + j];
      P.grad[(size_t)plan * Nc + j] = P.gradc[src + j];
    }
  }
  if (threadIdx.x == 0) {
    hist[P.it + 1] = pick >= 0 ? P.Tc[(size_t)plan * J + pick] : Tcur;
    P.step_hist[(size_t)plan * P.K + P.it] = pick;
  }
}

__global__ void __launch_bounds__(64) minlap_box_kernel(MinlapBoxParams P) {
  const int plan = blockIdx.x, Nc = P.N_c;
  for (int j = threadIdx.x; j < Nc; j += 64) {
    double lb = P.lo[(size_t)plan * Nc + j], ub = P.hi[(size_t)plan * Nc + j];
    if (!(lb < ub)) { lb = NAN; ub = NAN; }   // (no box: the QP of this plan has non-finite data and is not solved)
    P.lb[(size_t)plan * Nc + j] = lb;
    P.ub[(size_t)plan * Nc + j] = ub;
    if (plan > 0) P.g[(size_t)plan * Nc + j] = P.g[j];
  }
}

template <bool DYN, class PAR> hipError_t lapgrad_launch_one(const MinlapGradParams& P, const typename PAR::Args& pa, hipStream_t st) {
  const size_t lds = minlap_lapgrad_lds_bytes(P.N_s, P.N_c);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&plan_line_lapgrad_kernel<DYN, PAR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((plan_line_lapgrad_kernel<DYN, PAR>), dim3(P.n_waves), dim3(64), lds, st, P, pa);
  return hipGetLastError();
}
template <bool DYN> hipError_t lapgrad_launch(const MinlapGradParams& P, const double* par, int par_stride, hipStream_t st) {
  if (par) return lapgrad_launch_one<DYN, RtPar>(P, ParArgs{par, par_stride, nullptr}, st);
  return lapgrad_launch_one<DYN, FixedPar>(P, NoParArgs{}, st);
}

}  // namespace

size_t minlap_lapgrad_lds_bytes(int N_s, int N_c) {
  return sizeof(double) * ((size_t)8 * (size_t)N_s + (size_t)N_c) + sizeof(int) * (size_t)N_s;
}
hipError_t minlap_lapgrad_launch(const MinlapGradParams& P, const double* par, int par_stride, hipStream_t st) {
  if (P.n_waves == 0) return hipSuccess;
  return P.dynamic ? lapgrad_launch<true>(P, par, par_stride, st) : lapgrad_launch<false>(P, par, par_stride, st);
}
hipError_t minlap_candidates_launch(const MinlapCandParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(minlap_candidates_kernel, dim3(P.n_plans * P.J), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t minlap_select_launch(const MinlapSelectParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(minlap_select_kernel, dim3(P.n_plans), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t minlap_box_launch(const MinlapBoxParams& P, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  hipLaunchKernelGGL(minlap_box_kernel, dim3(P.n_plans), dim3(64), 0, st, P);
  return hipGetLastError();
}
