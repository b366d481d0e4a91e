// plan_profile_kernel.h -- the body of the plan kernel, written once for the centre line and for a racing line, out of the phases of
// plan_profile.h.  Included by planner.hip (LINE = false) and by raceline.hip (LINE = true, 6j).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "planner.h"
#include "raceline.h"
#include "plan_profile.h"
#include "mpc_params.h"

namespace {

// A quasi-steady-state minimum-time speed profile, the stand-in for the table dynamic_minimum_time_planner.m produces (main.m:20; the
// planner itself needs IPOPT): curvature and length of every cell, the grip-limited corner speed, the two passes of pp_passes, then
// the 8 planner values and the traversal time of each cell.  One wavefront per plan: the cells are dealt to the lanes for the
// parallel phases, curvature and speed sit in LDS, lane 0 runs the two recurrences.
// LINE = false: the centre line.  No control points, every cell has the length ds, n = mu = 0; LDS: 16 N_s bytes.
// LINE = true: the line of the plan's control points (the centre line for a plan whose flag is set): offset, heading offset, length
// and curvature of every cell from them, the cells' own lengths in the passes and rows; LDS: 24 N_s + 8 N_c bytes.
// Every cross-lane operation and barrier is met by all 64 lanes; a plan that is NaN leaves as one (uniform over the wave).
template <bool DYN, class PAR, bool LINE> __global__ void __launch_bounds__(64)
plan_profile_kernel(std::conditional_t<LINE, PlanLineParams, PlanProfileParams> P, typename PAR::Args pa) {
#pragma clang fp contract(off)
  extern __shared__ double lds[];
  const int plan = blockIdx.x, lane = threadIdx.x, Ns = P.N_s;
  const int per = (Ns + 63) / 64;   // cells per lane
  double* kq = lds;              // Ns: curvature of the centre line, then (LINE) of the line
  double* vq = lds + Ns;         // Ns: (LINE: heading offset, then) speed
  double* dq = lds + 2 * Ns;     // LINE, Ns: |dp/ds|, then the cell's length on the line
  double* cq = lds + 3 * Ns;     // LINE, Nc: control points
  double* tab = P.table + (size_t)plan * Ns * 8;
  double* tt = P.t + (size_t)plan * Ns;
  const PAR p = par_get<PAR>(pa, plan);
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double ds = P.ds, grip = P.grip;
  bool nan_plan = p.bad;   // a block that cannot describe a car
  int Nc = 0; double* lout = nullptr;
  if constexpr (LINE) {
    Nc = P.N_c;
    if (P.line_out) lout = P.line_out + (size_t)plan * Nc;
    const bool flagged = P.flag && P.flag[plan] != 0;   // the QP of this plan was not solved: the centre line
    nan_plan = nan_plan || (P.check_width && !(p.N_MAX - P.margin > 0.0));
    if (!nan_plan) {
      pp_load_points(cq, P.line + (size_t)plan * P.line_stride, Nc, lane, flagged, nullptr, nullptr, nullptr);
      __syncthreads();
      nan_plan = pp_line_geometry(sp, cq, Ns, Nc, ds, P.h, lane, per, kq, vq, dq);
    }
  }
  if (nan_plan) {
    pp_nan_table(tab, tt, Ns, lane);
    if (lout) for (int j = lane; j < Nc; j += 64) lout[j] = NAN;
    return;
  }
  if constexpr (LINE) {
    if (lout) for (int j = lane; j < Nc; j += 64) lout[j] = cq[j];
    __syncthreads();
    pp_line_curvature(kq, vq, dq, Ns, ds, lane, per);
    __syncthreads();
  }

  const double A_lat = grip * (DYN ? p.ELL_LAT : p.ALAT_MAX);
  double best; int ibest;
  pp_corner_phase<!LINE>(sp, ds, kq, vq, Ns, lane, A_lat, P.v_cap, best, ibest);
  const int i0 = pp_wave_first_min(best, ibest, Ns);
  __syncthreads();

  if (lane == 0) {
    const MlCar car{p.U_ACC_MAX, p.ELL_LONG};
    if constexpr (LINE) pp_passes<DYN>(car, Ns, i0, A_lat, grip, kq, (const double*)dq, vq, PpNoRecord{});
    else pp_passes<DYN>(car, Ns, i0, A_lat, grip, kq, PpConstLen{ds}, vq, PpNoRecord{});
  }
  __syncthreads();

  for (int i = lane; i < Ns; i += 64) {
    if constexpr (LINE) {
      const RlPoint q = rl_point(cq, i, Ns, Nc, P.h, kappa(sp, (double)i * ds));
      pp_table_row(p.WB, i, Ns, kq, vq, dq[i], q.n, q.mu, tab, tt);
    } else {
      pp_table_row(p.WB, i, Ns, kq, vq, ds, 0.0, 0.0, tab, tt);
    }
  }
}

// P.dynamic and a parameter block or none select the instantiation.  par: plan p reads par + p * par_stride; null: the constants compiled in
template <bool LINE, class PARAMS> hipError_t plan_profile_kernel_launch(const PARAMS& P, size_t lds, const double* par, int par_stride, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  const dim3 grid(P.n_plans), wave(64);
  const ParArgs pa{par, par_stride, nullptr};
  if (P.dynamic) {
    if (par) hipLaunchKernelGGL((plan_profile_kernel<true, RtPar, LINE>), grid, wave, lds, st, P, pa);
    else hipLaunchKernelGGL((plan_profile_kernel<true, FixedPar, LINE>), grid, wave, lds, st, P, NoParArgs{});
  } else {
    if (par) hipLaunchKernelGGL((plan_profile_kernel<false, RtPar, LINE>), grid, wave, lds, st, P, pa);
    else hipLaunchKernelGGL((plan_profile_kernel<false, FixedPar, LINE>), grid, wave, lds, st, P, NoParArgs{});
  }
  return hipGetLastError();
}

}  // namespace
