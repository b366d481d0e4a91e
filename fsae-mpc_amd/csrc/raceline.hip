// raceline.hip -- the minimum-curvature racing line of the s-domain plans, batched on the device.
//
//   raceline_qp_kernel        H and g of the line QP (min summed squared second difference of the line's points over the control
//                             points of the lateral offset).  They depend on the track, N_s and N_c only: one workgroup, one lane
//                             per control point, each summing its band row over the cells that touch it in ascending cell order
//                             (no atomics: the same bits on every run).  The band sits in LDS; every lane then writes its row of
//                             the dense H, zeros included, upper and lower triangle from the same band entry.
//   raceline_bounds_kernel    per plan: lb = -w_p, ub = +w_p (w_p = N_MAX_p - margin) and the plan's copy of g (the solver reads
//                             g per instance)
//   plan_profile_kernel       <DYN, PAR, LINE = true> of plan_profile_kernel.h: the speed profile on a line (offset, heading offset,
//                             length and curvature of every cell from the control points, the cell's own length in the recurrences
//                             and rows), instantiated and launched here
// The solve between them is the library's own (qp_solve_launch through fsaempc_qp_solve_batch_device_s: nC = 0, shared H).
#include <hip/hip_runtime.h>
#include <math.h>
#include "raceline.h"
#include "mpc_params.h"
#include "cl_frame.h"   // (compiled as in planner.hip: the pragma below comes after it)
#include "plan_profile_kernel.h"

// plain IEEE operations in source order (no FMA contraction): restated operation for operation in tests/raceline_numpy.py
#pragma clang fp contract(off)

namespace {

struct TrackFrame {   // centre point and unit left normal at s_i = i ds (curvilinear_to_cartesian.m:16-23)
  Spl sp; double ds;
  DEVINL RlFrame operator()(int i) const {
    const double s = (double)i * ds;
    double X, Xd, Xdd, Y, Yd, Ydd;
    spline3(sp.xP, sp.M, sp.dl, s, X, Xd, Xdd);
    spline3(sp.yP, sp.M, sp.dl, s, Y, Yd, Ydd);
    const double tx = -Yd, ty = Xd;
    const double nrm = sqrt(tx * tx + ty * ty);
    return RlFrame{X, Y, tx / nrm, ty / nrm};
  }
};

__global__ void __launch_bounds__(256) raceline_qp_kernel(RacelineQpParams P) {
  extern __shared__ double lds[];   // the band: N_c x RL_BAND
  const int j = threadIdx.x, Nc = P.N_c;
  if (j < Nc) {
    const TrackFrame frame{Spl{P.spM, P.spdl, P.xP, P.yP}, P.ds};
    double band[RL_BAND], gj;
    rl_row(frame, j, P.N_s, Nc, P.ds, band, gj);
#pragma unroll
    for (int c = 0; c < RL_BAND; ++c) lds[j * RL_BAND + c] = band[c];
    P.g[j] = gj;
  }
  __syncthreads();
  if (j < Nc)
    for (int k = 0; k < Nc; ++k) P.H[(size_t)k * Nc + j] = rl_H_entry(lds, j, k, Nc);   // (column k, row j: lanes write neighbouring addresses)
}

template <class PAR> __global__ void __launch_bounds__(64) raceline_bounds_kernel(RacelineBoundsParams P, typename PAR::Args pa) {
  const int plan = blockIdx.x, Nc = P.N_c;
  const PAR p = par_get<PAR>(pa, plan);
  double w = p.N_MAX - P.margin;
  if (p.bad || !(w > 0.0) || !(w < INFINITY)) w = 1.0;   // (no usable width: any box will do, the profile kernel makes this plan NaN)
  for (int j = threadIdx.x; j < Nc; j += 64) {
    P.lb[(size_t)plan * Nc + j] = -w;
    P.ub[(size_t)plan * Nc + j] = w;
    if (plan > 0) P.g[(size_t)plan * Nc + j] = P.g[j];
  }
}

}  // namespace

hipError_t raceline_qp_launch(const RacelineQpParams& P, hipStream_t st) {
  hipLaunchKernelGGL(raceline_qp_kernel, dim3(1), dim3(256), sizeof(double) * (size_t)P.N_c * RL_BAND, st, P);
  return hipGetLastError();
}
hipError_t raceline_bounds_launch(const RacelineBoundsParams& P, const double* par, int par_stride, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  if (par) hipLaunchKernelGGL((raceline_bounds_kernel<RtPar>), dim3(P.n_plans), dim3(64), 0, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((raceline_bounds_kernel<FixedPar>), dim3(P.n_plans), dim3(64), 0, st, P, NoParArgs{});
  return hipGetLastError();
}
hipError_t plan_line_profile_launch(const PlanLineParams& P, const double* par, int par_stride, hipStream_t st) {
  return plan_profile_kernel_launch<true>(P, sizeof(double) * ((size_t)3 * (size_t)P.N_s + (size_t)P.N_c), par, par_stride, st);
}
