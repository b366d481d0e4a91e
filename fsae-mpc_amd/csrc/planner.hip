// planner.hip -- the s-domain plan the closed loop tracks, batched on the device.
//
//   plan_profile_kernel    <DYN, PAR, LINE = false> of plan_profile_kernel.h: the speed profile on the centre line (curvature of
//                          the spline table per cell, every cell of length ds), instantiated and launched here
//   plan_reference_kernel util/obtain_reference.m:5-48 in the state layout of the model, batched over s0 (one thread per car),
//                          on a plan shared by the batch or given per car
//   cl_pre_plan_kernel     cl_pre_kernel (plant.hip) with the live ramp of main.m:107-114 replaced by main.m:115: frame
//                          transform, x0 assembly, lap check, out-of-race rule, then the walk from the car's own s
#include <hip/hip_runtime.h>
#include <math.h>
#include "planner.h"
#include "mpc_params.h"
#include "cl_frame.h"   // (compiled as in plant.hip: the pragma below comes after it)
#include "plan_profile_kernel.h"

// plain IEEE operations in source order (no FMA contraction): the walk is compared bit for bit with the oracle (the profile's
// functions carry the pragma themselves)
#pragma clang fp contract(off)

namespace {

DEVINL PlanTable plan_of(const PlanTable& pl, int b) {
  PlanTable q = pl;
  if (pl.per_instance) { q.table += (size_t)b * pl.N_s * 8; q.t += (size_t)b * pl.N_s; }
  return q;
}

__global__ void plan_reference_kernel(PlanRefParams P) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  const PlanTable pl = plan_of(P.plan, b);
  plan_walk(pl.table, pl.t, pl.N_s, pl.ds, P.s0[b], P.dt, P.N, P.nx, P.x_ref + (size_t)b * P.nx * P.N);
}

__global__ void cl_pre_plan_kernel(ClPrePlanParams P) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= P.batch) return;
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const int nx = P.nx;
  double* x0 = P.x0 + (size_t)b * nx;
  cl_pre_frame(sp, nx, P.L, P.cart + (size_t)b * 7, P.s_guess[b], x0, P.finished + b);   // main.m:93-104
  const PlanTable pl = plan_of(P.plan, b);
  // main.m:115 (a car out of the race has x0 = 0: finite placeholder rows from the start of the plan)
  plan_walk(pl.table, pl.t, pl.N_s, pl.ds, x0[0], P.dt, P.N, nx, P.x_ref + (size_t)b * nx * P.N);
}

}  // namespace

hipError_t plan_profile_launch(const PlanProfileParams& P, const double* par, int par_stride, hipStream_t st) {
  return plan_profile_kernel_launch<false>(P, (size_t)2 * sizeof(double) * (size_t)P.N_s, par, par_stride, st);
}
hipError_t plan_reference_launch(const PlanRefParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  hipLaunchKernelGGL(plan_reference_kernel, dim3((P.batch + 63) / 64), dim3(64), 0, st, P);
  return hipGetLastError();
}
hipError_t cl_pre_plan_launch(const ClPrePlanParams& P, hipStream_t st) {
  if (P.batch == 0) return hipSuccess;
  hipLaunchKernelGGL(cl_pre_plan_kernel, dim3((P.batch + 63) / 64), dim3(64), 0, st, P);
  return hipGetLastError();
}
