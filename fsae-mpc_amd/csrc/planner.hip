// planner.hip -- the s-domain plan the closed loop tracks, batched on the device.
//
//   plan_profile_kernel    a quasi-steady-state minimum-time speed profile on the centre line, the stand-in for the table
//                          dynamic_minimum_time_planner.m produces (main.m:20; the planner itself needs IPOPT): curvature of the
//                          spline table per cell, the grip-limited corner speed, one forward and one backward pass under the
//                          longitudinal limit the controller's own QP rows carry, then the 8 planner values and the traversal
//                          time of each cell.  One wavefront per plan: the cells are dealt to the lanes for the parallel phases,
//                          curvature and speed sit in LDS, lane 0 runs the two recurrences.
//   plan_reference_kernel  util/obtain_reference.m:5-48 in the state layout of the model, batched over s0 (one thread per car),
//                          on a plan shared by the batch or given per car
//   cl_pre_plan_kernel     cl_pre_kernel (plant.hip) with the live ramp of main.m:107-114 replaced by main.m:115: frame
//                          transform, x0 assembly, lap check, out-of-race rule, then the walk from the car's own s
#include <hip/hip_runtime.h>
#include <math.h>
#include "planner.h"
#include "mpc_params.h"
#include "cl_frame.h"   // (compiled as in plant.hip: the pragma below comes after it)

// plain IEEE operations in source order (no FMA contraction): the profile is restated operation for operation in numpy
// (tests/plan_numpy.py), the walk is compared bit for bit with the oracle
#pragma clang fp contract(off)

namespace {

// Largest longitudinal acceleration at speed v in a cell of curvature magnitude K.
//   kinematic: the input box scaled by grip (with the soft +-ALAT_MAX rows a rectangle)
//   dynamic:   the boundary of the inscribed 12-gon of dynamic_tyre_linearise_constraints.m:18-23 in the first quadrant, at the
//              lateral share y = v^2 K / A_lat, capped by the input box.  The polygon is what the tyre rows enforce, and unlike the
//              ellipse it is Lipschitz at the apex.
template <bool DYN, class PAR> DEVINL double plan_ax(const PAR& p, double v, double K, double A_lat, double grip) {
  if constexpr (!DYN) {
    return grip * p.U_ACC_MAX;
  } else {
    const double y = fmin(v * v * K / A_lat, 1.0);
    double c0 = 1.0, c1 = 0.8660254037844386, s0 = 0.0, s1 = 0.5;                        // edge 0
    if (!(y <= 0.5)) { c0 = 0.8660254037844386; c1 = 0.5; s0 = 0.5; s1 = 0.8660254037844386; }   // edge 1
    if (!(y <= 0.8660254037844386)) { c0 = 0.5; c1 = 0.0; s0 = 0.8660254037844386; s1 = 1.0; }   // edge 2
    const double X = c0 + (c1 - c0) * (y - s0) / (s1 - s0);
    return fmin(p.U_ACC_MAX, grip * p.ELL_LONG * X);
  }
}

template <bool DYN, class PAR> __global__ void __launch_bounds__(64) plan_profile_kernel(PlanProfileParams P, typename PAR::Args pa) {
  extern __shared__ double lds[];
  const int plan = blockIdx.x, lane = threadIdx.x, Ns = P.N_s;
  double* kq = lds;            // Ns signed curvatures
  double* vq = lds + Ns;       // Ns speeds
  double* tab = P.table + (size_t)plan * Ns * 8;
  double* tt = P.t + (size_t)plan * Ns;
  const PAR p = par_get<PAR>(pa, plan);
  if (p.bad) {   // (uniform over the wave) a block that cannot describe a car: this plan is NaN, the others are unaffected
    for (int i = lane; i < Ns; i += 64) {
      tt[i] = NAN;
      for (int c = 0; c < 8; ++c) tab[(size_t)i * 8 + c] = NAN;
    }
    return;
  }
  const Spl sp{P.spM, P.spdl, P.xP, P.yP};
  const double ds = P.ds, grip = P.grip;
  const double A_lat = grip * (DYN ? p.ELL_LAT : p.ALAT_MAX);

  // curvature and grip-limited corner speed of every cell; each lane keeps the first minimum among its cells
  double best = INFINITY; int ibest = 0x7fffffff;
  for (int i = lane; i < Ns; i += 64) {
    const double k = kappa(sp, (double)i * ds);
    const double K = fmax(fabs(k), 1e-12);
    const double vl = fmin(P.v_cap, sqrt(A_lat / K));
    kq[i] = k; vq[i] = vl;
    if (vl < best) { best = vl; ibest = i; }
  }
  // first index of the minimum over the wave (every lane takes part; a tie goes to the lower index)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ob = __shfl_xor(best, m, 64);
    const int oi = __shfl_xor(ibest, m, 64);
    if (ob < best || (ob == best && oi < ibest)) { best = ob; ibest = oi; }
  }
  const int i0 = ibest < Ns ? ibest : 0;   // (no cell compared below infinity: a table of NaN; any start will do)
  __syncthreads();

  if (lane == 0) {   // the two recurrences; since vlat[i0] is the global minimum, one pass each way closes the lap
    double vp = vq[i0]; int i = i0;
    for (int j = 1; j <= Ns; ++j) {                 // forward: acceleration out of the slower predecessor
      const int pr = i;
      i = i + 1; if (i >= Ns) i = 0;
      const double Kp = fmax(fabs(kq[pr]), 1e-12);
      const double a = plan_ax<DYN>(p, vp, Kp, A_lat, grip);
      const double v = fmin(vq[i], sqrt(vp * vp + 2.0 * a * ds));
      vq[i] = v; vp = v;
    }
    vp = vq[i0]; i = i0;
    for (int j = 1; j <= Ns; ++j) {                 // backward: braking into the slower successor
      const int nx = i;
      i = i - 1; if (i < 0) i = Ns - 1;
      const double Kn = fmax(fabs(kq[nx]), 1e-12);
      const double a = plan_ax<DYN>(p, vp, Kn, A_lat, grip);
      const double v = fmin(vq[i], sqrt(vp * vp + 2.0 * a * ds));
      vq[i] = v; vp = v;
    }
  }
  __syncthreads();

  for (int i = lane; i < Ns; i += 64) {   // the planner's 8 values per cell and the cell's traversal time (cyclic successor)
    const int n = i + 1 < Ns ? i + 1 : 0;
    const double v = vq[i], vn = vq[n], k = kq[i], kn = kq[n];
    const double delta = atan(p.WB * k), delta_n = atan(p.WB * kn);
    const double ti = ds / v;                        // the reference's ds / s_d (dynamic_minimum_time_planner.m:73-83)
    double* row = tab + (size_t)i * 8;
    row[0] = 0.0; row[1] = 0.0; row[2] = v; row[3] = 0.0; row[4] = v * k; row[5] = delta;
    row[6] = (vn * vn - v * v) / (2.0 * ds);
    row[7] = (delta_n - delta) / ti;
    tt[i] = ti;
  }
}

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

template <bool DYN> hipError_t profile_launch(const PlanProfileParams& P, const double* par, int par_stride, hipStream_t st) {
  const size_t lds = (size_t)2 * sizeof(double) * (size_t)P.N_s;
  if (par) hipLaunchKernelGGL((plan_profile_kernel<DYN, RtPar>), dim3(P.n_plans), dim3(64), lds, st, P, ParArgs{par, par_stride, nullptr});
  else hipLaunchKernelGGL((plan_profile_kernel<DYN, FixedPar>), dim3(P.n_plans), dim3(64), lds, st, P, NoParArgs{});
  return hipGetLastError();
}

}  // namespace

hipError_t plan_profile_launch(const PlanProfileParams& P, const double* par, int par_stride, hipStream_t st) {
  if (P.n_plans == 0) return hipSuccess;
  return P.dynamic ? profile_launch<true>(P, par, par_stride, st) : profile_launch<false>(P, par, par_stride, st);
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
